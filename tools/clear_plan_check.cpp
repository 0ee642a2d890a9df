// clear_plan_check.cpp -- CPU: how much of the node table's clear debt a launch of the level-1 scatter takes along (csrc/sdt_clear_plan.h):
//   * what the launch covers + what it leaves = the debt, for every combination of slot counts (whole units, ragged ends, fewer slots
//     than a unit, counts past 2^32 and near 2^63), tile counts (none, one, fewer than units, more than units, a workload's) and caps;
//   * units_per_tile is the share rounded up, the cap at most, and 0 only where nothing is covered; the covered range starts at the debt,
//     is whole units and never passes the debt's end -- so the stores of tile t, units [t * units_per_tile, + units_per_tile) clipped at
//     the range's end (replayed here tile by tile for the small cases), write every covered slot once and no other;
//   * a sequence of launches carries the debt down to the ragged end and no further;
//   * the unit: entry, aux and first pieces of CLEAR_UNIT_SLOTS slots are whole 64-byte blocks, and the cap per tile is about 128 KB.
// Built with -fsanitize=address,undefined by tests/test_clear_plan.py.  Prints "clear_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include "../soapdenovo-trans_amd/csrc/sdt_clear_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("clear_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

typedef unsigned long long ull;

static uint64_t plans = 0;

// one plan against the rules; returns what it covers
static uint64_t check_plan(uint64_t lo, uint64_t hi, uint64_t tiles, uint32_t unit, uint32_t cap)
{
	const ClearPlan p = plan_clear(lo, hi, tiles, unit, cap);
	plans++;
	const uint64_t debt = hi > lo ? hi - lo : 0, units = debt / unit;
	CHECK(p.lo == lo && p.hi >= p.lo && p.hi <= (hi > lo ? hi : lo), "debt [%llu, %llu): covers [%llu, %llu)", (ull)lo, (ull)hi, (ull)p.lo, (ull)p.hi);
	const uint64_t covered = p.hi - p.lo, left = debt - covered;
	CHECK(covered % unit == 0, "covered %llu slots are not whole units of %u", (ull)covered, unit);
	CHECK(covered + left == debt, "covered + remainder != debt");
	CHECK(p.units_per_tile <= cap, "%u units per tile, cap %u", p.units_per_tile, cap);
	CHECK((covered == 0) == (p.units_per_tile == 0), "covered %llu with %u units per tile", (ull)covered, p.units_per_tile);
	if (tiles == 0 || units == 0) {
		CHECK(covered == 0, "nothing to cover, covered %llu", (ull)covered);
		return 0;
	}
	// the share rounded up, capped; units per tile times tiles, clipped at the whole units of the debt, is what is covered
	const uint64_t share = units / tiles + (units % tiles != 0);
	CHECK(p.units_per_tile == (share < cap ? share : cap), "%llu units over %llu tiles, cap %u: %u per tile", (ull)units, (ull)tiles, cap, p.units_per_tile);
	const unsigned __int128 reach = (unsigned __int128)p.units_per_tile * tiles;
	CHECK(covered / unit == (reach < units ? (uint64_t)reach : units), "covered %llu units of %llu", (ull)(covered / unit), (ull)units);
	// the remainder is the ragged end alone unless the cap cut the launch short
	if (share <= cap)
		CHECK(left == debt % unit, "no cap in the way, yet %llu slots are left of %llu", (ull)left, (ull)debt);
	else
		CHECK(left == debt - (uint64_t)cap * tiles * unit, "capped: %llu left", (ull)left);
	return covered;
}

// the kernel's tile loop (sk_clear_tile of sdt_sk_scatter_seq.cuh) on a table of bytes: every covered slot once, nothing else
static void replay_tiles(uint64_t lo, uint64_t hi, uint64_t slots, uint64_t tiles, uint32_t unit, uint32_t cap)
{
	const ClearPlan p = plan_clear(lo, hi, tiles, unit, cap);
	unsigned char *hit = (unsigned char *)calloc(slots ? slots : 1, 1);       // (exactly the table: a store past it is a finding)
	CHECK(hit, "calloc");
	const uint64_t unit0 = p.lo / unit, unit_end = p.hi / unit;
	for (uint64_t t = 0; t < tiles; t++) {
		const uint64_t u0 = unit0 + t * p.units_per_tile;
		if (u0 >= unit_end)
			continue;
		const uint64_t left = unit_end - u0, n = left < p.units_per_tile ? left : p.units_per_tile;
		for (uint64_t s = u0 * unit; s < (u0 + n) * unit; s++)
			hit[s]++;
	}
	for (uint64_t s = 0; s < slots; s++)
		CHECK(hit[s] == (s >= p.lo && s < p.hi ? 1 : 0), "slot %llu of %llu written %d times (covered [%llu, %llu), %llu tiles)", (ull)s, (ull)slots,
		      hit[s], (ull)p.lo, (ull)p.hi, (ull)tiles);
	free(hit);
}

int main(void)
{
	// the unit and the cap
	static_assert((CLEAR_UNIT_SLOTS & (CLEAR_UNIT_SLOTS - 1)) == 0, "a power of two");
	static_assert(CLEAR_UNIT_SLOTS * 16 % 64 == 0 && CLEAR_UNIT_SLOTS * 32 % 64 == 0 && CLEAR_UNIT_SLOTS * 4 % 64 == 0 && CLEAR_UNIT_SLOTS * 8 % 64 == 0,
	              "entry, aux and first pieces are whole 64-byte blocks");
	static_assert(CLEAR_UNIT_SLOTS * 16 == 256 * 16, "one 16-byte store per lane of a workgroup of 256 covers a unit's 1-word entries");
	CHECK(clear_cap_units(20) == 25 && clear_cap_units(28) == 18 && clear_cap_units(36) == 14 && clear_cap_units(44) == 11, "cap units per tile");
	for (const uint64_t per_slot : {(uint64_t)20, (uint64_t)28, (uint64_t)36, (uint64_t)44}) {
		const uint64_t bytes = (uint64_t)clear_cap_units(per_slot) * CLEAR_UNIT_SLOTS * per_slot;
		CHECK(bytes <= 128 * 1024 && bytes > 112 * 1024, "%llu bytes per tile at %llu per slot", (ull)bytes, (ull)per_slot);
	}

	static const uint64_t slot_counts[] = {0, 1, 255, 256, 257, 511, 512, 65536, 65536 + 16, 66672, 1ULL << 22, (1ULL << 22) + 4095, 1800000000ULL,
	                                       (1ULL << 32) - 1, 1ULL << 32, (1ULL << 32) + 1, (1ULL << 32) + 256 + 17, 1ULL << 40, (1ULL << 62) + 12345};
	static const uint64_t tile_counts[] = {0, 1, 2, 3, 15, 16, 17, 255, 256, 257, 4096, 781250, 1ULL << 33, ~0ULL >> 8};
	static const uint32_t caps[] = {1, 11, 14, 18, 25, 1000};
	for (const uint64_t slots : slot_counts)
		for (const uint64_t tiles : tile_counts)
			for (const uint32_t cap : caps) {
				check_plan(0, slots, tiles, CLEAR_UNIT_SLOTS, cap);
				// a debt that earlier launches have shortened: any whole number of units in
				for (const uint64_t done_units : {(uint64_t)1, (uint64_t)7, slots / CLEAR_UNIT_SLOTS})
					if (done_units * CLEAR_UNIT_SLOTS <= slots)
						check_plan(done_units * CLEAR_UNIT_SLOTS, slots, tiles, CLEAR_UNIT_SLOTS, cap);
				if (slots <= 70000 && tiles <= 4096) {
					replay_tiles(0, slots, slots, tiles, CLEAR_UNIT_SLOTS, cap);
					if (slots >= 512)
						replay_tiles(256, slots, slots, tiles, CLEAR_UNIT_SLOTS, cap);
				}
			}
	// other units
	for (const uint32_t unit : {1u, 16u, 1024u, 1u << 20})
		for (const uint64_t slots : slot_counts)
			for (const uint64_t tiles : tile_counts)
				check_plan(0, slots, tiles, unit, 25);
	// refused: a debt that does not start on a unit, a unit that is no power of two, no cap
	CHECK(plan_clear(17, 1 << 20, 100, 256, 25).hi == 17 && plan_clear(0, 1 << 20, 100, 100, 25).hi == 0 && plan_clear(0, 1 << 20, 100, 256, 0).hi == 0 &&
	      plan_clear(0, 1 << 20, 100, 0, 25).hi == 0 && plan_clear(512, 256, 100, 256, 25).hi == 512, "refusals cover nothing");

	// the flagship: 1.8 G slots over 781 250 tiles take 9 units a tile -- 46 KB, eleven to twelve 16-byte stores per lane -- and all of it
	{
		const uint64_t slots = 1799999488ULL;                // (a multiple of 4096 near 0.68 G nodes at a load of 45 %)
		const ClearPlan p = plan_clear(0, slots, 781250, CLEAR_UNIT_SLOTS, clear_cap_units(20));
		CHECK(p.units_per_tile == 9 && p.hi == slots, "flagship: %u units per tile, covers %llu of %llu", p.units_per_tile, (ull)p.hi, (ull)slots);
	}
	// launches one after the other carry the debt down to the ragged end: three pushes of 6, 5 and 5 tiles into 2^22 + 100 slots, then as
	// many as it takes
	{
		const uint64_t slots = (1ULL << 22) + 100;
		uint64_t lo = 0, launches = 0;
		for (const uint64_t tiles : {(uint64_t)6, (uint64_t)5, (uint64_t)5}) {
			const uint64_t got = check_plan(lo, slots, tiles, CLEAR_UNIT_SLOTS, 25);
			CHECK(got == tiles * 25 * CLEAR_UNIT_SLOTS, "a capped launch of %llu tiles covered %llu", (ull)tiles, (ull)got);
			lo += got;
		}
		while (check_plan(lo, slots, 16, CLEAR_UNIT_SLOTS, 25)) {
			lo += plan_clear(lo, slots, 16, CLEAR_UNIT_SLOTS, 25).hi - lo;
			launches++;
			CHECK(launches < 1000, "the debt does not shrink");
		}
		CHECK(slots - lo == 100, "%llu slots left for the host, the ragged end has 100", (ull)(slots - lo));
	}
	printf("clear_plan_check: ok (%llu plans)\n", (ull)plans);
	return 0;
}
