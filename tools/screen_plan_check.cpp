// screen_plan_check.cpp -- the pure functions the reference screen adds to csrc/sdt_read_plan.h, on the CPU: every refusal of the
// parameters and their boundaries; the size of the set's table and which forced sizes hold a set; the rule of a read at its boundaries;
// and the unit verdicts of the kept form against a walk over every ordinal, on random pair ranges, presence and records.
// Stand-alone, meant for a sanitizer build:
//   g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o screen_plan_check tools/screen_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd(uint64_t n)
{
	rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17;
	return n ? rnd_state % n : 0;
}

// the verdicts once more: per ordinal, is it in a range, which one is its mate, is the mate there
static uint64_t by_walk(std::vector<ScreenRec> &rec, const std::vector<uint8_t> &present, const std::vector<uint64_t> &ranges, const ScreenParams &p)
{
	const uint64_t n = rec.size();
	std::vector<int> matched(n, 0), unit(n, 0);
	for (uint64_t o = 0; o < n; o++)
		matched[o] = present[o] && rec[o].hits >= (p.min_hits ? p.min_hits : 1) && 100ULL * rec[o].hits >= (uint64_t)p.min_hit_pct * rec[o].kmers;
	for (uint64_t o = 0; o < n; o++) {
		uint64_t mate = n;
		for (size_t i = 0; i + 1 < ranges.size(); i += 2)
			if (o >= ranges[i] && o < ranges[i + 1]) mate = ((o - ranges[i]) & 1) ? o - 1 : o + 1;
		unit[o] = matched[o] || (mate < n && present[mate] && matched[mate]);
	}
	uint64_t kept = 0;
	for (uint64_t o = 0; o < n; o++) {
		if (!present[o]) continue;
		const bool dropped = (p.flags & SCREEN_KEEP_MATCHED) ? !unit[o] : unit[o];
		rec[o].start = 0;
		rec[o].verdict = dropped;
		if (dropped) rec[o].len = 0; else kept++;
	}
	return kept;
}

int main()
{
	// ---- the parameters ----
	CHECK(check_screen_params(ScreenParams{1, 0, 0, 0}) == SCREEN_OK && check_screen_params(ScreenParams{0, 100, SCREEN_KEEP_MATCHED, 0}) == SCREEN_OK);
	CHECK(check_screen_params(ScreenParams{0xFFFFFFFFu, 100, 1, 0}) == SCREEN_OK);
	CHECK(check_screen_params(ScreenParams{1, 101, 0, 0}) == SCREEN_MIN_HIT_PCT && check_screen_params(ScreenParams{1, 0xFFFFFFFFu, 0, 0}) == SCREEN_MIN_HIT_PCT);
	CHECK(check_screen_params(ScreenParams{1, 0, 2, 0}) == SCREEN_FLAGS && check_screen_params(ScreenParams{1, 0, 3, 0}) == SCREEN_FLAGS);
	CHECK(check_screen_params(ScreenParams{1, 0, SCREEN_PER_READ, 0}) == SCREEN_FLAGS);              // the internal bit is never a caller's
	CHECK(check_screen_params(ScreenParams{1, 0, 0, 1}) == SCREEN_RESERVED);
	CHECK(check_screen_params(ScreenParams{1, 101, 2, 1}) == SCREEN_MIN_HIT_PCT && check_screen_params(ScreenParams{1, 100, 2, 1}) == SCREEN_FLAGS);   // the first that fails

	// ---- the table ----
	CHECK(screen_table_slots(0) == 1024 && screen_table_slots(1) == 1024 && screen_table_slots(512) == 1024 && screen_table_slots(513) == 2048);
	CHECK(screen_table_slots(31500) == 65536 && screen_table_slots(1ULL << 40) == 1ULL << 41 && screen_table_slots((1ULL << 40) + 1) == 1ULL << 42);
	for (uint64_t n = 1; n < 5000; n += 7) {
		const uint64_t s = screen_table_slots(n);
		CHECK(!(s & (s - 1)) && s >= 2 * n && (s == 1024 || s / 2 < 2 * n));
	}
	CHECK(screen_forced_slots_ok(32768, 31500) && !screen_forced_slots_ok(30000, 100) && !screen_forced_slots_ok(16384, 16384) && screen_forced_slots_ok(16384, 16383));
	CHECK(!screen_forced_slots_ok(0, 0) && screen_forced_slots_ok(1, 0));
	const uint64_t offs[] = {7, 7, 17, 28, 40, 40, 1040};                                           // lengths 0, 10, 11, 12, 0, 1000
	CHECK(screen_positions(offs, 6, 11) == 0 + 0 + 1 + 2 + 0 + 990 && screen_positions(offs, 6, 31) == 970 && screen_positions(offs, 0, 11) == 0);
	CHECK(screen_positions(offs, 2, 11) == 0);

	// ---- a read ----
	const ScreenParams one = {1, 0, 0, 0}, zero = {0, 0, 0, 0}, three = {3, 0, 0, 0}, pct = {1, 37, 0, 0}, all = {1, 100, 0, 0};
	CHECK(!screen_read_matched(100, 0, one) && screen_read_matched(100, 1, one) && !screen_read_matched(100, 0, zero) && screen_read_matched(100, 1, zero));
	CHECK(!screen_read_matched(100, 2, three) && screen_read_matched(100, 3, three));
	CHECK(screen_read_matched(100, 37, pct) && !screen_read_matched(100, 36, pct) && !screen_read_matched(101, 37, pct));
	CHECK(screen_read_matched(5, 5, all) && !screen_read_matched(5, 4, all) && !screen_read_matched(0, 0, all));
	CHECK(screen_read_matched(0xFFFFFFFFull, 0xFFFFFFFFull, all) && !screen_read_matched(0xFFFFFFFFull, 0xFFFFFFFEull, all));   // 64 bits
	CHECK(screen_unit_dropped(true, 0) && !screen_unit_dropped(false, 0) && !screen_unit_dropped(true, 1) && screen_unit_dropped(false, 1));

	// ---- the kept form: random ranges, presence and records against the walk ----
	for (int round = 0; round < 400; round++) {
		const uint64_t n = rnd(60);
		std::vector<uint64_t> ranges;
		for (uint64_t at = rnd(5); at < n + 6 && ranges.size() < 8;) {
			const uint64_t len = 2 * rnd(6);
			ranges.push_back(at);
			ranges.push_back(at + len);                                                          // (may end past n, may be empty)
			at += len + rnd(4);
		}
		PairRangeFault fault;
		CHECK(check_pair_ranges(ranges.data(), ranges.size() / 2, &fault) == ranges.size() / 2 && fault == PAIR_RANGES_OK);
		const ScreenParams p = {(uint32_t)rnd(4), (uint32_t)rnd(3) * 50, (uint32_t)rnd(2), 0};
		std::vector<ScreenRec> rec(n), want;
		std::vector<uint8_t> present(n);
		for (uint64_t o = 0; o < n; o++) {
			present[o] = rnd(4) != 0;
			const uint32_t kmers = (uint32_t)rnd(6), hits = (uint32_t)rnd(kmers + 1);
			rec[o] = ScreenRec{kmers, hits, hits ? (uint32_t)rnd(3) : SCREEN_NO_REF, 99, kmers + 20, 99};
		}
		want = rec;
		const uint64_t kept_want = by_walk(want, present, ranges, p);
		const uint64_t kept = screen_unit_verdicts(rec.data(), present.data(), n, ranges.data(), ranges.size() / 2, p);
		CHECK(kept == kept_want);
		for (uint64_t o = 0; o < n; o++) {
			const ScreenRec &a = rec[o], &b = want[o];
			CHECK(a.kmers == b.kmers && a.hits == b.hits && a.ref == b.ref && a.start == b.start && a.len == b.len && a.verdict == b.verdict);
			if (!present[o]) CHECK(a.start == 99 && a.verdict == 99);                            // not looked at
		}
	}
	// no ordinals, no ranges
	const ScreenParams p0 = {1, 0, 0, 0};
	CHECK(screen_unit_verdicts(nullptr, nullptr, 0, nullptr, 0, p0) == 0);

	if (failures) { fprintf(stderr, "screen_plan_check: %d checks failed\n", failures); return 1; }
	printf("screen_plan_check: ok\n");
	return 0;
}
