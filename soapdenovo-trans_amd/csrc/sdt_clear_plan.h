// sdt_clear_plan.h -- how much of the node table's clear debt one launch of the level-1 scatter takes along, as a PURE function
// (the idiom of sdt_count_plan.h and sdt_read_plan.h).  sdt_gpu_reset does not clear the table: it notes that the slots [lo, hi) still
// have to be cleared (sdt_ctx.hpp: clear_lo / clear_hi).  A fused launch of k_sk_scatter_reads_seq stores the clear pattern of a few
// UNITS of slots at the top of every tile; what the cap per tile or a ragged last unit leaves over stays debt, for the next launch
// or for settle_clear's k_clear.  sk_scatter_launch (sdt_pipeline.hip) calls this; tools/clear_plan_check.cpp (tests/test_clear_plan.py)
// calls it on the CPU under sanitizers.  No HIP in here.
#pragma once
#include <stdint.h>

namespace sdt {

// A unit is a power-of-two number of slots whose pieces of all three arrays are whole 64-byte blocks: 256 slots are 4 KiB of 16-byte
// entries (one 16-byte store per lane of a workgroup of 256), 1 KiB of `aux` and 2 KiB of `first`.
constexpr uint32_t CLEAR_UNIT_SLOTS = 256;
// what a tile stores at most: a launch of a few tiles must not turn into a slow clear kernel
constexpr uint64_t CLEAR_TILE_CAP_BYTES = 128 * 1024;

constexpr uint32_t clear_cap_units(uint64_t bytes_per_slot)
{
	return (uint32_t)(CLEAR_TILE_CAP_BYTES / (bytes_per_slot * CLEAR_UNIT_SLOTS));
}

struct ClearPlan {
	uint32_t units_per_tile;       // tile t of the launch stores units [t * units_per_tile, (t + 1) * units_per_tile) of the range, clipped at its end
	uint64_t lo, hi;               // the slots the launch covers: lo = debt_lo, hi - lo a whole number of units (lo == hi: nothing)
};

// debt [debt_lo, debt_hi), `tiles` tiles in the launch, units of `unit` slots (a power of two; debt_lo must be a multiple of it,
// as it is when every earlier launch was planned here), at most `cap` units per tile.  The units are spread over ALL tiles -- the
// stores are meant to drain under the walk of the tile that issued them -- so units_per_tile is the quotient rounded up and the last
// tiles may find less than their share, or nothing, left.
inline ClearPlan plan_clear(uint64_t debt_lo, uint64_t debt_hi, uint64_t tiles, uint32_t unit, uint32_t cap)
{
	ClearPlan p = {0, debt_lo, debt_lo};
	if (debt_hi <= debt_lo || tiles == 0 || unit == 0 || (unit & (unit - 1)) || cap == 0 || (debt_lo & (uint64_t)(unit - 1)))
		return p;
	const uint64_t units = (debt_hi - debt_lo) / unit;       // (whole units only: a ragged end is the host's)
	if (units == 0)
		return p;
	const uint64_t share = units / tiles + (units % tiles != 0);
	uint64_t covered = units;
	if (share > (uint64_t)cap) {                             // (then cap * tiles < units: no overflow)
		p.units_per_tile = cap;
		covered = (uint64_t)cap * tiles;
	} else {
		p.units_per_tile = (uint32_t)share;
	}
	p.hi = debt_lo + covered * unit;
	return p;
}

} // namespace sdt
