// sdt_layout_plan.h -- the growth schedule of the layout replay as a PURE host function of the sizes of the sets.
//
// The reference puts the keys of a set into its KmerSet one after the other (first occurrence ascending); a put that finds
// count + 1 > max grows the table first (encap_kmerset, newhash.c:318-330) and rehashes it in place.  When a set grows, and to what
// size, depends on its number of keys only:
//   * a set starts with next_prime(1024) = 1031 slots, 3 in the variants of more than one word under small_init (init_kmerset,
//     prlHashReads.c:402-423, newhash.c:163-166), and max = (ubyte8)(size * 0.77f);
//   * a growth doubles the size below 2^28 - 1 slots and adds 2^24 - 1 past that, then takes the next "prime" of
//     find_next_prime_kh (newhash.c:116-158: the bound of its trial division is (ubyte8)sqrt((float)n), exclusive), until
//     size * load_factor holds count + 1, load_factor being the float 0.77f widened to double;
//   * generation g of a set: the ids [lo, hi) that are put into its table of `size` slots after the growth from generation g - 1.
// The float / double arithmetic decides whether the device's visiting order equals the reference's: it stays as it is, literally.
// sdt_gpu_layout_on_device (sdt_gpu_graph.hip) replays the generations of all sets side by side; graph.c has its own copy of the rule.
// tools/layout_plan_check.cpp checks this header on the CPU (tests/test_layout_plan_host.py).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace sdt {

constexpr int RP_PLAN_DEPTH_BITS = 6;            // = RP_DEPTH_BITS (sdt_graph_kernels.cuh): bits of the depth in an insertion time
constexpr uint32_t RP_PLAN_CHUNK = 256;          // = AP_CH (sdt_append.cuh): entries of a chunk of a round's list
constexpr uint32_t RP_PLAN_WAVES = 4;            // = TPB / 64: waves of a workgroup, each with an open chunk

// RP_PLAN_SLOTS: a set's table passes 2^32 slots; RP_PLAN_BITS: twice the slot bits do not fit the table word (or the sets the list entry)
enum RpPlanStatus { RP_PLAN_OK = 0, RP_PLAN_SLOTS, RP_PLAN_BITS };

struct RpGen { uint32_t lo, hi, size; };         // ids [lo, hi) are put into a table of `size` slots (after a growth from the previous size)

struct RpSchedule {
	std::vector<std::vector<RpGen>> gens;        // per set; never empty (a set without keys has the generation [0, 0))
	std::vector<uint64_t> tab0;                  // per set: first slot of its region in the table buffers (regions of the final sizes)
	uint64_t tab_total = 0, max_size = 0;        // slots of all regions; the largest final size
	size_t max_gens = 0;
	int qbits = 1;                               // bits of (slot + 1) in the table word of a growth's rounds: time << qbits | q + 1
};

inline int rp_prime(uint64_t num)                    // find_next_prime_kh's test (newhash.c:116-158): the bound is (ubyte8)sqrt((float)n)
{
	if (num < 4) return 1;
	if (num % 2 == 0) return 0;
	const uint64_t lim = (uint64_t)sqrt((float)num);
	for (uint64_t i = 3; i < lim; i += 2)
		if (num % i == 0) return 0;
	return 1;
}
inline uint64_t rp_next_prime(uint64_t n) { if (n % 2 == 0) n++; while (!rp_prime(n)) n += 2; return n; }
inline uint64_t rp_next_size(uint64_t size, double lf, uint64_t count)      // encap_kmerset's growth (newhash.c:318-330)
{
	uint64_t n = size;
	do {
		n = n < 0xFFFFFFFu ? n << 1 : n + 0xFFFFFFu;
		n = rp_next_prime(n);
	} while (n * lf < (double)(count + 1));
	return n;
}

// the schedule of p sets of set_size[s] keys each; on RP_PLAN_BITS out.qbits is what did not fit
inline RpPlanStatus rp_schedule(const uint64_t *set_size, int p, int nw_variant, int small_init, RpSchedule &out)
{
	out = RpSchedule();
	out.gens.resize(p);
	out.tab0.resize(p);
	const double lf = (double)0.77f;
	for (int s = 0; s < p; s++) {
		const uint64_t ms = set_size[s];
		uint64_t size = (nw_variant != 1 && small_init) ? 3 : rp_next_prime(1024);
		uint64_t max = (uint64_t)(size * 0.77f), lo = 0;
		for (;;) {
			const uint64_t hi = ms < max ? ms : max;
			out.gens[s].push_back(RpGen{(uint32_t)lo, (uint32_t)hi, (uint32_t)size});
			if (hi >= ms) break;
			size = rp_next_size(size, lf, max);                // the put of id == max finds count + 1 > max
			if (size >= 0xFFFFFFFFULL) return RP_PLAN_SLOTS;
			lo = hi;
			max = (uint64_t)(size * lf);
		}
		out.tab0[s] = out.tab_total;
		out.tab_total += size;
		if (size > out.max_size) out.max_size = size;
		if (out.gens[s].size() > out.max_gens) out.max_gens = out.gens[s].size();
	}
	// table word of a growth's rounds: time << qbits | q + 1 (q = old slot, time = old slot << depth bits | depth); a dirty cluster's
	// list entry keeps the set in 10 bits
	while ((1ULL << out.qbits) <= out.max_size) out.qbits++;
	if (2 * out.qbits + RP_PLAN_DEPTH_BITS > 64 || p >= 1024) return RP_PLAN_BITS;
	return RP_PLAN_OK;
}

// chunks of one of the two lists of a growth's rounds.  A round lists the entries whose time changed: a fifth of the entries of a growth
// in round 0 (tools/replay_fixed_point.c), i.e. an eighth of all keys when the largest set grows; room for a quarter of all n keys (past
// that: SDT_ELIMIT, the caller replays on the host).  A closed chunk holds more than RP_PLAN_CHUNK - 64 entries, every wave has an open one
inline unsigned long long rp_list_chunks(uint64_t n, int cu_count)
{
	const uint64_t m = n ? n : 1;
	return (m / 4 + 1) / (RP_PLAN_CHUNK - 64) + 1 + (unsigned long long)cu_count * 8 * RP_PLAN_WAVES;
}

} // namespace sdt
