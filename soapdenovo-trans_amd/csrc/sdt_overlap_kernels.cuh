// sdt_overlap_kernels.cuh -- the overlap of the two mates of a pair found on the device, and what lies past the fragment's end
// clipped without an adapter list (the rule: include/sdt_gpu.h).  Needs no table and no LDS; every pair is decided on its own by one
// wavefront:
//   k_overlap_pairs : mate b reverse-complemented (b') is laid under mate a at every shift d whose overlap can reach min_overlap:
//                     lane j takes d = d_first + 64 step + j, steps ascending.  The lane walks its columns 32 at a time: the 32 bases
//                     of a as one 64-bit window (read_window), the 32 bases of b' as the window of b that ENDS where b' starts
//                     (read_window_end), turned round in registers (overlap_rc_window); one XOR compares 32 bases, a pair of bits
//                     that differs is a mismatch, counted by a popcount and masked to the columns left.  The lane leaves its shift as
//                     soon as the mismatches pass the budget of the whole shift: on unrelated sequence after the first window.  Every
//                     lane keeps the best admissible (score, d) of its own shifts; one wave reduction at the end finds the pair's.
//                     Lane 0 writes both records and both keep bytes.
// A unit that is a single read (the kept form: an ordinal outside every pair range, a pair of which one mate is not kept) gets the
// record of a pair without overlap.  Every loop is bounded by La + Lb or by the overlap; no lane waits for another, the matching uses
// no atomics; one atomic per wavefront counts the reads kept.
#pragma once
#include "sdt_clip_kernels.cuh"

namespace sdt {

struct ReadOverlap {                                     // == sdt_read_overlap of include/sdt_gpu.h
	uint32_t overlap, mismatches, insert, start, len, verdict;
};
static_assert(sizeof(ReadOverlap) == 24, "sdt_read_overlap is six 32-bit words");

constexpr uint32_t OVERLAP_ABSENT = 0xFFFFFFFFu;         // verdict of a record that no read has written (kept form: the array is preset)
constexpr uint64_t PAIR_HIGH = 0xAAAAAAAAAAAAAAAAULL;

// A window of read_window_end (the LAST base in the least significant pair) as the same bases reverse-complemented, the first of them
// in the most significant pair: the 64 bits reversed, the two bits of every pair swapped back, every code x turned into x ^ 2.
// Pairs that held no base (before the read's start) come out as code 2 at the window's end: the caller masks them.
__device__ inline uint64_t overlap_rc_window(uint64_t w)
{
	const uint64_t r = __brevll(w);
	return (((r & PAIR_HIGH) >> 1) | ((r & PAIR_LOW) << 1)) ^ PAIR_HIGH;
}

// the record of a read of L bases in a pair whose overlap is (o, h, F); F == 0: none
__device__ inline ReadOverlap overlap_record(uint64_t L, uint64_t o, uint64_t h, uint64_t F, uint32_t min_len)
{
	const uint64_t len = F && F < L ? F : L;
	ReadOverlap rec = {(uint32_t)o, (uint32_t)h, (uint32_t)F, 0u, (uint32_t)len, CLIP_CLIPPED};
	if (len < (min_len > 1 ? min_len : 1u)) { rec.len = 0; rec.verdict = CLIP_DROPPED; }
	else if (len == L) rec.verdict = CLIP_WHOLE;
	return rec;
}

template <class Reads>
static __global__ __launch_bounds__(TPB) void k_overlap_pairs(Reads reads, Units U, OverlapParams P, ReadOverlap *__restrict__ ov,
                                                              uint8_t *__restrict__ keep, unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t mine = 0;
	for (uint64_t u = blockIdx.x * (uint64_t)(TPB / 64) + wave; u < U.n; u += (uint64_t)gridDim.x * (TPB / 64)) {
		const Unit t = unit_of(U, reads, u);
		if (!t.n) continue;
		const ReadRef a = reads.ref(t.r0);
		if (t.n == 1) {                                                      // a single read: the record of a pair without overlap
			const ReadOverlap rec = overlap_record(a.len, 0, 0, 0, P.min_len);
			if (rec.len) mine++;
			if (lane == 0) {
				ov[t.r0] = rec;
				if (keep) keep[t.r0] = rec.len ? 1 : 0;
			}
			continue;
		}
		const ReadRef b = reads.ref(t.r1);
		const uint64_t La = a.len, Lb = b.len;
		// the shifts whose overlap can reach min_overlap: d_first + s, s < nshift (sdt_read_plan.h)
		const uint64_t nshift = overlap_shifts(La, Lb, P.min_overlap);
		const long long d_first = (long long)P.min_overlap - (long long)Lb;
		long long best_score = 0, best_d = 0;
		uint32_t best_h = 0;
		int has = 0;
		for (uint64_t s0 = 0; s0 < nshift; s0 += 64) {
			const uint64_t s = s0 + lane;
			if (s >= nshift) continue;
			const long long d = d_first + (long long)s;
			const uint64_t i0 = d > 0 ? (uint64_t)d : 0, q0 = d < 0 ? (uint64_t)-d : 0;      // the first column in a and in b'
			const uint64_t end = (uint64_t)(d + (long long)Lb) < La ? (uint64_t)(d + (long long)Lb) : La;
			const uint64_t o = end - i0, budget = (uint64_t)P.max_err_pct * o / 100;         // 100 h <= pct o  <=>  h <= budget
			uint64_t h = 0;
			for (uint64_t c = 0; c < o && h <= budget; c += 32) {
				const uint64_t nb = o - c;
				uint64_t x = read_window(a, i0 + c) ^ overlap_rc_window(read_window_end(b, Lb - q0 - c));
				x = (x | x >> 1) & PAIR_LOW;
				if (nb < 32) x &= ~(~0ULL >> (2 * nb));
				h += (uint64_t)__popcll(x);
			}
			if (h > budget) continue;
			const long long score = (long long)o - 3 * (long long)h;
			if (!has || score >= best_score) {                                   // (d ascends: the greatest insert among equals stays)
				best_score = score;
				best_d = d;
				best_h = (uint32_t)h;
				has = 1;
			}
		}
#pragma unroll
		for (int m = 32; m > 0; m >>= 1) {
			const long long os = __shfl_xor(best_score, m), od = __shfl_xor(best_d, m);
			const uint32_t oh = __shfl_xor(best_h, m);
			const int ohas = __shfl_xor(has, m);
			if (ohas && (!has || os > best_score || (os == best_score && od > best_d))) {
				best_score = os;
				best_d = od;
				best_h = oh;
				has = 1;
			}
		}
		uint64_t o = 0, F = 0;
		if (has) {
			F = (uint64_t)(best_d + (long long)Lb);
			o = (F < La ? F : La) - (best_d > 0 ? (uint64_t)best_d : 0);
		}
		const ReadOverlap ra = overlap_record(La, o, best_h, F, P.min_len), rb = overlap_record(Lb, o, best_h, F, P.min_len);
		mine += (ra.len ? 1u : 0u) + (rb.len ? 1u : 0u);
		if (lane == 0) {
			ov[t.r0] = ra;
			ov[t.r1] = rb;
			if (keep) {
				keep[t.r0] = ra.len ? 1 : 0;
				keep[t.r1] = rb.len ? 1 : 0;
			}
		}
	}
	if (lane == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
