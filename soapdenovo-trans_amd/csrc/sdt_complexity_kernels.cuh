// sdt_complexity_kernels.cuh -- low-complexity reads flagged, dropped or trimmed on the device (the rule: include/sdt_gpu.h).  Needs no
// table and no LDS; every read is decided on its own by one wavefront:
//   k_complexity_reads : the 64 kinds of triplets on the 64 lanes: lane t owns the triplet (t >> 4, t >> 2 & 3, t & 3).  A window of 64
//                        bases is two 64-bit words (read_chunk); window j + 1's first word is window j's second, so a window costs
//                        one load.  Per word and per base of its triplet the lane marks the positions that hold that base
//                        (complexity_marks); the marks of the second base moved one base forward and those of the third moved two
//                        bases forward, with the carry across the word boundary, ANDed with the marks of the first base, are the
//                        positions where the lane's triplet starts.  They are masked to the triplets that exist, which also takes
//                        out whatever lies past the read's end, and counted by two popcounts: c_t.  One wave reduction of
//                        c_t (c_t - 1) gives D to every lane.
//                        What follows is wave-uniform: the threshold, the score, and a sweep over the read in segments of 32 bases
//                        (segment k is low iff window k - 1 or window k is) that counts the low bases and keeps the clean run that
//                        is open and the best one so far.  Lane 0 writes the record and the keep byte.
// The only loop is over the windows, bounded by L / 32: there is no limit on the read length.  No lane waits for another, the
// scoring uses no atomics; one atomic per wavefront counts the reads kept.
#pragma once
#include "sdt_clip_kernels.cuh"

namespace sdt {

struct ReadComplexity {                                  // == sdt_read_complexity of include/sdt_gpu.h
	uint32_t windows, low, score, start, len, verdict;
};
static_assert(sizeof(ReadComplexity) == 24, "sdt_read_complexity is six 32-bit words");

// the positions of w (32 bases, the first in the most significant pair) that hold the base of which rep is 32 copies: the low bit
// of their pair
__device__ inline uint64_t complexity_marks(uint64_t w, uint64_t rep)
{
	const uint64_t x = w ^ rep;
	return ~(x | x >> 1) & PAIR_LOW;
}

// the first n pairs of a word, 0 <= n <= 32
__device__ inline uint64_t complexity_first_pairs(uint32_t n) { return n >= 32 ? ~0ULL : ~(~0ULL >> (2 * n)); }

template <class Reads>
static __global__ __launch_bounds__(TPB) void k_complexity_reads(Reads reads, ComplexityParams P, ReadComplexity *__restrict__ cx,
                                                                 uint8_t *__restrict__ keep, unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t rep0 = (uint64_t)(lane >> 4) * PAIR_LOW, rep1 = (uint64_t)(lane >> 2 & 3) * PAIR_LOW, rep2 = (uint64_t)(lane & 3) * PAIR_LOW;
	uint32_t mine = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + wave; r < reads.n; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const ReadRef rd = reads.ref(r);
		const uint64_t L = rd.len, W = complexity_windows(L);
		uint32_t nlow = 0, score = 0;
		uint64_t B = 0, run_s = 0, run_n = 0, best_s = 0, best_n = 0;            // low bases; the clean run that is open; the best so far
		bool prev = false;                                                       // was window j - 1 low
		// a segment [a, e) of bases that are all low or all clean, segments ascending
		auto segment = [&](uint64_t a, uint64_t e, bool low) {
			if (low) { B += e - a; run_n = 0; return; }
			if (!run_n) run_s = a;
			run_n += e - a;
			if (run_n > best_n) { best_s = run_s; best_n = run_n; }              // (ascending: the first among equals stays)
		};
		uint64_t w = L ? read_chunk(rd, 0) : 0;
		uint64_t a0 = complexity_marks(w, rep0), a1 = complexity_marks(w, rep1), a2 = complexity_marks(w, rep2);
		for (uint64_t j = 0; j < W; j++) {
			const uint64_t begin = complexity_window_begin(j);
			const uint32_t m = (uint32_t)(complexity_window_end(j, L) - begin), l = m > 2 ? m - 2 : 0;
			w = begin + 32 < L ? read_chunk(rd, j + 1) : 0;
			const uint64_t b0 = complexity_marks(w, rep0), b1 = complexity_marks(w, rep1), b2 = complexity_marks(w, rep2);
			const uint64_t hi = a0 & (a1 << 2 | b1 >> 62) & (a2 << 4 | b2 >> 60) & complexity_first_pairs(l);
			const uint64_t lo = b0 & (b1 << 2) & (b2 << 4) & complexity_first_pairs(l > 32 ? l - 32 : 0);
			const uint32_t c = (uint32_t)__popcll(hi) + (uint32_t)__popcll(lo);
			uint32_t D = c * (c - 1);
#pragma unroll
			for (int d = 32; d > 0; d >>= 1)
				D += __shfl_xor(D, d);
			D = __builtin_amdgcn_readfirstlane(D);                               // (every lane has it: what follows is scalar work)
			bool low = false;
			if (l >= 2) {
				const uint32_t pairs = l * (l - 1);                              // 3 782 at most: 100 D fits
				low = 100 * D >= P.max_score_pct * pairs;
				const uint32_t s = 100 * D / pairs;
				if (s > score) score = s;
			}
			nlow += low ? 1u : 0u;
			segment(begin, begin + 32 < L ? begin + 32 : L, prev || low);
			prev = low;
			a0 = b0; a1 = b1; a2 = b2;
		}
		if (L > 32) segment(32 * W, L, prev);                                    // the last 32 bases or fewer: window W - 1 alone covers them
		uint64_t start = 0, len = L;
		if (P.flags & COMPLEXITY_TRIM) { start = best_s; len = best_n; }
		else if (100 * B > (uint64_t)P.max_low_pct * L) len = 0;
		ReadComplexity rec = {(uint32_t)W, nlow, score, (uint32_t)start, (uint32_t)len, CLIP_CLIPPED};
		if (len < (P.min_len > 1 ? P.min_len : 1u)) { rec.start = rec.len = 0; rec.verdict = CLIP_DROPPED; }
		else if (len == L) rec.verdict = CLIP_WHOLE;
		if (rec.len) mine++;
		if (lane == 0) {
			cx[r] = rec;
			if (keep) keep[r] = rec.len ? 1 : 0;
		}
	}
	if (lane == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
