// sdt_clip_kernels.cuh -- adapters and poly-A/T tails clipped from reads on the device (the rule: include/sdt_gpu.h).  Needs no table
// and no LDS; every read is decided on its own by one wavefront:
//   k_clip_reads : 3' adapters: lane j tests position p = 64 step + j, steps ascending.  The lane holds the 32 bases of the read at p
//                  as one 64-bit window (read_window) and XORs it with the adapter's first chunk; a pair of bits that differs is a
//                  mismatch, counted by a popcount and masked to the overlap.  Further chunks are fetched only by the lanes that
//                  are still within their budget of mismatches.  The adapters are the inner loop, so the window is loaded once per
//                  step; a ballot of the hits gives the adapter's smallest p of the step.  The smallest p over all adapters lies
//                  in the first step in which any adapter hits: the steps end there.
//                  5' adapters: the mirror image over ends e = L - 64 step - j, with windows that END at e and chunks that are
//                  aligned to the adapter's end (sdt_read_plan.h: split_adapter).
//                  Tails, per eligible base: lane j takes one base of the segment per step, 64 per step from the segment's end;
//                  the mismatches up to the lane are a popcount over a ballot, with a carry across the steps.  Every lane keeps
//                  its best admissible (score, t); one wave reduction at the end.  The steps end once so many mismatches are
//                  behind that no longer tail is admissible.
// The adapter chunks are wave-uniform loads from a small device buffer.  Every loop is bounded by the read length, the adapter
// length or the number of adapters; no lane waits for another, the matching uses no atomics; one atomic per wavefront counts the
// reads kept.
#pragma once
#include "sdt_dedup_kernels.cuh"

namespace sdt {

struct ReadClip {                                        // == sdt_read_clip of include/sdt_gpu.h
	uint32_t adapters, tail3, tail5, start, len, verdict;
};
static_assert(sizeof(ReadClip) == 24, "sdt_read_clip is six 32-bit words");

constexpr uint32_t CLIP_WHOLE = 0, CLIP_CLIPPED = 2, CLIP_DROPPED = 3;

// the adapters on the device: ad[0, n3) are the 3' adapters, ad[n3, n3 + n5) the 5' adapters, each group by ascending id
struct ClipSet {
	const ClipAdapter *ad;
	uint32_t n3, n5;
};

constexpr uint64_t PAIR_LOW = 0x5555555555555555ULL;

// the bases [e - 32, e) of the read (0 < e <= len), the LAST in the least significant pair, zero before the read's start
__device__ inline uint64_t read_window_end(const ReadRef &r, uint64_t e)
{
	const uint32_t nb = e < 32 ? (uint32_t)e : 32u;
	const uint64_t v = read_window(r, e - nb);
	return nb == 32 ? v : v >> (2 * (32 - nb));
}

// does 3' adapter a hit at position p of the read (len - p >= min_overlap)?  w0 = read_window(rd, p)
__device__ inline bool clip_hit3(const ReadRef &rd, const ClipAdapter &a, uint64_t p, uint64_t w0, uint32_t pct)
{
	const uint64_t left = rd.len - p;
	const uint32_t o = left < a.m ? (uint32_t)left : a.m, budget = pct * o / 100;        // 100 h <= pct o  <=>  h <= budget
	uint32_t h = 0;
	for (uint32_t c = 0; 32 * c < o; c++) {
		const uint32_t nb = o - 32 * c;
		uint64_t x = (c ? read_window(rd, p + 32 * c) : w0) ^ a.chunk[c];
		x = (x | x >> 1) & PAIR_LOW;
		if (nb < 32) x &= ~(~0ULL >> (2 * nb));
		h += (uint32_t)__popcll(x);
		if (h > budget) return false;
	}
	return true;
}

// does 5' adapter a hit with its end at e of the read (e >= min_overlap)?  w0 = read_window_end(rd, e)
__device__ inline bool clip_hit5(const ReadRef &rd, const ClipAdapter &a, uint64_t e, uint64_t w0, uint32_t pct)
{
	const uint32_t o = e < a.m ? (uint32_t)e : a.m, budget = pct * o / 100;
	uint32_t h = 0;
	for (uint32_t c = 0; 32 * c < o; c++) {
		const uint32_t nb = o - 32 * c;
		uint64_t x = (c ? read_window_end(rd, e - 32 * c) : w0) ^ a.chunk[c];
		x = (x | x >> 1) & PAIR_LOW;
		if (nb < 32) x &= (1ULL << (2 * nb)) - 1;
		h += (uint32_t)__popcll(x);
		if (h > budget) return false;
	}
	return true;
}

// the tail of base b on the segment [s, e) of the read: END3: the suffix [e - t, e), else the prefix [s, s + t).  Wave-uniform.
template <bool END3>
__device__ inline uint64_t clip_tail(const ReadRef &rd, uint64_t s, uint64_t e, uint32_t b, uint32_t min_tail, uint32_t pct, int lane)
{
	const uint64_t n = e - s;
	long long best_score = 0;
	uint64_t best_t = 0, behind = 0;                         // best_t == 0: no admissible t yet; behind: mismatches of the steps so far
	for (uint64_t t0 = 0; t0 < n; t0 += 64) {
		const uint64_t t = t0 + lane + 1;
		const bool in = t <= n;
		uint32_t c = 4;
		if (in) {
			const uint64_t at = rd.sh + (END3 ? e - t : s + t - 1);
			c = (rd.w[at >> 4] >> (30 - 2 * (at & 15))) & 3u;
		}
		const uint64_t mism = __ballot(in && c != b);
		const uint64_t x = behind + __popcll(mism & (~0ULL >> (63 - lane)));
		if (c == b && t >= min_tail && 100 * x <= (uint64_t)pct * t) {
			const long long score = (long long)t - 3 * (long long)x;
			if (!best_t || score > best_score) { best_score = score; best_t = t; }        // (t ascends: the smallest among equals stays)
		}
		behind += __popcll(mism);
		if (100 * behind > (uint64_t)pct * n) break;         // every longer tail has at least these mismatches: none is admissible
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		const long long os = __shfl_xor(best_score, d);
		const unsigned long long ot = __shfl_xor((unsigned long long)best_t, d);
		if (ot && (!best_t || os > best_score || (os == best_score && ot < best_t))) { best_score = os; best_t = ot; }
	}
	return best_t;
}

static __global__ __launch_bounds__(TPB) void k_clip_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                           ClipParams P, ClipSet S, ReadClip *__restrict__ clip, uint8_t *__restrict__ keep,
                                                           unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t mine = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + wave; r < nreads; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const uint64_t at = offs[r];
		const ReadRef rd = {words + (at >> 4), (uint32_t)(at & 15), offs[r + 1] - at};
		const uint64_t L = rd.len;
		uint64_t e0 = L, s0 = 0;
		uint32_t a3 = 0, a5 = 0;
		if (L >= P.min_overlap) {
			const uint64_t span = L - P.min_overlap;                             // p <= span, e >= L - span
			for (uint64_t p0 = 0; S.n3 && p0 <= span && !a3; p0 += 64) {
				const uint64_t p = p0 + lane;
				const bool in = p <= span;
				const uint64_t w0 = in ? read_window(rd, p) : 0;
				uint32_t first = 64;
				for (uint32_t i = 0; i < S.n3; i++) {
					const uint64_t hits = __ballot(in && clip_hit3(rd, S.ad[i], p, w0, P.max_err_pct));
					const uint32_t l = hits ? (uint32_t)__ffsll((unsigned long long)hits) - 1 : 64u;
					if (l < first) { first = l; a3 = S.ad[i].id + 1; }
				}
				if (a3) e0 = p0 + first;
			}
			for (uint64_t d0 = 0; S.n5 && d0 <= span && !a5; d0 += 64) {
				const uint64_t d = d0 + lane;
				const bool in = d <= span;
				const uint64_t e = in ? L - d : L;
				const uint64_t w0 = in ? read_window_end(rd, e) : 0;
				uint32_t first = 64;
				for (uint32_t i = S.n3; i < S.n3 + S.n5; i++) {
					const uint64_t hits = __ballot(in && clip_hit5(rd, S.ad[i], e, w0, P.max_err_pct));
					const uint32_t l = hits ? (uint32_t)__ffsll((unsigned long long)hits) - 1 : 64u;
					if (l < first) { first = l; a5 = S.ad[i].id + 1; }
				}
				if (a5) s0 = L - d0 - first;
			}
		}
		uint64_t t3 = 0, t5 = 0;
		if (s0 < e0) {
			for (uint32_t b = 0; b < 4; b++)
				if (P.tail3_bases >> b & 1) {
					const uint64_t t = clip_tail<true>(rd, s0, e0, b, P.min_tail, P.tail_err_pct, lane);
					if (t > t3) t3 = t;
				}
			for (uint32_t b = 0; b < 4; b++)
				if (P.tail5_bases >> b & 1) {
					const uint64_t t = clip_tail<false>(rd, s0, e0 - t3, b, P.min_tail, P.tail_err_pct, lane);
					if (t > t5) t5 = t;
				}
		}
		const uint64_t start = s0 + t5, end = e0 - t3;
		const uint64_t len = end > start ? end - start : 0;
		ReadClip rec = {a3 | a5 << 16, (uint32_t)t3, (uint32_t)t5, (uint32_t)start, (uint32_t)len, CLIP_CLIPPED};
		if (len < (P.min_len > 1 ? P.min_len : 1u)) { rec.start = rec.len = 0; rec.verdict = CLIP_DROPPED; }
		else if (len == L) rec.verdict = CLIP_WHOLE;
		if (rec.len) mine++;
		if (lane == 0) {
			clip[r] = rec;
			if (keep) keep[r] = rec.len ? 1 : 0;
		}
	}
	if (lane == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
