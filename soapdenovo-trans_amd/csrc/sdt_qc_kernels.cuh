// sdt_qc_kernels.cuh -- the per-cycle QC report of a read batch (the rule: include/sdt_gpu.h).  The one read stage that is a reduction
// over the batch: no record per read, but histograms by (row, base) and (row, quality).  One global atomic per base would queue
// 1.2 G adds on a few thousand addresses for 4 M reads of 150 bases, so the counting happens in LDS:
//   k_qc_reads : a workgroup of QC_WAVES wavefronts owns a strided share of the reads and ONE set of LDS histograms: a tile of QC_TILE
//                rows x (4 bases + 94 qualities) 32-bit counters, the whole len[R], gc[101] and meanq[94], and row C in 64 bits.  It
//                walks its reads once per tile of rows [t0, t0 + QC_TILE), t0 < C:
//                  pass 0 (t0 = 0) walks every counted base of every read: it needs them all for the read's own sums (#C + #G: the low
//                    bit of a code, sum of q), which a wave reduction turns into the read's gc and meanq bins; one lane adds those and
//                    the len bin.  Of the rows it counts those below QC_TILE and row C.
//                  pass t0 > 0 walks only the positions whose row lies in the tile: [t0, t1) forward, [n - t1, n - t0) from the end,
//                    t1 = min(t0 + QC_TILE, C).  A read with n <= t0 is skipped from its offsets (and its range) alone.
//                Within a read a lane takes 4 consecutive positions: the 4 quality bytes as ONE aligned 32-bit load, what lies outside
//                [first, last counted byte] masked, exactly as k_quality_reads does; the 4 bases from the one or two 2-bit words
//                that hold them, at any of the 16 phases.  A wavefront takes 256 positions per step.  Neither a word of the stream nor
//                a quality word without a counted base is loaded.  Lanes hit different rows, so below row C the ds_add_u32 of one
//                instruction never meet on an address (the row stride is 99 counters, odd: consecutive rows fall into different
//                banks); on row C they do, and serialise: accepted (a read past C cycles is the rare case the row exists for).
//                After each pass the workgroup adds its non-zero counters to the report with 64-bit global atomics, zeroes them, and
//                stops once t0 + QC_TILE reaches min(longest n it saw, C).
// Why nothing wraps.  A 32-bit LDS counter below row C grows by at most 1 per read and pass; len, gc and meanq by 1 per read.  A
// workgroup flushes after every QC_EPOCH = 2^27 reads of each of its 16 wavefronts, 2^31 reads: no counter reaches 2^32.  Row C takes
// n - C additions from one read and is 64-bit in LDS, like the per-read sums and the totals (registers).
// The byte of base b of the stream is quals[b + delta]: 0 in the device form; in the host form words are staged from a multiple of 16
// bases and bytes from a multiple of 4, so one signed delta per launch lies between the two.
#pragma once
#include "sdt_trim_kernels.cuh"

namespace sdt {

constexpr int QC_TPB = QC_WAVES * 64;                    // 1024: two workgroups per CU fill its 32 wavefronts
constexpr int QC_COLS = 4 + (int)QC_QUALS;               // counters of a row: 4 bases, 94 qualities
constexpr int QC_STRIDE = QC_COLS + 1;                   // (odd)
constexpr uint64_t QC_EPOCH = 1ULL << 27;                // reads a wavefront takes between two flushes
constexpr int QC_STEP = 256;                             // positions a wavefront takes per step: 4 per lane

struct QcArgs {
	const uint32_t *words;
	const uint8_t *quals;                                // or nullptr
	const uint64_t *offs;
	uint64_t nreads;
	const ReadTrim *ranges;                              // or nullptr
	const uint8_t *classes;                              // or nullptr
	long long delta;                                     // byte of a base - its index in the stream
	QcParams P;
	unsigned long long *report;
};

struct QcLds {
	unsigned long long rowC[QC_COLS];
	uint32_t tile[QC_TILE * QC_STRIDE];
	uint32_t len[QC_MAX_CYCLES + 1];
	uint32_t gc[QC_GC_BINS];
	uint32_t meanq[QC_QUALS];
	uint32_t longest;                                    // min(n, C) of the longest counted read of the epoch
};
static_assert(2 * sizeof(QcLds) <= 160 * 1024, "two workgroups per CU");

// Positions [i_lo, i_hi), i_lo < i_hi, of a read whose position 0 is base b0 of the stream and which has n counted bases.  FIRST: pass
// 0, which also sums the read's C + G into gc and its qualities into sq (per lane) and counts row C; else every position's row lies
// in [t0, t0 + QC_TILE).
template <bool FIRST>
__device__ inline void qc_walk(const QcArgs &A, QcLds &S, uint64_t b0, uint64_t n, uint64_t i_lo, uint64_t i_hi, uint32_t t0, int lane,
                               uint64_t &gc, uint64_t &sq)
{
	const uint32_t C = A.P.cycles;
	const bool from_end = (A.P.flags & QC_FROM_END) != 0;
	const uint64_t q0 = b0 + (uint64_t)A.delta;                          // the byte of position 0
	const uint64_t lo = q0 + i_lo, hi = q0 + i_hi;                       // the counted bytes
	for (uint64_t p = (lo & ~3ULL) + 4 * (uint64_t)lane; p < hi; p += QC_STEP) {
		// the lane's bytes p + [kf, kl): at least one (p + 3 >= lo and p < hi)
		const int kf = p < lo ? (int)(lo - p) : 0, kl = hi - p < 4 ? (int)(hi - p) : 4;
		const uint32_t w = A.quals ? *(const uint32_t *)(A.quals + p) : 0u;
		const uint64_t bb = p - (uint64_t)A.delta;                       // base of byte p (used from kf on)
		const uint64_t wlo = (bb + kf) >> 4, whi = (bb + kl - 1) >> 4;
		const uint32_t xlo = A.words[wlo], xhi = whi != wlo ? A.words[whi] : xlo;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (k < kf || k >= kl) continue;
			const uint64_t b = bb + k, i = p + k - q0;
			const uint32_t code = (((b >> 4) == wlo ? xlo : xhi) >> (30 - 2 * (int)(b & 15))) & 3u;
			const uint32_t q = quality_of(w >> (8 * k) & 255u, A.P.phred_offset);
			const uint64_t rw = from_end ? n - 1 - i : i;
			if (FIRST) {
				gc += code & 1u;                                         // C 1, G 3
				sq += q;
				if (rw >= C) {
					atomicAdd(&S.rowC[code], 1ULL);
					if (A.quals) atomicAdd(&S.rowC[4 + q], 1ULL);
					continue;
				}
				if (rw >= (uint64_t)QC_TILE) continue;
			}
			uint32_t *row = S.tile + ((uint32_t)rw - t0) * QC_STRIDE;
			atomicAdd(row + code, 1u);
			if (A.quals) atomicAdd(row + 4 + q, 1u);
		}
	}
}

__device__ inline uint64_t qc_wave_sum(uint64_t v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d);
	return v;
}

// (8 wavefronts per SIMD: two workgroups per CU.  The registers that allows, 64, cost a few spills outside the walk; SDT_QC_MIN_WAVES=4
// is the build without them, one workgroup per CU: the A/B of DESIGN.md 4r)
#ifndef SDT_QC_MIN_WAVES
#define SDT_QC_MIN_WAVES 8
#endif
static __global__ __launch_bounds__(QC_TPB, SDT_QC_MIN_WAVES) void k_qc_reads(QcArgs A)
{
	__shared__ QcLds S;
	// (readfirstlane: the wavefront's number, and with it the read, its offsets, range and class, are uniform values in scalar registers)
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t C = A.P.cycles;
	const bool from_end = (A.P.flags & QC_FROM_END) != 0;
	const QcLayout lay = qc_layout(C);
	for (uint32_t j = threadIdx.x; j < sizeof(QcLds) / 4; j += QC_TPB) ((uint32_t *)&S)[j] = 0;
	__syncthreads();
	unsigned long long n_reads = 0, n_empty = 0, n_bases = 0, n_passed = 0, n_clamped = 0;     // wave-uniform
	const uint64_t per_round = (uint64_t)gridDim.x * QC_WAVES;
	const uint64_t rounds = A.nreads / per_round + (A.nreads % per_round != 0);
	for (uint64_t e0 = 0; e0 < rounds; e0 += QC_EPOCH) {
		const uint64_t e1 = rounds - e0 < QC_EPOCH ? rounds : e0 + QC_EPOCH;
		for (uint32_t t0 = 0;; t0 += QC_TILE) {
			const uint32_t t1 = C - t0 < (uint32_t)QC_TILE ? C : t0 + QC_TILE;
			uint32_t longest = 0;
			for (uint64_t it = e0; it < e1; it++) {
				const uint64_t r = (it * gridDim.x + blockIdx.x) * QC_WAVES + wave;
				if (r >= A.nreads) break;
				if (A.classes && A.classes[r] != A.P.class_sel) {
					if (t0 == 0) n_passed++;
					continue;
				}
				const uint64_t o0 = A.offs[r], L = A.offs[r + 1] - o0;
				uint64_t s = 0, n = L;
				if (A.ranges) {
					s = A.ranges[r].start;
					n = A.ranges[r].len;
					bool clamped = false;
					if (s > L) { s = L; clamped = true; }
					if (n > L - s) { n = L - s; clamped = true; }
					if (t0 == 0 && clamped) n_clamped++;
				}
				if (t0 == 0) {
					n_reads++;
					n_bases += n;
					if (n == 0) {
						n_empty++;
						if (lane == 0) atomicAdd(&S.len[0], 1u);
						continue;
					}
					uint64_t gc = 0, sq = 0;
					qc_walk<true>(A, S, o0 + s, n, 0, n, 0, lane, gc, sq);
					gc = qc_wave_sum(gc);
					sq = qc_wave_sum(sq);
					const uint32_t nc = n < C ? (uint32_t)n : C;
					if (nc > longest) longest = nc;
					if (lane == 0) {
						atomicAdd(&S.len[nc], 1u);
						atomicAdd(&S.gc[100 * gc / n], 1u);
						if (A.quals) atomicAdd(&S.meanq[sq / n], 1u);
					}
				} else if (n > t0) {
					uint64_t gc = 0, sq = 0;
					const uint64_t i_lo = from_end ? (n > t1 ? n - t1 : 0) : t0, i_hi = from_end ? n - t0 : (n < t1 ? n : t1);
					qc_walk<false>(A, S, o0 + s, n, i_lo, i_hi, t0, lane, gc, sq);
				}
			}
			if (t0 == 0 && lane == 0 && longest) atomicMax(&S.longest, longest);
			__syncthreads();
			const uint32_t lim = S.longest;                              // rows [0, lim) hold something
			const uint32_t rows = lim <= t0 ? 0 : (lim - t0 < (uint32_t)QC_TILE ? lim - t0 : QC_TILE);
			for (uint32_t j = threadIdx.x; j < rows * QC_STRIDE; j += QC_TPB) {
				const uint32_t v = S.tile[j];
				if (!v) continue;
				const uint32_t rr = j / QC_STRIDE, col = j - rr * QC_STRIDE;
				atomicAdd(A.report + (col < 4 ? lay.base + (uint64_t)(t0 + rr) * 4 + col : lay.qual + (uint64_t)(t0 + rr) * QC_QUALS + (col - 4)),
				          (unsigned long long)v);
				S.tile[j] = 0;
			}
			if (t0 == 0) {
				for (uint32_t j = threadIdx.x; j <= C; j += QC_TPB)
					if (const uint32_t v = S.len[j]) { atomicAdd(A.report + lay.len + j, (unsigned long long)v); S.len[j] = 0; }
				for (uint32_t j = threadIdx.x; j < QC_GC_BINS; j += QC_TPB)
					if (const uint32_t v = S.gc[j]) { atomicAdd(A.report + lay.gc + j, (unsigned long long)v); S.gc[j] = 0; }
				for (uint32_t j = threadIdx.x; j < QC_QUALS; j += QC_TPB)
					if (const uint32_t v = S.meanq[j]) { atomicAdd(A.report + lay.meanq + j, (unsigned long long)v); S.meanq[j] = 0; }
				for (uint32_t j = threadIdx.x; j < (uint32_t)QC_COLS; j += QC_TPB)
					if (const unsigned long long v = S.rowC[j]) {
						atomicAdd(A.report + (j < 4 ? lay.base + (uint64_t)C * 4 + j : lay.qual + (uint64_t)C * QC_QUALS + (j - 4)), v);
						S.rowC[j] = 0;
					}
			}
			__syncthreads();
			if (t1 >= lim) break;                                        // (uniform: lim comes from LDS)
		}
		if (threadIdx.x == 0) S.longest = 0;
		__syncthreads();
	}
	if (lane == 0) {
		if (n_reads) atomicAdd(A.report + lay.totals + 0, n_reads);
		if (n_empty) atomicAdd(A.report + lay.totals + 1, n_empty);
		if (n_bases) atomicAdd(A.report + lay.totals + 2, n_bases);
		if (n_passed) atomicAdd(A.report + lay.totals + 3, n_passed);
		if (n_clamped) atomicAdd(A.report + lay.totals + 4, n_clamped);
	}
}

} // namespace sdt
