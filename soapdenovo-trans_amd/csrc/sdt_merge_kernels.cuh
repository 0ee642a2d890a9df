// sdt_merge_kernels.cuh -- the two mates of an overlapping pair merged into one fragment read on the device, and the quality bytes of
// a stream carried through a compaction (the rule: include/sdt_gpu.h).  Needs no table, no LDS and no atomics on the stream:
//   k_merge_decide  : one lane per unit (a pair; in the kept form also a single read): merge_decide (sdt_read_plan.h) on the two
//                     overlap records and the two lengths -> flen[u], the merged length or 0.  The smallest id of a unit whose records
//                     are inconsistent is kept by one atomic min: the kept form refuses the call with it, the device form does not
//                     look at it.  Three scans over flen (sdt_merge.hip) place every merged read.
//   k_merge_pairs   : one wavefront per unit.  Lane j of step s produces bases [32 (64 s + j), + 32) of the merged read as one 64-bit
//                     value.  A position comes from one of two windows: read_window(a, p), or the window of b that ENDS where b'
//                     starts at this position, turned round in registers (overlap_rc_window(read_window_end(b, F - p)): the identity
//                     of k_overlap_pairs), chosen by masks built from p < La and p >= d.  One XOR finds the mismatch columns among
//                     the columns both cover; their popcount is counted.  Only a lane with a mismatch column and qualities visits each
//                     set bit: two byte loads, the base of the better quality, ties to mate 1.  Neighbouring merged reads share words
//                     of the dense output, so the wavefront stores whole 64-bit values into a SCRATCH stream in which every merged read
//                     starts at a 64-bit value (coalesced across lanes); k_compact_words (sdt_select_kernels.cuh) packs the dense
//                     stream and its pad from there.  One wave reduction for mismatches and from_b; lane 0 writes both records, the
//                     read's output offset and where it starts in the scratch.
//   k_compact_quals : one lane per 4 OUTPUT bytes: the read that holds the first of them by binary search in the scan of the kept
//                     lengths, then byte by byte on into the following reads.  No partial stores; zero behind the last byte.
// Every loop is bounded by F, by 4 or by the number of stretches; no lane waits for another.
#pragma once
#include "sdt_overlap_kernels.cuh"
#include "sdt_trim_kernels.cuh"

namespace sdt {

struct ReadMerge {                                       // == sdt_read_merge of include/sdt_gpu.h
	uint32_t merged, mismatches, from_b, start, len, verdict;
};
static_assert(sizeof(ReadMerge) == 24, "sdt_read_merge is six 32-bit words");

constexpr uint32_t MERGE_MERGED = 5;                     // SDT_MERGE_MERGED
constexpr uint32_t MERGE_ABSENT = 0xFFFFFFFFu;           // verdict of a record that no read has written (kept form: the array is preset)
constexpr unsigned long long MERGE_NO_UNIT = ~0ULL;

// where the quality bytes of read r start: under the offsets of the dense stream; the kept reads carry none
__device__ inline uint64_t merge_qual_start(const DenseReads &R, uint64_t r) { return R.offs[r]; }
__device__ inline uint64_t merge_qual_start(const KeptReads &, uint64_t) { return 0; }

// flen[u] for u < U.n, flen[U.n] = 0 (the scans' last output is the total)
template <class Reads>
static __global__ __launch_bounds__(TPB) void k_merge_decide(Reads reads, Units U, const ReadOverlap *__restrict__ ov, MergeParams P,
                                                             uint32_t *__restrict__ flen, unsigned long long *first_bad)
{
	for (uint64_t u = blockIdx.x * (uint64_t)TPB + threadIdx.x; u <= U.n; u += (uint64_t)gridDim.x * TPB) {
		uint32_t F = 0;
		if (u < U.n) {
			const Unit t = unit_of(U, reads, u);
			if (t.n == 2) {
				const int64_t m = merge_decide(reads.ref(t.r0).len, reads.ref(t.r1).len, ov[t.r0].insert, ov[t.r1].insert, P.min_len, P.max_len);
				if (m == MERGE_INCONSISTENT) atomicMin(first_bad, (unsigned long long)t.id);
				else F = (uint32_t)m;
			}
		}
		flen[u] = F;
	}
}

// what the three scans run over
struct MergedLen {
	const uint32_t *flen;
	__device__ uint64_t operator()(uint64_t u) const { return flen[u]; }
};
struct MergedFlag {
	const uint32_t *flen;
	__device__ uint64_t operator()(uint64_t u) const { return flen[u] ? 1 : 0; }
};
struct MergedChunks {
	const uint32_t *flen;
	__device__ uint64_t operator()(uint64_t u) const { return merge_chunks(flen[u]); }
};

// the first n pairs of a 64-bit window (n <= 32)
__device__ inline uint64_t merge_first_pairs(uint64_t n) { return n >= 32 ? ~0ULL : ~(~0ULL >> (2 * n)); }

// new_off / rank / chunk0: the exclusive scans of MergedLen / MergedFlag / MergedChunks over U.n + 1 entries; total = new_off[U.n],
// n_merged = rank[U.n].  scratch: 64-bit values as two 32-bit words, the first 16 bases in the first (the word order of the stream).
template <class Reads>
static __global__ __launch_bounds__(TPB) void k_merge_pairs(Reads reads, Units U, const ReadOverlap *__restrict__ ov, const uint8_t *__restrict__ quals,
                                                            uint32_t phred_offset, const uint32_t *__restrict__ flen,
                                                            const uint64_t *__restrict__ new_off, const uint64_t *__restrict__ rank,
                                                            const uint64_t *__restrict__ chunk0, uint64_t total, uint64_t n_merged,
                                                            ReadMerge *__restrict__ mg, uint2 *__restrict__ scratch,
                                                            uint64_t *__restrict__ out_offs, uint64_t *__restrict__ src_start)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (blockIdx.x == 0 && threadIdx.x == 0) out_offs[n_merged] = total;
	for (uint64_t u = blockIdx.x * (uint64_t)(TPB / 64) + wave; u < U.n; u += (uint64_t)gridDim.x * (TPB / 64)) {
		const Unit t = unit_of(U, reads, u);
		if (!t.n) continue;
		const uint64_t F = flen[u];
		if (!F) {                                                            // not merged: what the overlap record keeps of every read
			if (lane == 0) {
				const ReadOverlap oa = ov[t.r0];
				mg[t.r0] = ReadMerge{0, 0, 0, oa.start, oa.len, oa.verdict};
				if (t.n == 2) {
					const ReadOverlap ob = ov[t.r1];
					mg[t.r1] = ReadMerge{0, 0, 0, ob.start, ob.len, ob.verdict};
				}
			}
			continue;
		}
		const ReadRef a = reads.ref(t.r0), b = reads.ref(t.r1);              // (F != 0: both mates are there)
		const uint64_t La = a.len, Lb = b.len;
		const long long d = (long long)F - (long long)Lb;                    // -Lb < d < La
		const uint64_t qa0 = quals ? merge_qual_start(reads, t.r0) : 0, qb0 = quals ? merge_qual_start(reads, t.r1) : 0;
		const uint64_t at = chunk0[u];
		uint32_t mism = 0, fromb = 0;
		for (uint64_t p0 = (uint64_t)lane << 5; p0 < F; p0 += 2048) {
			const uint64_t in_f = merge_first_pairs(F - p0);                 // the positions of this window that are in [0, F)
			const uint64_t in_a = p0 < La ? merge_first_pairs(La - p0) & in_f : 0;
			const uint64_t wa = p0 < La ? read_window(a, p0) : 0;
			// b' lies on positions [d, F): from pair i0 of this window on
			const uint64_t i0 = d > (long long)p0 ? (uint64_t)(d - (long long)p0) : 0;
			uint64_t wb = 0, in_b = 0;
			if (i0 < 32 && i0 < F - p0) {                                    // (a window of b is read only where b' has a position)
				wb = overlap_rc_window(read_window_end(b, F - p0 - i0)) >> (2 * i0);         // b'[p0 + i0 - d ...] from pair i0 on
				in_b = (~0ULL >> (2 * i0)) & in_f;
			}
			uint64_t x = wa ^ wb;
			x = (x | x >> 1) & PAIR_LOW & in_a & in_b;                       // the mismatch columns: the low bit of their pairs
			uint64_t m = (wa & in_a) | (wb & in_b & ~in_a);
			mism += (uint32_t)__popcll(x);
			if (x && quals) {
				for (uint64_t rest = x; rest; rest &= rest - 1) {
					const int bit = __ffsll((unsigned long long)rest) - 1;  // pair i has its low bit at 62 - 2 i
					const uint64_t p = p0 + (uint64_t)((62 - bit) >> 1);
					const uint32_t qa = quality_of(quals[qa0 + p], phred_offset), qb = quality_of(quals[qb0 + (F - 1 - p)], phred_offset);
					if (qb > qa) {                                           // (a tie goes to mate 1)
						m = (m & ~(3ULL << bit)) | (wb & (3ULL << bit));
						fromb++;
					}
				}
			}
			scratch[at + (p0 >> 5)] = make_uint2((uint32_t)(m >> 32), (uint32_t)m);
		}
#pragma unroll
		for (int k = 32; k > 0; k >>= 1) {
			mism += __shfl_xor(mism, k);
			fromb += __shfl_xor(fromb, k);
		}
		if (lane == 0) {
			const ReadMerge rec = {(uint32_t)F, mism, fromb, 0, 0, MERGE_MERGED};
			mg[t.r0] = rec;
			mg[t.r1] = rec;
			out_offs[rank[u]] = new_off[u];
			src_start[rank[u]] = at << 5;
		}
	}
}

// ---- quality bytes through a compaction --------------------------------------------------------------------------------------------
// new_off: the exclusive scan of TrimmedLen over nreads + 1 entries, total = new_off[nreads] > 0.  Output word w holds bytes
// [4 w, 4 w + 4) of the compacted bytes: the byte at 4 w + k in bits [8 k, 8 k + 8); zero past `total`.
static __global__ __launch_bounds__(TPB) void k_compact_quals(const uint8_t *__restrict__ quals, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                              const ReadTrim *__restrict__ trim, const uint64_t *__restrict__ new_off,
                                                              uint64_t total, uint32_t *__restrict__ out)
{
	const uint64_t nw = (total + 3) >> 2;
	for (uint64_t w = blockIdx.x * (uint64_t)TPB + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * TPB) {
		const uint64_t b0 = w << 2;
		uint64_t lo = 0, hi = nreads;                                    // the last read whose kept bytes start at or before b0: among reads
		while (hi - lo > 1) {                                            // that start there, the one that is not empty
			const uint64_t mid = lo + ((hi - lo) >> 1);
			if (new_off[mid] <= b0) lo = mid; else hi = mid;
		}
		uint64_t r = lo, s, l;
		trim_range(trim, offs, r, s, l);
		uint32_t v = 0;
		for (int k = 0; k < 4 && b0 + k < total; k++) {
			const uint64_t b = b0 + k;
			while (new_off[r + 1] <= b) {                                // (b < total = new_off[nreads]: ends at a read below nreads)
				r++;
				trim_range(trim, offs, r, s, l);
			}
			v |= (uint32_t)quals[offs[r] + s + (b - new_off[r])] << (8 * k);
		}
		out[w] = v;
	}
}

} // namespace sdt
