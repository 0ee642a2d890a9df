// sdt_select_kernels.cuh -- in-silico read normalisation against the counted node table (read-only; the rule: include/sdt_gpu.h):
//   k_pick_stats    : one wavefront per read, the shape of k_profile_reads: the 32-bit count of every k-mer of the read into an LDS
//                     strip, S1 = sum and S2 = sum of squares of the counts saturated at 65 535 carried per lane beside min and max,
//                     then the lower median by strip_lower_median and the dispersion test, uniform over the wave.  Writes kmers, median
//                     and the own-aberrant bit of the read's record.
//   k_pick_decide   : one lane per unit (a read, or the two mates of a pair): combines the mates' records, draws, writes cov and the
//                     verdict to every read of the unit and keep[]; kept reads are counted with one atomic per wave.  A kernel of its
//                     own because the mates of a kept pair sit in different kept batches (read-1 file, read-2 file).
//   k_compact_place / k_compact_words : the kept reads of a 2-bit stream packed base-contiguous again, one lane per OUTPUT word: no
//                     atomics, no partial-word stores, the same words whatever the launch geometry.
#pragma once
#include "sdt_search_kernels.cuh"
#include "sdt_read_plan.h"

namespace sdt {

struct ReadPick {                                        // == sdt_read_pick of include/sdt_gpu.h
	uint32_t kmers, median, cov, verdict;
};
static_assert(sizeof(ReadPick) == 16, "sdt_read_pick is four 32-bit words");

constexpr uint32_t PICK_KEPT = 0, PICK_KEPT_DRAW = 1, PICK_DROPPED_DRAW = 2, PICK_ABERRANT = 3, PICK_SHORT = 4;
constexpr uint32_t PICK_OWN_ABERRANT = 1u << 4;
constexpr uint32_t PICK_ABSENT = 0xFFFFFFFFu;            // verdict of a record that no read has written (kept form: the array is preset)
constexpr uint32_t PICK_SAT = 65535u;                    // the dispersion is computed on counts saturated here

// stdev / mean > max_cv_pct / 100 without a division: 10000 * (n * S2 - S1^2) > max_cv_pct^2 * S1^2.  n <= 65 536 and the saturated
// counts keep n * S2 and S1^2 below 2^64; the two products need up to 124 bits.
__device__ inline bool pick_aberrant(uint32_t n, uint64_t s1, uint64_t s2, uint32_t max_cv_pct)
{
	if (!max_cv_pct) return false;
	const uint64_t q = s1 * s1, d = (uint64_t)n * s2 - q;
	const uint64_t cv2 = (uint64_t)max_cv_pct * max_cv_pct;
	return (unsigned __int128)d * 10000u > (unsigned __int128)cv2 * q;
}

// pick[out_base + r * out_stride] for read r: a dense batch has (0, 1); the kept reads of a paired stream their read ordinals.
// LDS: max_kmers 32-bit counts per wave.
template <int NW>
__global__ __launch_bounds__(TPB) void k_pick_stats(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                    int K, Table<NW> tbl, HiView hv, uint32_t max_cv_pct, int max_kmers, int waves_per_block,
                                                    ReadPick *__restrict__ pick, uint64_t out_base, uint64_t out_stride,
                                                    unsigned long long *too_long)
{
	extern __shared__ uint32_t smem_pick[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (wave >= waves_per_block) return;
	uint32_t *cnt = smem_pick + (size_t)wave * (size_t)max_kmers;
	uint32_t bad = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)waves_per_block + wave; r < nreads; r += (uint64_t)gridDim.x * waves_per_block) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		ReadPick rec = {0, 0, 0, 0};
		ReadPick *dst = pick + (out_base + r * out_stride);
		if (len < (uint64_t)K || len - (uint64_t)K + 1 > (uint64_t)max_kmers) {
			if (len >= (uint64_t)K) {                                    // longer than promised: marked, never read
				rec.kmers = COV_TOO_LONG;
				bad++;
			}
			if (lane == 0) *dst = rec;
			continue;
		}
		const int n = (int)(len - (uint64_t)K) + 1;
		uint32_t mn = ~0u, mx = 0;
		uint64_t s1 = 0, s2 = 0;
		for (int j = lane; j < n; j += 64) {
			const Key<NW> fw = global_kmer<NW>(words, start + (uint64_t)j, K);
			const Key<NW> rc = key_revcomp<NW>(fw, K);
			bool f;
			const uint32_t c = lookup_count<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f);
			cnt[j] = c;
			mn = c < mn ? c : mn;
			mx = c > mx ? c : mx;
			const uint32_t cs = c < PICK_SAT ? c : PICK_SAT;
			s1 += cs;
			s2 += (uint64_t)(cs * cs);                                   // (65 535^2 < 2^32)
		}
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) {
			const uint32_t a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
			mn = a < mn ? a : mn;
			mx = b > mx ? b : mx;
			s1 += __shfl_xor(s1, d);
			s2 += __shfl_xor(s2, d);
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();
		rec.kmers = (uint32_t)n;
		rec.median = strip_lower_median(cnt, n, mn, mx, lane);
		rec.verdict = pick_aberrant((uint32_t)n, s1, s2, max_cv_pct) ? PICK_OWN_ABERRANT : 0u;
		if (lane == 0) *dst = rec;
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();                                 // the strip is reused
	}
	if (lane == 0 && bad) atomicAdd(too_long, (unsigned long long)bad);
}

// a stretch of units: unit unit0 + t is the read at record ord0 + t * stride, and with stride == 2 its mate at the next record
// (sdt_read_plan.h: cut_unit_stretches makes the list of the kept form)
using UnitSeg = UnitStretch;

// one lane per unit.  segs == NULL: the one stretch `dense`.  npick: records of pick[] (a mate past it is not there).  The unit's id
// in the draw is id_base + the record index of its first read.  keep (may be NULL) is indexed like pick.  A record whose verdict
// is PICK_ABSENT belongs to no read: it is left as it is, and its mate is judged alone.  (static: sdt_trim.hip includes this header too)
static __global__ __launch_bounds__(TPB) void k_pick_decide(ReadPick *__restrict__ pick, uint64_t npick, const UnitSeg *__restrict__ segs,
                                                            uint32_t nsegs, UnitSeg dense, uint64_t nunits, uint64_t id_base, uint32_t target,
                                                            uint64_t seed, uint8_t *__restrict__ keep, unsigned long long *n_kept)
{
	uint32_t mine = 0;
	for (uint64_t u0 = blockIdx.x * (uint64_t)TPB; u0 < nunits; u0 += (uint64_t)gridDim.x * TPB) {
		const uint64_t u = u0 + threadIdx.x;
		if (u >= nunits) continue;
		UnitSeg sg = dense;
		if (segs) {                                                      // the last stretch that starts at or before u
			uint32_t lo = 0, hi = nsegs;
			while (hi - lo > 1) {
				const uint32_t mid = lo + ((hi - lo) >> 1);
				if (segs[mid].unit0 <= u) lo = mid; else hi = mid;
			}
			sg = segs[lo];
		}
		const uint64_t at[2] = {sg.ord0 + (u - sg.unit0) * sg.stride, sg.ord0 + (u - sg.unit0) * sg.stride + 1};
		const int mates = sg.stride == 2 ? 2 : 1;
		bool here[2] = {false, false}, ab = false;
		uint32_t own[2] = {0, 0};
		int with_kmers = 0, present = 0;
		uint64_t sum = 0;
#pragma unroll
		for (int m = 0; m < 2; m++) {
			if (m >= mates || at[m] >= npick) continue;
			const ReadPick p = pick[at[m]];
			if (p.verdict == PICK_ABSENT) continue;
			here[m] = true;
			present++;
			if (p.kmers == COV_TOO_LONG) { own[m] = COV_TOO_LONG; continue; }
			own[m] = p.verdict & PICK_OWN_ABERRANT;
			if (p.kmers) {
				with_kmers++;
				sum += p.median;
				ab = ab || own[m];
			}
		}
		if (!present) continue;
		const uint32_t cov = with_kmers == 2 ? (uint32_t)((sum + 1) >> 1) : (uint32_t)sum;
		uint32_t v;
		if (!with_kmers) v = PICK_SHORT;
		else if (ab) v = PICK_ABERRANT;
		else if (cov <= target) v = PICK_KEPT;
		else {
			const uint64_t draw = mix64(seed ^ ((id_base + at[0]) * 0x9E3779B97F4A7C15ULL)) >> 32;
			v = draw * cov < ((uint64_t)target << 32) ? PICK_KEPT_DRAW : PICK_DROPPED_DRAW;
		}
#pragma unroll
		for (int m = 0; m < 2; m++) {
			if (!here[m]) continue;
			const bool too_long = own[m] == COV_TOO_LONG;                // its record says so and nothing else: dropped as short
			pick[at[m]].cov = too_long ? 0u : cov;
			pick[at[m]].verdict = too_long ? PICK_SHORT : v | own[m];
			const bool k = !too_long && v <= PICK_KEPT_DRAW;
			if (keep) keep[at[m]] = k ? 1 : 0;
			mine += k;
		}
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		mine += __shfl_xor(mine, d);
	if ((threadIdx.x & 63) == 0 && mine)
		atomicAdd(n_kept, (unsigned long long)mine);
}

// ---- compaction -------------------------------------------------------------------------------------------------------------------
// what the two scans run over: the kept length of read r and whether it is kept (entry nreads is 0: the scans' last output is the total)
struct KeptLen {
	const uint8_t *keep;
	const uint64_t *offs;
	uint64_t nreads;
	__device__ uint64_t operator()(uint64_t r) const { return r < nreads && keep[r] ? offs[r + 1] - offs[r] : 0; }
};
struct KeptFlag {
	const uint8_t *keep;
	uint64_t nreads;
	__device__ uint64_t operator()(uint64_t r) const { return r < nreads && keep[r] ? 1 : 0; }
};

// new_off / rank: the exclusive scans over nreads + 1 entries.  Kept read r becomes output read rank[r]: its new offset and where its
// bases start in the input; entry rank[nreads] closes the offsets.
static __global__ __launch_bounds__(TPB) void k_compact_place(const uint8_t *__restrict__ keep, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                              const uint64_t *__restrict__ new_off, const uint64_t *__restrict__ rank,
                                                              uint64_t *__restrict__ out_offs, uint64_t *__restrict__ src_start)
{
	for (uint64_t r = blockIdx.x * (uint64_t)TPB + threadIdx.x; r <= nreads; r += (uint64_t)gridDim.x * TPB) {
		if (r < nreads && !keep[r]) continue;
		out_offs[rank[r]] = new_off[r];
		if (r < nreads) src_start[rank[r]] = offs[r];
	}
}

// 16 bases of the stream from base s on, first base in the most significant pair (the words are readable TAIL_PAD past the last base)
__device__ inline uint32_t stream_word_at(const uint32_t *__restrict__ words, uint64_t s)
{
	const uint64_t two = (uint64_t)words[s >> 4] << 32 | words[(s >> 4) + 1];
	return (uint32_t)((two << (2 * (int)(s & 15))) >> 32);
}

// output word w holds bases [16 w, 16 w + 16) of the compacted stream: the read that holds base 16 w by binary search in the new
// offsets, then up to 16 bases, on into the following kept reads.  Words [n_out_words, n_out_words + TAIL_PAD) are the pad.
static __global__ __launch_bounds__(TPB) void k_compact_words(const uint32_t *__restrict__ words, const uint64_t *__restrict__ out_offs,
                                                              const uint64_t *__restrict__ src_start, uint64_t n_out_reads, uint64_t n_out_words,
                                                              uint32_t *__restrict__ out_words)
{
	for (uint64_t w = blockIdx.x * (uint64_t)TPB + threadIdx.x; w < n_out_words + TAIL_PAD; w += (uint64_t)gridDim.x * TPB) {
		uint32_t out = 0;
		if (w < n_out_words) {
			uint64_t b = w << 4;
			uint64_t lo = 0, hi = n_out_reads;                           // the last read that starts at or before b: it holds b, b < total
			while (hi - lo > 1) {
				const uint64_t mid = lo + ((hi - lo) >> 1);
				if (out_offs[mid] <= b) lo = mid; else hi = mid;
			}
			int filled = 0;
			for (uint64_t k = lo; filled < 16 && k < n_out_reads; k++) {
				const uint64_t begin = out_offs[k], end = out_offs[k + 1];
				if (end <= b) continue;                                  // (an empty kept read)
				const uint64_t avail = end - b;
				const int take = avail < (uint64_t)(16 - filled) ? (int)avail : 16 - filled;
				const uint32_t bits = stream_word_at(words, src_start[k] + (b - begin)) & ~(take == 16 ? 0u : 0xFFFFFFFFu >> (2 * take));
				out |= bits >> (2 * filled);
				filled += take;
				b += (uint64_t)take;
			}
		}
		out_words[w] = out;
	}
}

} // namespace sdt
