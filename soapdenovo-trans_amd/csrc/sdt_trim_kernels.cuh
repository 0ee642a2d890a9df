// sdt_trim_kernels.cuh -- reads cut back to their longest solid stretch against the counted node table (read-only; the rule:
// include/sdt_gpu.h):
//   k_trim_reads    : one wavefront per read, the shape of k_profile_reads.  Phase 1 is the profile's look-up loop: the 32-bit count of
//                     every k-mer of the read into an LDS strip, min, max and the number of weak k-mers (count < min_count) carried
//                     per lane; then the lower median by strip_lower_median, before anything overwrites the strip.  Under
//                     SDT_TRIM_CORRECTED phase 2 walks the runs of weak k-mers as k_correct_reads does and judges each with the same
//                     judge_weak_run; a run that would be fixed has its strip entries lifted to min_count.  Phase 3 scans the strip
//                     64 k-mers at a time, one ballot of "solid" each, carries the open stretch across the chunks and keeps the
//                     longest (the first among equals).  Everything after phase 1 is uniform over the wave.
//   k_trim_place    : k_compact_place for a range per read: read r contributes bases [offs[r] + start, + len) of its record, clamped to
//                     the read; len == 0 leaves it out.  k_compact_words then packs the ranges as it packs whole reads.
#pragma once
#include "sdt_correct_kernels.cuh"
#include "sdt_select_kernels.cuh"

namespace sdt {

struct ReadTrim {                                        // == sdt_read_trim of include/sdt_gpu.h
	uint32_t kmers, weak, median, start, len, verdict;
};
static_assert(sizeof(ReadTrim) == 24, "sdt_read_trim is six 32-bit words");
struct TrimParams {                                      // == sdt_trim_params
	uint32_t min_count, min_cov, min_len, flags;
};
static_assert(sizeof(TrimParams) == 16, "sdt_trim_params is four 32-bit words");

constexpr uint32_t TRIM_WHOLE = 0, TRIM_GATED = 1, TRIM_TRIMMED = 2, TRIM_DROPPED = 3, TRIM_SHORT = 4;
constexpr uint32_t TRIM_CORRECTED = 1u;                  // == SDT_TRIM_CORRECTED

// trim[r] for read r of the batch (dense); keep (may be NULL) likewise.  LDS: max_kmers 32-bit counts per wave.
template <int NW>
__global__ __launch_bounds__(TPB) void k_trim_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                    int K, Table<NW> tbl, HiView hv, TrimParams prm, int max_kmers, int waves_per_block,
                                                    ReadTrim *__restrict__ trim, uint8_t *__restrict__ keep, unsigned long long *too_long,
                                                    unsigned long long *n_kept)
{
	extern __shared__ uint32_t smem_trim[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (wave >= waves_per_block) return;
	uint32_t *cnt = smem_trim + (size_t)wave * (size_t)max_kmers;
	const uint32_t min_count = prm.min_count;
	uint32_t bad = 0, kept = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)waves_per_block + wave; r < nreads; r += (uint64_t)gridDim.x * waves_per_block) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		ReadTrim rec = {0, 0, 0, 0, 0, TRIM_SHORT};
		if (len < (uint64_t)K || len - (uint64_t)K + 1 > (uint64_t)max_kmers) {
			if (len >= (uint64_t)K) {                                    // longer than promised: marked, never read
				rec.kmers = COV_TOO_LONG;
				bad++;
			}
			if (lane == 0) {
				trim[r] = rec;
				if (keep) keep[r] = 0;
			}
			continue;
		}
		const int n = (int)(len - (uint64_t)K) + 1;
		// phase 1: the counts of the read's k-mers, as k_profile_reads sees them
		uint32_t mn = ~0u, mx = 0, nweak = 0;
		for (int j = lane; j < n; j += 64) {
			const Key<NW> fw = global_kmer<NW>(words, start + (uint64_t)j, K);
			const Key<NW> rc = key_revcomp<NW>(fw, K);
			bool f;
			const uint32_t c = lookup_count<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f);
			cnt[j] = c;
			mn = c < mn ? c : mn;
			mx = c > mx ? c : mx;
			nweak += c < min_count;
		}
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) {
			const uint32_t a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
			mn = a < mn ? a : mn;
			mx = b > mx ? b : mx;
			nweak += __shfl_xor(nweak, d);
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();
		rec.kmers = (uint32_t)n;
		rec.weak = nweak;
		rec.median = strip_lower_median(cnt, n, mn, mx, lane);           // (of the read as it came: the strip is still untouched)
		// phase 2: the runs that k_correct_reads would fix become solid (its walk: run starts 64 k-mers at a time, then run by run)
		uint32_t left = nweak;
		if (prm.flags & TRIM_CORRECTED) {
			for (int base = 0; left && base < n; base += 64) {
				const int s = base + lane;
				const bool w = s < n && cnt[s] < min_count;
				const bool pw = s > 0 && s < n && cnt[s - 1] < min_count;
				unsigned long long starts = __ballot(w && !pw);
				while (starts) {
					const int a = base + (int)__builtin_ctzll(starts);
					starts &= starts - 1;
					const RunFix rf = judge_weak_run<NW>(words, start, n, K, tbl, hv, min_count, cnt, a, lane);
					if (!rf.l) continue;
					// (k-mers [a, a + l) are weak and l <= K <= 127; nobody reads them again before the scan: the runs that follow lie
					// behind the solid k-mer that ended this one)
					for (int t = lane; t < rf.l; t += 64)
						cnt[a + t] = min_count;
					left -= (uint32_t)rf.l;
				}
				__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
				__builtin_amdgcn_wave_barrier();                         // the next chunk looks at cnt[base + 63]
			}
		}
		// phase 3: the longest stretch of solid k-mers, the first among equals
		if (left == 0) {
			rec.verdict = TRIM_WHOLE;
			rec.len = (uint32_t)len;
		} else if (prm.min_cov && rec.median < prm.min_cov) {
			rec.verdict = TRIM_GATED;
			rec.len = (uint32_t)len;
		} else {
			int open = -1, best_len = 0, best_start = 0;
			for (int base = 0; base < n; base += 64) {
				const int s = base + lane;
				const unsigned long long m = __ballot(s < n && cnt[s] >= min_count);
				int pos = 0;
				while (pos < 64) {                                       // (every turn but the last passes a stretch's end: 33 turns at most)
					if (open < 0) {
						const unsigned long long rest = m >> pos;
						if (!rest) break;
						pos += (int)__builtin_ctzll(rest);
						open = base + pos;
					}
					const unsigned long long z = ~m >> pos;
					if (!z) break;                                       // solid to the end of the chunk: the stretch stays open
					pos += (int)__builtin_ctzll(z);
					if (base + pos - open > best_len) {
						best_len = base + pos - open;
						best_start = open;
					}
					open = -1;
				}
			}
			if (open >= 0 && n - open > best_len) {                      // (n is a multiple of 64 and the read ends solid)
				best_len = n - open;
				best_start = open;
			}
			const uint32_t bases = best_len ? (uint32_t)(best_len + K - 1) : 0u;
			if (!best_len || bases < prm.min_len) {
				rec.verdict = TRIM_DROPPED;
			} else {
				rec.verdict = TRIM_TRIMMED;
				rec.start = (uint32_t)best_start;
				rec.len = bases;
			}
		}
		kept += rec.len > 0;
		if (lane == 0) {
			trim[r] = rec;
			if (keep) keep[r] = rec.len > 0 ? 1 : 0;
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();                                 // the strip is reused
	}
	if (lane == 0 && bad) atomicAdd(too_long, (unsigned long long)bad);
	if (lane == 0 && kept) atomicAdd(n_kept, (unsigned long long)kept);
}

// ---- compaction of ranges ---------------------------------------------------------------------------------------------------------
// the bases of read r that its record keeps, clamped to the read: [offs[r] + s, + l), l == 0 when nothing is kept
__device__ inline void trim_range(const ReadTrim *__restrict__ trim, const uint64_t *__restrict__ offs, uint64_t r, uint64_t &s, uint64_t &l)
{
	const uint64_t len = offs[r + 1] - offs[r];
	s = trim[r].start;
	l = trim[r].len;
	if (s > len) s = len;
	if (l > len - s) l = len - s;
}

// what the two scans run over (entry nreads is 0: the scans' last output is the total)
struct TrimmedLen {
	const ReadTrim *trim;
	const uint64_t *offs;
	uint64_t nreads;
	__device__ uint64_t operator()(uint64_t r) const
	{
		if (r >= nreads) return 0;
		uint64_t s, l;
		trim_range(trim, offs, r, s, l);
		return l;
	}
};
struct TrimmedFlag {
	const ReadTrim *trim;
	const uint64_t *offs;
	uint64_t nreads;
	__device__ uint64_t operator()(uint64_t r) const
	{
		if (r >= nreads) return 0;
		uint64_t s, l;
		trim_range(trim, offs, r, s, l);
		return l ? 1 : 0;
	}
};

// new_off / rank: the exclusive scans over nreads + 1 entries.  A read with kept bases becomes output read rank[r]: its new offset and
// where its kept bases start in the input; entry rank[nreads] closes the offsets.
static __global__ __launch_bounds__(TPB) void k_trim_place(const ReadTrim *__restrict__ trim, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                           const uint64_t *__restrict__ new_off, const uint64_t *__restrict__ rank,
                                                           uint64_t *__restrict__ out_offs, uint64_t *__restrict__ src_start)
{
	for (uint64_t r = blockIdx.x * (uint64_t)TPB + threadIdx.x; r <= nreads; r += (uint64_t)gridDim.x * TPB) {
		uint64_t s = 0, l = 1;
		if (r < nreads) trim_range(trim, offs, r, s, l);
		if (!l) continue;
		out_offs[rank[r]] = new_off[r];
		if (r < nreads) src_start[rank[r]] = offs[r] + s;
	}
}

} // namespace sdt
