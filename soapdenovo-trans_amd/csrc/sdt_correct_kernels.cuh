// sdt_correct_kernels.cuh -- k-mer-spectrum correction of substitution errors against the counted node table (read-only):
//   k_correct_reads : one wavefront per read, the shape of k_profile_reads.  Phase 1 is the profile's look-up loop: the 32-bit count of
//                     every k-mer of the read into an LDS strip.  Phase 2 finds the runs of weak k-mers (count < min_count) in the
//                     strip and walks them in a wave-uniform loop; a run whose shape says "one wrong base at p" (include/sdt_gpu.h)
//                     has its 3 alternatives tried, the lanes sharing the 3 * l look-ups, and is fixed when exactly one alternative
//                     makes every k-mer of the run solid.  Every run is judged on the ORIGINAL read: a substitution at p only changes
//                     k-mers of its own run, so runs do not interact and nothing is looked up twice.
// The kernel writes neither the table nor the input stream: the substitutions go into a copy of the stream (one 32-bit atomicXor per
// edit -- two reads can share a word) and into a list of edits behind a device counter.
#pragma once
#include "sdt_search_kernels.cuh"

namespace sdt {

struct ReadFix {                                         // == sdt_read_fix of include/sdt_gpu.h
	uint32_t kmers, weak, runs, fixed;
};
static_assert(sizeof(ReadFix) == 16, "sdt_read_fix is four 32-bit words");

constexpr int FIX_MAX_RUN = 127;                         // a candidate run has at most K <= 127 k-mers: two ballots find its end

// what judge_weak_run found for a run that is to be fixed: the run's k-mers [a, a + l), base p of the read becomes neu
struct RunFix {
	int l, p;
	uint32_t old, neu;
};

// The judgement of the run of weak k-mers that starts at k-mer a of a read (the rule: include/sdt_gpu.h), for the whole wave: the
// run's shape, the 3 * l look-ups of its alternatives shared among the lanes, and "exactly one alternative makes every k-mer of
// the run solid".  cnt: the read's counts in the wave's strip (fenced by the caller), n of them.  Uniform over the wave; reads the
// strip, the stream and the table only.  (k_correct_reads, k_trim_reads)
template <int NW>
__device__ inline RunFix judge_weak_run(const uint32_t *words, uint64_t start, int n, int K, const Table<NW> &tbl, const HiView &hv,
                                      uint32_t min_count, const uint32_t *cnt, int a, int lane)
{
	// the run's length, as far as it matters: the first solid k-mer (or the read's end) among the next 128
	int l = FIX_MAX_RUN + 1;
#pragma unroll
	for (int t = 1; t >= 0; t--) {
		const int q = a + 64 * t + lane;
		const unsigned long long ends = __ballot(q >= n || cnt[q] >= min_count);
		if (ends) l = 64 * t + (int)__builtin_ctzll(ends);
	}
	const RunFix none = {0, 0, 0, 0};
	if (l > K) return none;
	const int b = a + l - 1;
	const bool head = a == 0, tail = b == n - 1;
	if (head && tail) return none;                                   // nothing solid in the read
	if (!head && !tail && l != K) return none;
	const int p = tail ? a + K - 1 : b;                              // every k-mer of [a, b] holds base p
	// look-up t of 3 * l: alternative old ^ (t / l + 1) in k-mer a + t % l
	uint32_t invalid = 0;
	for (int t0 = 0; t0 < 3 * l; t0 += 64) {
		const int t = t0 + lane;
		const bool active = t < 3 * l;
		const int alt = active ? t / l : 0, j = a + (active ? t - alt * l : 0);
		Key<NW> fw = global_kmer<NW>(words, start + (uint64_t)j, K);
		const int bit = 2 * (K - 1 - (p - j));
#pragma unroll
		for (int wd = 0; wd < NW; wd++)
			if (wd == NW - 1 - (bit >> 6)) fw.w[wd] ^= (uint64_t)(alt + 1) << (bit & 63);
		const Key<NW> rc = key_revcomp<NW>(fw, K);
		bool f;
		const uint32_t c = lookup_count<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f);         // (lanes past 3 * l look k-mer a up again)
		const bool miss = active && c < min_count;
#pragma unroll
		for (int x = 0; x < 3; x++)
			if (__ballot(miss && alt == x)) invalid |= 1u << x;
	}
	if (__popc(invalid) != 2) return none;                           // none or several alternatives fit
	const uint64_t g = start + (uint64_t)p;
	const uint32_t old = (words[g >> 4] >> (30 - 2 * (int)(g & 15))) & 3u;
	return RunFix{l, p, old, old ^ (uint32_t)(__ffs((int)(~invalid & 7u)))};
}

// fix[r] for read r of the batch (dense).  An edit is (edit_base + r * edit_stride) << 18 | pos << 2 | new_base: (0, 1) for a batch,
// the read ordinals for a kept batch.  out_words: NULL, or a copy of `words` made before the launch.  edits: NULL, or max_edits
// words; *n_edits counts every edit, stored or not.  LDS: max_kmers 32-bit counts per wave.
template <int NW>
__global__ __launch_bounds__(TPB) void k_correct_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                       int K, Table<NW> tbl, HiView hv, uint32_t min_count, int max_kmers, int waves_per_block,
                                                       ReadFix *__restrict__ fix, uint32_t *out_words, unsigned long long *edits,
                                                       unsigned long long max_edits, unsigned long long *n_edits, uint64_t edit_base,
                                                       uint64_t edit_stride, unsigned long long *too_long)
{
	extern __shared__ uint32_t smem_fix[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (wave >= waves_per_block) return;
	uint32_t *cnt = smem_fix + (size_t)wave * (size_t)max_kmers;
	uint32_t bad = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)waves_per_block + wave; r < nreads; r += (uint64_t)gridDim.x * waves_per_block) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		ReadFix rec = {0, 0, 0, 0};
		if (len < (uint64_t)K || len - (uint64_t)K + 1 > (uint64_t)max_kmers) {
			if (len >= (uint64_t)K) {                                    // longer than promised: marked, never read
				rec.kmers = COV_TOO_LONG;
				bad++;
			}
			if (lane == 0) fix[r] = rec;
			continue;
		}
		const int n = (int)(len - (uint64_t)K) + 1;
		// phase 1: the counts of the read's k-mers, as k_profile_reads sees them
		uint32_t nweak = 0;
		for (int j = lane; j < n; j += 64) {
			const Key<NW> fw = global_kmer<NW>(words, start + (uint64_t)j, K);
			const Key<NW> rc = key_revcomp<NW>(fw, K);
			bool f;
			const uint32_t c = lookup_count<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f);
			cnt[j] = c;
			nweak += c < min_count;
		}
#pragma unroll
		for (int d = 32; d > 0; d >>= 1)
			nweak += __shfl_xor(nweak, d);
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();
		// phase 2: run starts 64 k-mers at a time, then run by run (uniform over the wave: nweak, the ballots and the strip are)
		uint32_t nruns = 0, nfixed = 0;
		for (int base = 0; nweak && base < n; base += 64) {
			const int s = base + lane;
			const bool w = s < n && cnt[s] < min_count;
			const bool pw = s > 0 && s < n && cnt[s - 1] < min_count;
			unsigned long long starts = __ballot(w && !pw);
			nruns += (uint32_t)__popcll(starts);
			while (starts) {
				const int a = base + (int)__builtin_ctzll(starts);
				starts &= starts - 1;
				const RunFix rf = judge_weak_run<NW>(words, start, n, K, tbl, hv, min_count, cnt, a, lane);
				if (!rf.l) continue;
				const uint64_t g = start + (uint64_t)rf.p;
				nfixed++;
				if (lane == 0) {
					if (out_words) atomicXor(out_words + (g >> 4), (rf.old ^ rf.neu) << (30 - 2 * (int)(g & 15)));
					const unsigned long long at = atomicAdd(n_edits, 1ULL);
					if (edits && at < max_edits)
						edits[at] = (unsigned long long)(edit_base + r * edit_stride) << 18 | (unsigned long long)rf.p << 2 | rf.neu;
				}
			}
		}
		rec.kmers = (uint32_t)n;
		rec.weak = nweak;
		rec.runs = nruns;
		rec.fixed = nfixed;
		if (lane == 0) fix[r] = rec;
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();                                 // the strip is reused
	}
	if (lane == 0 && bad) atomicAdd(too_long, (unsigned long long)bad);
}

} // namespace sdt
