// sdt_search_kernels.cuh -- read-only questions to the counted node table:
//   k_search_kmers  : search_kmerset (newhash.c:239-283) for a batch of k-mers, one lane per query.  Every reference caller
//                     canonicalises first (e.g. prlRead2path.c:363-394: the smaller of word and its reverse complement); so does the lane.
//   k_profile_reads : the k-mer coverage of a read -- chopKmer4read's k-mers (prlHashReads.c:164-310) looked up instead of inserted --
//                     one wavefront per read, the shape of k_align_reads: counts into an LDS strip, then min / median / max and the
//                     found / solid tallies, uniform over the wave.
//   k_hi_count / k_hi_fill : the handful of nodes counted more than 65 535 times, into a small hash keyed by table slot.
//
// A node's count is split: bits 15..0 sit in the entry's val, bits 31..16 in aux[slot] -- a second random cache line per look-up.
// k_search_kmers reads it (it needs aux's flag bits anyway).  k_profile_reads does not: the slots with a non-zero high half are
// collected once per state of the table (streaming scan of aux) into a hash of a few KiB that stays cache-resident, and the kernel
// probes that -- or nothing at all when no node got that far, the common case (HI_NONE).
#pragma once
#include "sdt_ctg_kernels.cuh"

namespace sdt {

struct ReadCov {                                         // == sdt_read_cov of include/sdt_gpu.h
	uint32_t kmers, found, solid, min, median, max;
};
static_assert(sizeof(ReadCov) == 24, "sdt_read_cov is six 32-bit words");

constexpr uint32_t COV_TOO_LONG = 0xFFFFFFFFu;           // ReadCov.kmers of a read longer than the caller promised

// where the high half of a count comes from
constexpr int HI_NONE = 0;                               // no node of the table has one
constexpr int HI_HASH = 1;                               // the small hash: word = (slot + 1) << 16 | high half, 0 = empty
constexpr int HI_AUX = 2;                                // aux[slot] itself

struct HiView {
	const uint64_t *tab;
	uint64_t mask;                                       // slots of the hash - 1 (a power of two)
	int mode;
};

__device__ inline uint32_t hi_lookup(const HiView &hv, const uint32_t *__restrict__ aux, uint64_t slot)
{
	if (hv.mode == HI_AUX) return aux[slot] & 0xFFFFu;
	if (hv.mode == HI_NONE) return 0;
	for (uint64_t h = mix64(slot) & hv.mask;; h = (h + 1) & hv.mask) {      // (load <= 1/4: an empty word ends every probe)
		const uint64_t w = hv.tab[h];
		if (!w) return 0;
		if ((w >> 16) == slot + 1) return (uint32_t)(w & 0xFFFFu);
	}
}

static __global__ __launch_bounds__(TPB) void k_hi_count(const uint32_t *__restrict__ aux, uint64_t slots, unsigned long long *n_hi)
{
	uint32_t mine = 0;
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB)
		mine += (aux[s] & 0xFFFFu) != 0;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		mine += __shfl_down(mine, d);
	if ((threadIdx.x & 63) == 0 && mine)
		atomicAdd(n_hi, (unsigned long long)mine);
}

static __global__ __launch_bounds__(TPB) void k_hi_fill(const uint32_t *__restrict__ aux, uint64_t slots, uint64_t *tab, uint64_t mask)
{
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		const uint32_t hi = aux[s] & 0xFFFFu;
		if (!hi) continue;
		const uint64_t w = ((s + 1) << 16) | hi;
		for (uint64_t h = mix64(s) & mask;; h = (h + 1) & mask)
			if (atomicCAS((unsigned long long *)&tab[h], 0ULL, (unsigned long long)w) == 0ULL) break;
	}
}

// the 32-bit count of `k` (0 = absent); one entry read per probe, key + val in one 16-byte load for 1-word keys (lookup_val)
template <int NW>
__device__ inline uint32_t lookup_count(const Table<NW> &tbl, const Key<NW> &k, const HiView &hv, bool &found)
{
	uint64_t slot, lo, n;
	probe_begin<NW>(tbl, k, slot, lo, n);
	found = false;
	for (uint64_t probe = 0; probe < n; probe++, slot = probe_next(slot, lo, n)) {
		uint64_t val;
		if constexpr (NW == 1) {
			const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(tbl.ent + slot);
			if (kv.x == KEY_EMPTY) return 0;
			if (kv.x != k.w[0]) continue;
			val = kv.y;
		} else {
			const Entry<NW> *e = tbl.ent + slot;
			if (e->key[0] == KEY_EMPTY) return 0;
			bool same = true;
#pragma unroll
			for (int w = 0; w < NW; w++) same = same && e->key[w] == k.w[w];
			if (!same) continue;
			val = e->val;
		}
		found = true;
		return (uint32_t)(val >> 48) | (hi_lookup(hv, tbl.aux, slot) << 16);
	}
	return 0;
}

// lookup_count's sibling for the one caller that needs the node as well as its count (k_asm_support tallies by slot): the same probe,
// the same loads, and slot_out is set iff found
template <int NW>
__device__ inline uint32_t lookup_count_slot(const Table<NW> &tbl, const Key<NW> &k, const HiView &hv, bool &found, uint64_t &slot_out)
{
	uint64_t slot, lo, n;
	probe_begin<NW>(tbl, k, slot, lo, n);
	found = false;
	for (uint64_t probe = 0; probe < n; probe++, slot = probe_next(slot, lo, n)) {
		uint64_t val;
		if constexpr (NW == 1) {
			const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(tbl.ent + slot);
			if (kv.x == KEY_EMPTY) return 0;
			if (kv.x != k.w[0]) continue;
			val = kv.y;
		} else {
			const Entry<NW> *e = tbl.ent + slot;
			if (e->key[0] == KEY_EMPTY) return 0;
			bool same = true;
#pragma unroll
			for (int w = 0; w < NW; w++) same = same && e->key[w] == k.w[w];
			if (!same) continue;
			val = e->val;
		}
		found = true;
		slot_out = slot;
		return (uint32_t)(val >> 48) | (hi_lookup(hv, tbl.aux, slot) << 16);
	}
	return 0;
}

// status[i]: bit 0 found, bit 1 the query is the larger strand (the node is stored as its reverse complement; set whether or not
// the node exists).  count / l_links / r_flags: the words k_export writes for the node, as the STORED node has them; 0 when absent.
template <int NW>
__global__ __launch_bounds__(TPB) void k_search_kmers(const uint64_t *__restrict__ keys, uint64_t n, int K, Table<NW> tbl,
                                                      uint32_t *__restrict__ count, uint32_t *__restrict__ l_links,
                                                      uint32_t *__restrict__ r_flags, uint8_t *__restrict__ status)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		Key<NW> fw;
#pragma unroll
		for (int w = 0; w < NW; w++) fw.w[w] = keys[i * NW + w];
		const Key<NW> rc = key_revcomp<NW>(fw, K);
		const bool smaller = key_less<NW>(fw, rc);
		uint64_t slot;
		uint32_t cnt = 0, l = 0, rf = 0;
		uint8_t st = smaller ? 0 : 2;
		if (table_find<NW>(tbl, smaller ? fw : rc, slot)) {
			const uint64_t val = tbl.ent[slot].val;
			const uint32_t aux = tbl.aux[slot];
			cnt = ((aux & 0xFFFFu) << 16) | (uint32_t)(val >> 48);
			l = (uint32_t)(val & 0xFFFFFFu);
			rf = (uint32_t)((val >> 24) & 0xFFFFFFu) | ((aux & AUX_LINEAR) ? 1u << 24 : 0u) | ((aux & AUX_DELETED) ? 1u << 25 : 0u) |
			     (cnt == 1 ? 1u << 27 : 0u);
			st |= 1;
		}
		if (count) count[i] = cnt;
		if (l_links) l_links[i] = l;
		if (r_flags) r_flags[i] = rf;
		if (status) status[i] = st;
	}
}

// lower median = element (n - 1) / 2 in ascending order of the n counts in a wave's LDS strip, by radix select: every count lies in
// [mn, mx], so all of them share the bits above the highest bit in which mn and mx differ; below it one ballot per bit and 64 k-mers
// decides the next bit.  Uniform over the wave; the caller has fenced the strip.  (k_profile_reads, k_pick_stats)
__device__ inline uint32_t strip_lower_median(const uint32_t *cnt, int n, uint32_t mn, uint32_t mx, int lane)
{
	uint32_t med = mn;
	if (mn != mx) {
		const int top = 31 - __clz(mn ^ mx);
		uint32_t rank = (uint32_t)(n - 1) >> 1;
		med = top == 31 ? 0u : mx & ~((2u << top) - 1u);
		for (int b = top; b >= 0; b--) {
			uint32_t zeros = 0;                                          // counts that match `med` above bit b and have bit b clear
			for (int base = 0; base < n; base += 64) {
				const int s = base + lane;
				const uint32_t v = s < n ? cnt[s] : 0u;
				const bool z = s < n && ((uint64_t)(v ^ med) >> (b + 1)) == 0 && !((v >> b) & 1u);
				zeros += (uint32_t)__popcll(__ballot(z));
			}
			if (rank >= zeros) {
				rank -= zeros;
				med |= 1u << b;
			}
		}
	}
	return med;
}

// out[out_base + r * out_stride] for read r: a dense batch has (0, 1); the kept reads of a paired stream their read ordinals.
// LDS: max_kmers 32-bit counts per wave.
template <int NW>
__global__ __launch_bounds__(TPB) void k_profile_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                       int K, Table<NW> tbl, HiView hv, uint32_t min_count, int max_kmers, int waves_per_block,
                                                       ReadCov *__restrict__ out, uint64_t out_base, uint64_t out_stride,
                                                       unsigned long long *too_long)
{
	extern __shared__ uint32_t smem_cov[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (wave >= waves_per_block) return;
	uint32_t *cnt = smem_cov + (size_t)wave * (size_t)max_kmers;
	uint32_t bad = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)waves_per_block + wave; r < nreads; r += (uint64_t)gridDim.x * waves_per_block) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		ReadCov rec = {0, 0, 0, 0, 0, 0};
		ReadCov *dst = out + (out_base + r * out_stride);
		if (len < (uint64_t)K || len - (uint64_t)K + 1 > (uint64_t)max_kmers) {
			if (len >= (uint64_t)K) {                                    // longer than promised: marked, never read
				rec.kmers = COV_TOO_LONG;
				bad++;
			}
			if (lane == 0) *dst = rec;
			continue;
		}
		const int n = (int)(len - (uint64_t)K) + 1;
		uint32_t mn = ~0u, mx = 0, nfound = 0, nsolid = 0;
		for (int j = lane; j < n; j += 64) {
			const Key<NW> fw = global_kmer<NW>(words, start + (uint64_t)j, K);
			const Key<NW> rc = key_revcomp<NW>(fw, K);
			bool f;
			const uint32_t c = lookup_count<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f);
			cnt[j] = c;
			mn = c < mn ? c : mn;
			mx = c > mx ? c : mx;
			nfound += f;
			nsolid += c >= min_count;
		}
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) {
			const uint32_t a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
			mn = a < mn ? a : mn;
			mx = b > mx ? b : mx;
			nfound += __shfl_xor(nfound, d);
			nsolid += __shfl_xor(nsolid, d);
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();
		const uint32_t med = strip_lower_median(cnt, n, mn, mx, lane);
		rec.kmers = (uint32_t)n;
		rec.found = nfound;
		rec.solid = nsolid;
		rec.min = mn;
		rec.median = med;
		rec.max = mx;
		if (lane == 0) *dst = rec;
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();                                 // the strip is reused
	}
	if (lane == 0 && bad) atomicAdd(too_long, (unsigned long long)bad);
}

} // namespace sdt
