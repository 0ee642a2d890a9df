// sdt_cluster_kernels.cuh -- the counted node table as a graph (the rule: include/sdt_gpu.h): the connected components of its live
// nodes under their link counters, one 32-bit label per slot, and the reads' clusters from those labels.  Nothing here writes ent or
// aux; what is written by slot are two arrays of the context's own: label (kept) and work (freed by cluster_begin).
//   k_cl_init<NW>    : one lane per slot, grid-stride: label[s] = s for a live node, CL_NONE for everything else.  label is the
//                      union-find's parent[] until k_cl_rank.  Counts the live nodes and the nodes that are not.
//   k_cl_unite<NW>   : one lane per slot: a live node walks its link counters >= min_link, finds the neighbour's slot (table_find on
//                      the canonical strand) and unites the two when the neighbour is live.  Counts the link ends.
//   cl_find / cl_union : the lock-free union-find of sdt_graph_kernels.cuh (uf_find / uf_union) ordered by KEY instead of by index:
//                      the root with the larger k-mer goes under the root with the smaller.  A cluster's root is then its smallest
//                      k-mer, which is what the id rule sorts by.  What makes it safe is kept: parent[] is read with device-scope
//                      atomic loads and written with device-scope compare-and-swap only, so every exit of find ("p == x") and of
//                      union ("a == b", "the swap returned a") rests on a value from the memory side -- the per-XCD L2s are not
//                      coherent, and a plain load could show a stale self-parent for ever.  parent[] only changes from "root" to
//                      "child of a root with a smaller key" and, by path halving, to an ancestor: keys fall strictly along every
//                      chain, so there is no cycle, and a stale value still leads up the same tree.  The keys of two roots are plain
//                      loads of ent, which nothing writes.
//   k_cl_flatten     : work[s] = the root of s (CL_NONE for a slot without a live node); parent[] is read-only apart from path
//                      halving.  Roots (work[s] == s) are appended to a list, one atomic per wavefront.
//   k_cl_sortkey<NW> : word w of the keys of the roots in their current order: the list is sorted by stable radix passes from the
//                      least significant word (rocprim, sdt_cluster.hip).
//   k_cl_rank<NW>    : the i-th root of the sorted list has id i: label[root] = i, and its key goes to the component list.
//   k_cl_label<NW>   : label[s] = label[work[s]], and nodes / count_sum of the cluster grow by the node.  A large cluster would put
//                      most of the table's atomics on one address, so the lanes of a wavefront that share an id are merged first:
//                      a ballot / readfirstlane loop over the distinct ids, one pair of atomics per id and wavefront.
//   k_cl_lookup<NW>  : one lane per query k-mer, either strand.
//   k_cl_reads<NW>   : one wavefront per UNIT (a read, or the two mates of a pair), 64 consecutive k-mer positions per step -- the
//                      shape of k_asm_support without the tally and without a count: a lane builds its k-mer, finds the canonical
//                      node's slot and reads its label.  Per step one ballot of the live lanes, the first live lane by
//                      count-trailing-zeros, its label broadcast, the mismatches by popcount.  No strip of LDS, no limit on the length.
//                      RESOLVE: lane 0 also decides unit, verdict and keep of the unit's reads; otherwise (the kept form: the mates
//                      sit in different batches) the records go out by ordinal and k_cl_units decides.
//   k_cl_units       : one lane per unit over the ordinal-indexed records, as k_pick_decide.
#pragma once
#include "sdt_search_kernels.cuh"
#include "sdt_read_plan.h"

namespace sdt {

struct ReadCluster {                                     // == sdt_read_cluster of include/sdt_gpu.h
	uint32_t kmers, live, split, cluster, unit, verdict;
};
static_assert(sizeof(ReadCluster) == 24, "sdt_read_cluster is six 32-bit words");

struct ClusterComp {                                     // == sdt_cluster_comp of include/sdt_gpu.h
	unsigned long long count_sum;
	uint32_t nodes, reserved;
};
static_assert(sizeof(ClusterComp) == 16, "sdt_cluster_comp is 16 bytes");

struct ClusterRule {                                     // min_count: already max(min_count, 1); max_count 0: no upper bound
	uint32_t min_count, max_count, min_link;
};

constexpr uint32_t CL_NONE = 0xFFFFFFFFu;                // SDT_CLUSTER_NONE
constexpr uint32_t CL_WHOLE = 0, CL_NOT_WHOLE = 1, CL_THROUGH_MATE = 2, CL_UNASSIGNED = 3, CL_SHORT = 4;
constexpr uint32_t CL_ABSENT = 0xFFFFFFFFu;              // verdict of a record that no read has written (kept form: the array is preset)
// counters of cluster_begin
constexpr int CL_N_LIVE = 0, CL_N_ENDS = 1, CL_N_ROOTS = 2, CL_N_DEAD = 3, CL_COUNTERS = 4;

template <int NW> __device__ inline Key<NW> cl_key_at(const Table<NW> &tbl, uint64_t s)
{
	Key<NW> k;
#pragma unroll
	for (int w = 0; w < NW; w++) k.w[w] = tbl.ent[s].key[w];
	return k;
}

template <int NW> __device__ inline Key<NW> cl_mask(int K)
{
	Key<NW> mask;
#pragma unroll
	for (int i = 0; i < NW; i++) {
		const int bits = 2 * K - 64 * (NW - 1 - i);
		mask.w[i] = bits <= 0 ? 0ULL : (bits >= 64 ? ~0ULL : ((1ULL << bits) - 1ULL));
	}
	return mask;
}

// the word in front of k by base b (left neighbour) and behind it (right neighbour)
template <int NW> __device__ inline Key<NW> cl_prev(const Key<NW> &k, uint32_t b, int K)
{
	Key<NW> r = key_shr<NW>(k, 2);
	const int tb = 2 * (K - 1);
#pragma unroll
	for (int w = 0; w < NW; w++)
		if (w == NW - 1 - (tb >> 6)) r.w[w] |= (uint64_t)b << (tb & 63);
	return r;
}
template <int NW> __device__ inline Key<NW> cl_next(const Key<NW> &k, uint32_t b, const Key<NW> &mask)
{
	Key<NW> r = key_append<NW>(k, b);
#pragma unroll
	for (int i = 0; i < NW; i++) r.w[i] &= mask.w[i];
	return r;
}

__device__ inline bool cl_live(uint64_t key0, uint64_t val, uint32_t aux, const ClusterRule &rule, uint32_t &count)
{
	count = (uint32_t)(val >> 48) | ((aux & 0xFFFFu) << 16);
	return key0 != KEY_EMPTY && !(aux & AUX_DELETED) && count >= rule.min_count && (rule.max_count == 0 || count <= rule.max_count);
}

// key0 and val of slot s (one 16-byte load for 1-word keys)
template <int NW> __device__ inline void cl_load(const Table<NW> &tbl, uint64_t s, uint64_t &key0, uint64_t &val)
{
	if constexpr (NW == 1) {
		const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(tbl.ent + s);
		key0 = kv.x;
		val = kv.y;
	} else {
		key0 = tbl.ent[s].key[0];
		val = tbl.ent[s].val;
	}
}

__device__ inline uint32_t cl_wave_sum(uint32_t v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_init(Table<NW> tbl, ClusterRule rule, uint32_t *__restrict__ label, unsigned long long *ctr)
{
	const uint64_t slots = tbl.slots();
	uint32_t n_live = 0, n_dead = 0;
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		uint64_t key0, val;
		uint32_t count;
		cl_load<NW>(tbl, s, key0, val);
		const bool live = cl_live(key0, val, tbl.aux[s], rule, count);
		label[s] = live ? (uint32_t)s : CL_NONE;
		n_live += live;
		n_dead += key0 != KEY_EMPTY && !live;
	}
	n_live = cl_wave_sum(n_live);
	n_dead = cl_wave_sum(n_dead);
	if ((threadIdx.x & 63) == 0) {
		if (n_live) atomicAdd(ctr + CL_N_LIVE, (unsigned long long)n_live);
		if (n_dead) atomicAdd(ctr + CL_N_DEAD, (unsigned long long)n_dead);
	}
}

__device__ inline uint32_t cl_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; x has a live node (parent[] of such a slot is never CL_NONE)
__device__ inline uint32_t cl_find(uint32_t *parent, uint32_t x)
{
	for (;;) {
		const uint32_t p = cl_ld(parent + x);
		if (p == x) return x;
		const uint32_t gp = cl_ld(parent + p);
		if (gp != p) atomicCAS(parent + x, p, gp);           // path halving
		x = p;
	}
}

template <int NW> __device__ inline void cl_union(const Table<NW> &tbl, uint32_t *parent, uint32_t a, uint32_t b)
{
	for (;;) {
		a = cl_find(parent, a);
		b = cl_find(parent, b);
		if (a == b) return;
		if (key_less<NW>(cl_key_at<NW>(tbl, a), cl_key_at<NW>(tbl, b))) { const uint32_t t = a; a = b; b = t; }    // the root with the larger key goes under
		if (atomicCAS(parent + a, a, b) == a) return;
	}
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_unite(Table<NW> tbl, int K, ClusterRule rule, uint32_t *parent, unsigned long long *ctr)
{
	const uint64_t slots = tbl.slots();
	const Key<NW> mask = cl_mask<NW>(K);
	uint32_t ends = 0;
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		uint64_t key0, val;
		uint32_t count;
		cl_load<NW>(tbl, s, key0, val);
		if (!cl_live(key0, val, tbl.aux[s], rule, count)) continue;
		const Key<NW> me = cl_key_at<NW>(tbl, s);
		for (int side = 0; side < 2; side++)
			for (uint32_t b = 0; b < 4; b++) {
				if (((val >> (24 * side + 6 * b)) & 63u) < rule.min_link) continue;
				const Key<NW> word = side == 0 ? cl_prev<NW>(me, b, K) : cl_next<NW>(me, b, mask);
				const Key<NW> bal = key_revcomp<NW>(word, K);
				uint64_t ns;
				if (!table_find<NW>(tbl, key_less<NW>(bal, word) ? bal : word, ns)) continue;
				if (cl_ld(parent + ns) == CL_NONE) continue;     // (CL_NONE never changes: the neighbour is not live)
				ends++;
				if (ns != s) cl_union<NW>(tbl, parent, (uint32_t)s, (uint32_t)ns);
			}
	}
	ends = cl_wave_sum(ends);
	if ((threadIdx.x & 63) == 0 && ends) atomicAdd(ctr + CL_N_ENDS, (unsigned long long)ends);
}

// roots[]: the slots with work[s] == s, in no particular order (cap entries; the count goes on past it)
static __global__ __launch_bounds__(TPB) void k_cl_flatten(uint32_t *parent, uint64_t slots, uint32_t *__restrict__ work, uint32_t *__restrict__ roots,
                                                           uint64_t cap, unsigned long long *ctr)
{
	const int lane = threadIdx.x & 63;
	for (uint64_t s0 = blockIdx.x * (uint64_t)TPB; s0 < slots; s0 += (uint64_t)gridDim.x * TPB) {
		const uint64_t s = s0 + threadIdx.x;
		bool root = false;
		if (s < slots) {
			uint32_t r = CL_NONE;
			if (cl_ld(parent + s) != CL_NONE) r = cl_find(parent, (uint32_t)s);
			work[s] = r;
			root = r == (uint32_t)s;
		}
		const uint64_t m = __ballot(root);
		if (!m) continue;
		unsigned long long at = 0;
		if (lane == __builtin_ctzll(m)) at = atomicAdd(ctr + CL_N_ROOTS, (unsigned long long)__popcll(m));
		at = __shfl(at, __builtin_ctzll(m)) + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
		if (root && at < cap) roots[at] = (uint32_t)s;
	}
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_sortkey(Table<NW> tbl, const uint32_t *__restrict__ roots, uint64_t n, int w, uint64_t *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) out[i] = tbl.ent[roots[i]].key[w];
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_rank(Table<NW> tbl, const uint32_t *__restrict__ roots, uint64_t n, uint32_t *__restrict__ label,
                                                 uint64_t *__restrict__ keys)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint32_t r = roots[i];
		label[r] = (uint32_t)i;
#pragma unroll
		for (int w = 0; w < NW; w++) keys[i * NW + w] = tbl.ent[r].key[w];
	}
}

// comp[id]: zeroed.  A slot that is a root keeps the label k_cl_rank gave it; every other live slot reads its root's.
template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_label(Table<NW> tbl, const uint32_t *__restrict__ work, uint32_t *label, ClusterComp *comp)
{
	const uint64_t slots = tbl.slots();
	const int lane = threadIdx.x & 63;
	for (uint64_t s0 = blockIdx.x * (uint64_t)TPB; s0 < slots; s0 += (uint64_t)gridDim.x * TPB) {
		const uint64_t s = s0 + threadIdx.x;
		uint32_t id = CL_NONE;
		unsigned long long count = 0;
		if (s < slots) {
			const uint32_t r = work[s];
			if (r != CL_NONE) {
				id = label[r];
				if (r != (uint32_t)s) label[s] = id;
				count = (unsigned long long)((uint32_t)(tbl.ent[s].val >> 48) | ((tbl.aux[s] & 0xFFFFu) << 16));
			}
		}
		uint64_t todo = __ballot(id != CL_NONE);
		while (todo) {                                       // (uniform: todo, id0 and same are the same in every lane)
			const int lead = __builtin_ctzll(todo);
			const uint32_t id0 = __shfl(id, lead);
			const uint64_t same = __ballot(id == id0);
			unsigned long long sum = id == id0 ? count : 0;
			if (same & (same - 1)) {
#pragma unroll
				for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
			}
			if (lane == lead) {
				atomicAdd(&comp[id0].nodes, (uint32_t)__popcll(same));
				atomicAdd(&comp[id0].count_sum, sum);
			}
			todo &= ~same;
		}
	}
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_cl_lookup(const uint64_t *__restrict__ keys, uint64_t n, int K, Table<NW> tbl, const uint32_t *__restrict__ label,
                                                   uint32_t *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		Key<NW> fw;
#pragma unroll
		for (int w = 0; w < NW; w++) fw.w[w] = keys[i * NW + w];
		const Key<NW> rc = key_revcomp<NW>(fw, K);
		uint64_t slot;
		out[i] = table_find<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, slot) ? label[slot] : CL_NONE;
	}
}

// unit, verdict and keep of a unit's reads from what the walk left in their records; n: the reads that are there (1 or 2)
__device__ inline uint32_t cl_decide(ReadCluster *r, int n, uint32_t pick_lo, uint32_t pick_hi, bool &keep)
{
	bool all_short = true, any_live = false;
	uint32_t unit = CL_NONE;
#pragma unroll
	for (int m = 1; m >= 0; m--) {
		if (m >= n) continue;
		all_short = all_short && r[m].kmers == 0;
		any_live = any_live || r[m].live != 0;
		if (r[m].cluster != CL_NONE) unit = r[m].cluster;    // (mate 1 is looked at last: its cluster wins)
	}
#pragma unroll
	for (int m = 0; m < 2; m++) {
		if (m >= n) continue;
		r[m].unit = unit;
		r[m].verdict = all_short ? CL_SHORT : !any_live ? CL_UNASSIGNED : r[m].live == 0 ? CL_THROUGH_MATE :
		               (r[m].split > 0 || r[m].cluster != unit) ? CL_NOT_WHOLE : CL_WHOLE;
	}
	keep = unit != CL_NONE && pick_lo <= unit && unit <= pick_hi;
	return unit;
}

// mates: 1 or 2 reads per unit (unit u = reads mates * u ..).  Read r's record goes to rec[out_base + r * out_stride].  RESOLVE:
// unit, verdict and keep (may be NULL; indexed like rec) are decided here and the kept reads counted; else unit = CL_NONE, verdict = 0.
template <int NW, bool RESOLVE>
__global__ __launch_bounds__(TPB) void k_cl_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nunits, int mates, int K,
                                                  Table<NW> tbl, const uint32_t *__restrict__ label, uint32_t pick_lo, uint32_t pick_hi,
                                                  ReadCluster *__restrict__ rec, uint64_t out_base, uint64_t out_stride, uint8_t *__restrict__ keep,
                                                  unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	uint32_t kept = 0;
	for (uint64_t u = blockIdx.x * (uint64_t)(TPB / 64) + (uint64_t)wave; u < nunits; u += (uint64_t)gridDim.x * (TPB / 64)) {
		ReadCluster rr[2] = {};
#pragma unroll
		for (int m = 0; m < 2; m++) {
			if (m >= mates) continue;                            // (uniform)
			const uint64_t r = u * (uint64_t)mates + (uint64_t)m;
			const uint64_t start = offs[r], len = offs[r + 1] - start;
			const uint64_t nk = len >= (uint64_t)K ? len - (uint64_t)K + 1 : 0;
			uint32_t first = CL_NONE, nlive = 0, nsplit = 0;
			for (uint64_t p0 = 0; p0 < nk; p0 += 64) {
				const uint64_t p = p0 + (uint64_t)lane;
				uint32_t lab = CL_NONE;
				if (p < nk) {
					const Key<NW> fw = global_kmer<NW>(words, start + p, K);
					const Key<NW> rc = key_revcomp<NW>(fw, K);
					uint64_t slot;
					if (table_find<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, slot)) lab = label[slot];
				}
				const uint64_t livem = __ballot(lab != CL_NONE);
				if (!livem) continue;
				if (first == CL_NONE) first = __shfl(lab, __builtin_ctzll(livem));
				nlive += (uint32_t)__popcll(livem);
				nsplit += (uint32_t)__popcll(__ballot(lab != CL_NONE && lab != first));
			}
			rr[m] = ReadCluster{(uint32_t)nk, nlive, nsplit, first, CL_NONE, 0};
		}
		if (lane == 0) {
			bool k = false;
			if (RESOLVE) cl_decide(rr, mates, pick_lo, pick_hi, k);
#pragma unroll
			for (int m = 0; m < 2; m++) {
				if (m >= mates) continue;
				const uint64_t at = out_base + (u * (uint64_t)mates + (uint64_t)m) * out_stride;
				rec[at] = rr[m];
				if (RESOLVE && keep) keep[at] = k ? 1 : 0;
			}
			if (RESOLVE && k) kept += (uint32_t)mates;
		}
	}
	if (RESOLVE && lane == 0 && kept) atomicAdd(n_kept, (unsigned long long)kept);
}

// one lane per unit of the ordinal-indexed records (the kept form): the stretches as k_pick_decide reads them.  A record whose
// verdict is CL_ABSENT belongs to no read: it is left as it is, and its mate is judged alone.
static __global__ __launch_bounds__(TPB) void k_cl_units(ReadCluster *__restrict__ rec, uint64_t nrec, const UnitStretch *__restrict__ segs, uint32_t nsegs,
                                                         uint64_t nunits, uint32_t pick_lo, uint32_t pick_hi, unsigned long long *n_kept)
{
	uint32_t mine = 0;
	for (uint64_t u0 = blockIdx.x * (uint64_t)TPB; u0 < nunits; u0 += (uint64_t)gridDim.x * TPB) {
		const uint64_t u = u0 + threadIdx.x;
		if (u >= nunits) continue;
		uint32_t lo = 0, hi = nsegs;                                     // the last stretch that starts at or before u
		while (hi - lo > 1) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (segs[mid].unit0 <= u) lo = mid; else hi = mid;
		}
		const UnitStretch sg = segs[lo];
		const uint64_t a0 = sg.ord0 + (u - sg.unit0) * sg.stride;
		ReadCluster rr[2] = {};
		uint64_t at[2] = {0, 0};
		int n = 0;
		for (uint64_t m = 0; m < (sg.stride == 2 ? 2u : 1u); m++) {
			if (a0 + m >= nrec) continue;
			const ReadCluster r = rec[a0 + m];
			if (r.verdict == CL_ABSENT) continue;
			rr[n] = r;
			at[n++] = a0 + m;
		}
		if (!n) continue;
		bool k;
		cl_decide(rr, n, pick_lo, pick_hi, k);
		for (int m = 0; m < n; m++) rec[at[m]] = rr[m];
		if (k) mine += (uint32_t)n;
	}
	mine = cl_wave_sum(mine);
	if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
