// sdt_unitig_kernels.cuh -- the unitigs of the counted node table (the rule: include/sdt_gpu.h): the maximal chains of oriented k-mers
// in which every word has its neighbour as only successor and is that neighbour's only predecessor, and the links between them.
// Nothing here writes ent or aux.  Liveness, the oriented words, the probe and the successors are those of the bubbles (bb_probe,
// bb_succ, bb_link of sdt_bubble_kernels.cuh); what is new is the JOIN, a successor test in both directions.
//   ug_join<NW>      : JOIN(x, y) for the only successor y of x.  One probe per qualifying out counter of x (one in a linear stretch; it
//                      brings y's link word and count along), and for the way back none for x itself, which is live: only a second
//                      qualifying in counter of y is probed.
//   k_ug_starts<NW>  : one lane per slot, grid-stride.  A live node tests for both of its oriented words whether the word has a left
//                      join (= its reverse complement has a right join); a side with no qualifying counter costs no probe.  A word
//                      without one is the first word of a chain: (slot << 1 | orientation) goes to a list in chunks (sdt_append.cuh).
//   k_ug_walk<NW>    : ONE LANE PER START, all state in registers: x and revcomp(x) side by side, nodes, min, max, sum.  A chain is
//                      walked from both of its ends; the lane with x0 <= revcomp(last) gives the record.  Records go out dense: one
//                      ballot and one atomic per wavefront.  A wavefront waits for its longest chain.
//   k_ug_mark<NW>    : (only when the chains do not cover the live nodes) one lane per record: the chain again, a bit per slot.
//   k_ug_cycles<NW>  : (the same) one lane per slot: a live slot without its bit lies on a cycle; it walks the cycle from its stored key,
//                      gives up at the first smaller canonical key and gives the record when it is back at itself -- quadratic in the
//                      length of one cycle in the worst case.
//   k_ug_sortkey, k_ug_permute, k_ug_rlast, k_ug_gather : the list sorted by x0, and a second order by revcomp(last): the two arrays
//                      in which k_ug_links finds the unitig that a word begins.
//   k_ug_links<NW>   : one lane per (unitig, orientation) of the range: the successors of its out word, each searched in the two
//                      orders.  Run twice: the counts, then (offsets from the host) the records.
//   k_ug_seqs<NW>    : one lane per unitig of the range: the K bases of x0, then the chain again, a byte per step at its offset.
#pragma once
#include "sdt_bubble_kernels.cuh"

namespace sdt {

struct Unitig {                                          // == sdt_unitig of include/sdt_gpu.h
	unsigned long long sum;
	uint32_t nodes, min, max, info;
};
static_assert(sizeof(Unitig) == 24, "sdt_unitig is 24 bytes");

struct UnitigLink {                                      // == sdt_unitig_link
	uint32_t from, to, info, reserved;
};

// counters of unitigs_begin
constexpr int UG_N_LIVE = 0, UG_N_STARTS = 1, UG_N_REC = 2, UG_N_CIRC = 3, UG_NODES = 4, UG_SEQ_BYTES = 5, UG_LONGEST = 6, UG_BROKEN = 7, UG_TOO_LONG = 8,
              UG_COUNTERS = 10;
constexpr int UG_REC_WORDS = 3;                          // a raw record: x0, last (NW words each), then the 24 bytes of Unitig

// JOIN(x, y) for the only successor y of the live word x (rx, val: its reverse complement, its node's link word and count); deg = |succ(x)|
// either way; y, ry, yval, ycount, yb as bb_succ sets them
template <int NW>
__device__ inline bool ug_join(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, uint64_t val, int K, const Key<NW> &mask, const ClusterRule &rule, Key<NW> &y,
                               Key<NW> &ry, uint64_t &yval, uint32_t &ycount, uint32_t &yb, uint32_t &deg)
{
	deg = bb_succ<NW>(tbl, x, rx, val, K, mask, rule, BB_NO_BASE, y, ry, yval, ycount, yb);
	if (deg != 1) return false;
	if (key_eq<NW>(x, rx) || key_eq<NW>(y, ry) || key_eq<NW>(y, x) || key_eq<NW>(y, rx)) return false;      // a palindrome; the same node
	// succ(revcomp(y)) must be revcomp(x) alone: its counter towards the low base of rx qualifies (x is live: no probe), no other does
	const uint32_t back = (uint32_t)rx.w[NW - 1] & 3u;
	if (bb_link(yval, !key_less<NW>(y, ry), back) < rule.min_link) return false;
	return bb_degree<NW>(tbl, ry, y, yval, K, mask, rule, back) == 1;
}

__device__ inline unsigned long long ug_wave_sum64(unsigned long long v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// the raw record of every lane with emit set, dense: one ballot and one atomic per wavefront; every lane of the wavefront calls it
template <int NW>
__device__ inline void ug_emit(bool emit, const Key<NW> &x0, const Key<NW> &last, const Unitig &r, uint64_t *__restrict__ raw, unsigned long long cap,
                               unsigned long long *ctr)
{
	constexpr int STRIDE = 2 * NW + UG_REC_WORDS;
	const int lane = threadIdx.x & 63;
	const unsigned long long m = __ballot(emit);
	if (!m) return;                                          // (uniform)
	const int lead = __builtin_ctzll(m);
	unsigned long long at = 0;
	if (lane == lead) at = atomicAdd(ctr + UG_N_REC, (unsigned long long)__popcll(m));
	at = __shfl(at, lead) + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
	if (!emit || at >= cap) return;
	uint64_t *o = raw + at * STRIDE;
#pragma unroll
	for (int w = 0; w < NW; w++) { o[w] = x0.w[w]; o[NW + w] = last.w[w]; }
	*reinterpret_cast<Unitig *>(o + 2 * NW) = r;
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_starts(Table<NW> tbl, int K, ClusterRule rule, unsigned long long *__restrict__ list, ApOut ap, unsigned long long *ctr)
{
	__shared__ WaveApp s_app[TPB / 64];
	ap_init(s_app);
	const uint64_t slots = tbl.slots();
	const Key<NW> mask = cl_mask<NW>(K);
	uint32_t n_live = 0, n_starts = 0;
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		uint64_t key0, val;
		uint32_t count;
		cl_load<NW>(tbl, s, key0, val);
		if (!cl_live(key0, val, tbl.aux[s], rule, count)) continue;
		n_live++;
		const Key<NW> me = cl_key_at<NW>(tbl, s), rme = key_revcomp<NW>(me, K);
		Key<NW> y, ry;
		uint64_t yval;
		uint32_t ycount, yb, deg;
		// me has a left join iff rme has a right one, and the other way round
		if (!ug_join<NW>(tbl, rme, me, val, K, mask, rule, y, ry, yval, ycount, yb, deg)) {
			n_starts++;
			const unsigned long long r = ap_append(s_app, ap);
			if (r != AP_NONE) list[r] = s << 1;
		}
		if (!key_eq<NW>(me, rme) && !ug_join<NW>(tbl, me, rme, val, K, mask, rule, y, ry, yval, ycount, yb, deg)) {
			n_starts++;
			const unsigned long long r = ap_append(s_app, ap);
			if (r != AP_NONE) list[r] = s << 1 | 1ULL;
		}
	}
	ap_finish_mark(s_app, ap);
	n_live = cl_wave_sum(n_live);
	n_starts = cl_wave_sum(n_starts);
	if ((threadIdx.x & 63) == 0) {
		if (n_live) atomicAdd(ctr + UG_N_LIVE, (unsigned long long)n_live);
		if (n_starts) atomicAdd(ctr + UG_N_STARTS, (unsigned long long)n_starts);
	}
}

// the chain from the live word cur on (rcur, val, count: its reverse complement and its node) along the right joins; cur / rcur end as its
// last word, outdeg as its out-degree.  false: 2^32 nodes
template <int NW>
__device__ inline bool ug_chain(const Table<NW> &tbl, int K, const Key<NW> &mask, const ClusterRule &rule, Key<NW> &cur, Key<NW> &rcur, uint64_t val, uint32_t count,
                                Unitig &r, uint32_t &outdeg)
{
	r.sum = count;
	r.nodes = 1;
	r.min = r.max = count;
	for (;;) {
		Key<NW> y, ry;
		uint64_t yval;
		uint32_t ycount, yb;
		if (!ug_join<NW>(tbl, cur, rcur, val, K, mask, rule, y, ry, yval, ycount, yb, outdeg)) return true;
		if (r.nodes == 0xFFFFFFFFu) return false;
		r.nodes++;
		r.sum += ycount;
		r.min = ycount < r.min ? ycount : r.min;
		r.max = ycount > r.max ? ycount : r.max;
		cur = y; rcur = ry; val = yval;
	}
}

// list: n_list entries (slot << 1 | orientation, or AP_NONE).  raw: cap records of 2 NW + UG_REC_WORDS words; ctr[UG_N_REC] counts on past cap
template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_walk(Table<NW> tbl, int K, ClusterRule rule, const unsigned long long *__restrict__ list, unsigned long long n_list,
                                                 uint64_t *__restrict__ raw, unsigned long long cap, unsigned long long *ctr)
{
	const Key<NW> mask = cl_mask<NW>(K);
	unsigned long long nodes = 0;
	for (unsigned long long e0 = blockIdx.x * (unsigned long long)TPB; e0 < n_list; e0 += (unsigned long long)gridDim.x * TPB) {      // (uniform)
		const unsigned long long e = e0 + threadIdx.x;
		const unsigned long long f = e < n_list ? list[e] : AP_NONE;
		Key<NW> x0 = {}, cur = {};
		Unitig r = {};
		bool emit = false;
		if (f != AP_NONE) {
			const uint64_t slot = f >> 1;
			const Key<NW> me = cl_key_at<NW>(tbl, slot), rme = key_revcomp<NW>(me, K);
			const uint64_t val = tbl.ent[slot].val;
			const uint32_t count = (uint32_t)(val >> 48) | ((tbl.aux[slot] & 0xFFFFu) << 16);
			const bool fwd = !(f & 1ULL);
			x0 = fwd ? me : rme;
			cur = x0;
			Key<NW> rcur = fwd ? rme : me;
			const uint32_t indeg = bb_degree<NW>(tbl, rcur, cur, val, K, mask, rule);
			uint32_t outdeg = 0;
			if (!ug_chain<NW>(tbl, K, mask, rule, cur, rcur, val, count, r, outdeg)) atomicAdd(ctr + UG_TOO_LONG, 1ULL);
			r.info = indeg << 4 | outdeg << 8;
			emit = !key_less<NW>(rcur, x0);                  // x0 <= revcomp(last)
			if (emit) nodes += r.nodes;
		}
		ug_emit<NW>(emit, x0, cur, r, raw, cap, ctr);
	}
	nodes = ug_wave_sum64(nodes);
	if ((threadIdx.x & 63) == 0 && nodes) atomicAdd(ctr + UG_NODES, nodes);
}

// the nodes of the n raw records, a bit per slot (bits: (slots + 31) / 32 words, cleared)
template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_mark(Table<NW> tbl, int K, ClusterRule rule, const uint64_t *__restrict__ raw, uint64_t n, uint32_t *bits, unsigned long long *ctr)
{
	constexpr int STRIDE = 2 * NW + UG_REC_WORDS;
	const Key<NW> mask = cl_mask<NW>(K);
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *rw = raw + i * STRIDE;
		const uint32_t nodes = reinterpret_cast<const Unitig *>(rw + 2 * NW)->nodes;
		Key<NW> cur;
#pragma unroll
		for (int w = 0; w < NW; w++) cur.w[w] = rw[w];
		Key<NW> rcur = key_revcomp<NW>(cur, K);
		uint64_t val = 0;
		uint32_t count;
		bool ok = bb_probe<NW>(tbl, cur, rcur, rule, val, count);
		for (uint32_t k = 0; ok && k < nodes; k++) {
			uint64_t slot;
			ok = table_find<NW>(tbl, key_less<NW>(rcur, cur) ? rcur : cur, slot);
			if (!ok) break;
			atomicOr(bits + (slot >> 5), 1u << (slot & 31u));
			if (k + 1 == nodes) break;
			Key<NW> y, ry;
			uint64_t yval;
			uint32_t ycount, yb;
			ok = bb_succ<NW>(tbl, cur, rcur, val, K, mask, rule, BB_NO_BASE, y, ry, yval, ycount, yb) == 1;
			cur = y; rcur = ry; val = yval;
		}
		if (!ok) atomicAdd(ctr + UG_BROKEN, 1ULL);
	}
}

// a live slot whose bit is clear lies on a cycle: the record from the slot that holds the cycle's smallest canonical key
template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_cycles(Table<NW> tbl, int K, ClusterRule rule, const uint32_t *__restrict__ bits, uint64_t *__restrict__ raw,
                                                   unsigned long long cap, unsigned long long *ctr)
{
	const uint64_t slots = tbl.slots();
	const Key<NW> mask = cl_mask<NW>(K);
	unsigned long long nodes = 0;
	uint32_t n_circ = 0;
	for (uint64_t s0 = blockIdx.x * (uint64_t)TPB; s0 < slots; s0 += (uint64_t)gridDim.x * TPB) {      // (uniform)
		const uint64_t s = s0 + threadIdx.x;
		Key<NW> me = {}, cur = {};
		Unitig r = {};
		bool emit = false;
		uint64_t key0 = KEY_EMPTY, val = 0;
		uint32_t count = 0;
		if (s < slots) cl_load<NW>(tbl, s, key0, val);
		if (s < slots && cl_live(key0, val, tbl.aux[s], rule, count) && !(bits[s >> 5] >> (s & 31u) & 1u)) {
			me = cl_key_at<NW>(tbl, s);
			cur = me;
			Key<NW> rcur = key_revcomp<NW>(me, K);
			r.sum = count;
			r.nodes = 1;
			r.min = r.max = count;
			r.info = 1u | 1u << 4 | 1u << 8;                 // circular: every word has both joins
			for (;;) {
				Key<NW> y, ry;
				uint64_t yval;
				uint32_t ycount, yb, deg;
				if (!ug_join<NW>(tbl, cur, rcur, val, K, mask, rule, y, ry, yval, ycount, yb, deg)) { atomicAdd(ctr + UG_BROKEN, 1ULL); break; }
				if (key_eq<NW>(y, me)) { emit = true; break; }
				if (key_less<NW>(y, me) || key_less<NW>(ry, me)) break;      // a smaller canonical key: its slot reports the cycle
				if (r.nodes == 0xFFFFFFFFu) { atomicAdd(ctr + UG_TOO_LONG, 1ULL); break; }
				r.nodes++;
				r.sum += ycount;
				r.min = ycount < r.min ? ycount : r.min;
				r.max = ycount > r.max ? ycount : r.max;
				cur = y; rcur = ry; val = yval;
			}
			if (emit) { nodes += r.nodes; n_circ++; }
		}
		ug_emit<NW>(emit, me, cur, r, raw, cap, ctr);
	}
	nodes = ug_wave_sum64(nodes);
	n_circ = cl_wave_sum(n_circ);
	if ((threadIdx.x & 63) == 0 && n_circ) {
		atomicAdd(ctr + UG_NODES, nodes);
		atomicAdd(ctr + UG_N_CIRC, (unsigned long long)n_circ);
	}
}

// word w of record order[i] of src (records of `stride` words)
static __global__ __launch_bounds__(TPB) void k_ug_sortkey(const uint64_t *__restrict__ src, int stride, const uint32_t *__restrict__ order, uint64_t n, int w,
                                                           uint64_t *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) out[i] = src[(uint64_t)order[i] * stride + w];
}

// record i of the sorted list from the raw one; sums the sequence bytes and takes the longest unitig, per wavefront
static __global__ __launch_bounds__(TPB) void k_ug_permute(const uint64_t *__restrict__ raw, int stride, int nw, int K, const uint32_t *__restrict__ order, uint64_t n,
                                                           uint64_t *__restrict__ keys, Unitig *__restrict__ rec, unsigned long long *ctr)
{
	unsigned long long bytes = 0;
	uint32_t longest = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *r = raw + (uint64_t)order[i] * stride;
		for (int w = 0; w < 2 * nw; w++) keys[i * 2 * nw + w] = r[w];
		const Unitig u = *reinterpret_cast<const Unitig *>(r + 2 * nw);
		rec[i] = u;
		bytes += (unsigned long long)u.nodes + (unsigned long long)(K - 1);
		longest = u.nodes > longest ? u.nodes : longest;
	}
	bytes = ug_wave_sum64(bytes);
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		const uint32_t o = __shfl_xor(longest, d);
		longest = o > longest ? o : longest;
	}
	if ((threadIdx.x & 63) == 0 && bytes) {
		atomicAdd(ctr + UG_SEQ_BYTES, bytes);
		atomicMax(ctr + UG_LONGEST, (unsigned long long)longest);
	}
}

// revcomp(last) of every unitig of the sorted list: the word with which the unitig begins when it is read backwards
template <int NW> __global__ __launch_bounds__(TPB) void k_ug_rlast(const uint64_t *__restrict__ keys, uint64_t n, int K, uint64_t *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		Key<NW> last;
#pragma unroll
		for (int w = 0; w < NW; w++) last.w[w] = keys[(i * 2 + 1) * NW + w];
		const Key<NW> r = key_revcomp<NW>(last, K);
#pragma unroll
		for (int w = 0; w < NW; w++) out[i * NW + w] = r.w[w];
	}
}

// the second order: entry j holds revcomp(last) of unitig order[j], and that id
static __global__ __launch_bounds__(TPB) void k_ug_gather(const uint64_t *__restrict__ src, int nw, const uint32_t *__restrict__ order, uint64_t n,
                                                          uint64_t *__restrict__ idx_keys, uint32_t *__restrict__ idx_id)
{
	for (uint64_t j = blockIdx.x * (uint64_t)TPB + threadIdx.x; j < n; j += (uint64_t)gridDim.x * TPB) {
		const uint32_t i = order[j];
		for (int w = 0; w < nw; w++) idx_keys[j * nw + w] = src[(uint64_t)i * nw + w];
		idx_id[j] = i;
	}
}

// the position of y among n ascending words that lie `stride` words apart, or n
template <int NW> __device__ inline uint64_t ug_search(const uint64_t *__restrict__ words, int stride, uint64_t n, const Key<NW> &y)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		Key<NW> k;
#pragma unroll
		for (int w = 0; w < NW; w++) k.w[w] = words[mid * stride + w];
		if (key_less<NW>(k, y)) lo = mid + 1; else hi = mid;
	}
	if (lo == n) return n;
	bool same = true;
#pragma unroll
	for (int w = 0; w < NW; w++) same = same && words[lo * stride + w] == y.w[w];
	return same ? lo : n;
}

// entry j of the range: unitig first + (j >> 1), orientation j & 1.  links == nullptr: counts[j] = its links, *dangling grows by the
// successors of its out word that begin no unitig; else its records go to links[offs[j] ..]
template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_links(Table<NW> tbl, int K, ClusterRule rule, const uint64_t *__restrict__ keys, uint64_t n_all,
                                                  const uint64_t *__restrict__ idx_keys, const uint32_t *__restrict__ idx_id, uint64_t first, uint64_t n,
                                                  uint32_t *__restrict__ counts, const uint64_t *__restrict__ offs, UnitigLink *__restrict__ links, unsigned long long *ctr)
{
	const Key<NW> mask = cl_mask<NW>(K);
	for (uint64_t j = blockIdx.x * (uint64_t)TPB + threadIdx.x; j < 2 * n; j += (uint64_t)gridDim.x * TPB) {
		const uint64_t u = first + (j >> 1);
		const uint32_t o = (uint32_t)(j & 1);
		Key<NW> k;
#pragma unroll
		for (int w = 0; w < NW; w++) k.w[w] = keys[(u * 2 + (o ? 0 : 1)) * NW + w];      // (+): last; (-): revcomp(x0)
		const Key<NW> rk = key_revcomp<NW>(k, K);
		const Key<NW> x = o ? rk : k, rx = o ? k : rk;
		uint64_t val;
		uint32_t count, found = 0, dangling = 0;
		if (!bb_probe<NW>(tbl, x, rx, rule, val, count)) { atomicAdd(ctr + 1, 1ULL); continue; }
		const bool fwd = !key_less<NW>(rx, x);
		for (uint32_t b = 0; b < 4; b++) {
			const uint32_t link = bb_link(val, fwd, b);
			if (link < rule.min_link) continue;
			const Key<NW> y = cl_next<NW>(x, b, mask), ry = cl_prev<NW>(rx, b ^ 2u, K);
			uint64_t yval;
			uint32_t ycount;
			if (!bb_probe<NW>(tbl, y, ry, rule, yval, ycount)) continue;
			uint32_t o2 = 0;
			uint64_t v = ug_search<NW>(keys, 2 * NW, n_all, y);
			if (v == n_all) {
				const uint64_t at = ug_search<NW>(idx_keys, NW, n_all, y);
				if (at == n_all) { dangling++; continue; }
				v = idx_id[at];
				o2 = 1;
			}
			if (links) links[offs[j] + found] = UnitigLink{(uint32_t)u, (uint32_t)v, o | o2 << 1 | b << 2 | link << 8, 0u};
			found++;
		}
		if (!links) {
			counts[j] = found;
			if (dangling) atomicAdd(ctr, (unsigned long long)dangling);
		}
	}
}

// unitig first + i of the range: nodes + K - 1 bytes at bases[offs[i] ..].  A chain that does not walk as it did at begin counts in *bad
template <int NW>
__global__ __launch_bounds__(TPB) void k_ug_seqs(Table<NW> tbl, int K, ClusterRule rule, const uint64_t *__restrict__ keys, const Unitig *__restrict__ rec, uint64_t first,
                                                 uint64_t n, const uint64_t *__restrict__ offs, uint8_t *__restrict__ bases, unsigned long long *bad)
{
	const Key<NW> mask = cl_mask<NW>(K);
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *kw = keys + (first + i) * 2 * NW;
		const uint32_t nodes = rec[first + i].nodes;
		uint8_t *o = bases + offs[i];
		for (int j = 0; j < K; j++) {
			const int bit = 2 * (K - 1 - j);
			o[j] = (uint8_t)(kw[NW - 1 - (bit >> 6)] >> (bit & 63) & 3u);
		}
		Key<NW> cur, last;
#pragma unroll
		for (int w = 0; w < NW; w++) { cur.w[w] = kw[w]; last.w[w] = kw[NW + w]; }
		Key<NW> rcur = key_revcomp<NW>(cur, K);
		uint64_t val;
		uint32_t count;
		bool ok = bb_probe<NW>(tbl, cur, rcur, rule, val, count);
		for (uint32_t k = 1; ok && k < nodes; k++) {
			Key<NW> y, ry;
			uint64_t yval;
			uint32_t ycount, yb;
			ok = bb_succ<NW>(tbl, cur, rcur, val, K, mask, rule, BB_NO_BASE, y, ry, yval, ycount, yb) == 1;
			if (!ok) break;
			o[K - 1 + k] = (uint8_t)yb;
			cur = y; rcur = ry; val = yval;
		}
		if (!ok || !key_eq<NW>(cur, last)) atomicAdd(bad, 1ULL);
	}
}

} // namespace sdt
