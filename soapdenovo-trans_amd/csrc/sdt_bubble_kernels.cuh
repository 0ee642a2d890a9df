// sdt_bubble_kernels.cuh -- the bubbles of the counted node table (the rule: include/sdt_gpu.h): two non-branching paths that leave one
// oriented k-mer and meet again.  Nothing here writes ent or aux.  Liveness and the neighbour words are those of the clustering
// (cl_live, cl_prev, cl_next of sdt_cluster_kernels.cuh); what is new is the ORIENTED word: a walk carries x and its reverse complement
// rx side by side -- next(x, b) has the reverse complement prev(rx, b ^ 2), one shift, never a revcomp from scratch -- and reads the
// out side of x from the node's link word: the right counters when x is the stored key, the left ones with the base complemented when not.
//   k_bb_forks<NW>   : one lane per slot, grid-stride.  A live node counts the successors of both orientations (a palindrome has one)
//                      from the 16 bytes it loaded and one liveness probe per counter that qualifies -- on a side where two or more
//                      do: the others are no fork, and nearly every node leaves without a probe; (slot << 1 | orientation) of a
//                      side with two successors or more goes to a list in chunks (sdt_append.cuh, holes marked AP_NONE).  Live nodes and
//                      fork sides: one atomic per wavefront.
//   bb_branch<NW>    : the branch of the rule from its first word: sink, len, min, sum.  Per step the in-degree of cur (one probe per
//                      qualifying in-counter, but none for the counter that names the node the walk came from: that one is live) and
//                      its successors (one per out-counter; the probe of the only successor brings that node's link word and count
//                      along, so the next step starts with them): one probe per node of a linear stretch, and a probe is one trip to
//                      memory when the key sits in its home slot (bb_probe).  All state is in registers.
//   k_bb_walk<NW>    : ONE LANE PER FORK, its branches in turn, 64 forks per wavefront; the up to four sinks are compared in the lane and
//                      a pair that reached the same word with s <= revcomp(t) is a record.  Records go out dense: one ballot and one
//                      atomic per wavefront and pair -- the walks are few, their cursor is not hot.  (Four adjacent lanes per fork,
//                      one per base, the sinks compared by __shfl, was built first and measured: 21.4 ms against 14.1 ms for the same
//                      412 290 branches.  A fork mostly has two branches, so half of its lanes idle, and the wavefront waits for its
//                      longest branch either way -- profiles/bubbles/.)
//   k_bb_sortkey     : one word of the sort key of the records in their current order: the two bases, or word w of s.
//   k_bb_permute     : record i of the sorted list from the raw one; sums the path bytes and takes the longest branch, per wavefront.
//   k_bb_paths<NW>   : one lane per branch of the requested bubbles: the same steps again, a byte per step at the branch's offset.
#pragma once
#include "sdt_cluster_kernels.cuh"
#include "sdt_append.cuh"

namespace sdt {

struct Bubble {                                          // == sdt_bubble of include/sdt_gpu.h
	unsigned long long sum_a, sum_b;
	uint32_t len_a, len_b, min_a, min_b, src_count, snk_count, info, reserved;
};
static_assert(sizeof(Bubble) == 48, "sdt_bubble is 48 bytes");

struct BubbleRule {                                      // live: min_count already max(min_count, 1)
	ClusterRule live;
	uint32_t max_len;
};

// counters of bubbles_begin
constexpr int BB_N_LIVE = 0, BB_N_FORKS = 1, BB_N_BRANCHES = 2, BB_N_REACHED = 3, BB_N_REC = 4, BB_PATH_BYTES = 5, BB_LONGEST = 6, BB_COUNTERS = 8;
constexpr int BB_REC_WORDS = 6;                          // a raw record: s, t (NW words each), then the 48 bytes of Bubble

// the link counter of the oriented word x towards base b; fwd: x is its node's stored key; val: that node's link word and count
__device__ inline uint32_t bb_link(uint64_t val, bool fwd, uint32_t b) { return (uint32_t)(val >> (fwd ? 24u + 6u * b : 6u * (b ^ 2u))) & 63u; }

// the node of the oriented word x (rx: its reverse complement): live, with its link word and count
// (table_find with the aux word of every slot it looks at loaded beside the entry, not after the key matched: a step of a walk is a
// chain of dependent probes, and this makes a probe one trip to memory where the key sits in its home slot, not two)
template <int NW> __device__ inline bool bb_probe(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, const ClusterRule &rule, uint64_t &val, uint32_t &count)
{
	const Key<NW> key = key_less<NW>(rx, x) ? rx : x;
	uint64_t slot, lo, n;
	probe_begin<NW>(tbl, key, slot, lo, n);
	for (uint64_t probe = 0; probe < n; probe++, slot = probe_next(slot, lo, n)) {
		const Entry<NW> *e = tbl.ent + slot;
		const uint32_t aux = tbl.aux[slot];
		if (e->key[0] == KEY_EMPTY) return false;
		bool same = true;
#pragma unroll
		for (int w = 0; w < NW; w++) same = same && e->key[w] == key.w[w];
		if (!same) continue;
		val = e->val;
		return cl_live(0, val, aux, rule, count);
	}
	return false;
}

constexpr uint32_t BB_NO_BASE = 4;

// |succ(x)|; the LAST successor in y, ry, yval, ycount, yb (the only one when the degree is 1).  known: a base whose successor is known
// to be live and is not probed (the caller does not read y and the rest then), or BB_NO_BASE
template <int NW>
__device__ inline uint32_t bb_succ(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, uint64_t val, int K, const Key<NW> &mask, const ClusterRule &rule,
                                   uint32_t known, Key<NW> &y, Key<NW> &ry, uint64_t &yval, uint32_t &ycount, uint32_t &yb)
{
	const bool fwd = !key_less<NW>(rx, x);
	uint32_t deg = 0;
	for (uint32_t b = 0; b < 4; b++) {
		if (bb_link(val, fwd, b) < rule.min_link) continue;
		if (b == known) { deg++; continue; }
		const Key<NW> n = cl_next<NW>(x, b, mask), rn = cl_prev<NW>(rx, b ^ 2u, K);
		uint64_t nval;
		uint32_t ncount;
		if (!bb_probe<NW>(tbl, n, rn, rule, nval, ncount)) continue;
		deg++;
		y = n; ry = rn; yval = nval; ycount = ncount; yb = b;
	}
	return deg;
}

template <int NW>
__device__ inline uint32_t bb_degree(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, uint64_t val, int K, const Key<NW> &mask, const ClusterRule &rule,
                                     uint32_t known = BB_NO_BASE)
{
	Key<NW> y, ry;
	uint64_t yval;
	uint32_t ycount, yb;
	return bb_succ<NW>(tbl, x, rx, val, K, mask, rule, known, y, ry, yval, ycount, yb);
}

// the branch that starts at the live word cur (rcur, val, count: its reverse complement and its node).  true: it reached the sink, which
// is then cur / rcur / count.  mn is ~0 while the branch has no inner node.  back: the base by which revcomp(cur) leads back to where
// the walk came from -- the low base of that word's reverse complement.  That node is live (it is s, or an inner node), so the
// in-degree of cur needs no probe for it: a node of a linear stretch costs ONE probe, its successor's, not two.
template <int NW>
__device__ inline bool bb_branch(const Table<NW> &tbl, int K, const Key<NW> &mask, const BubbleRule &rule, Key<NW> &cur, Key<NW> &rcur, uint64_t val, uint32_t &count,
                                 uint32_t back, uint32_t &len, uint32_t &mn, unsigned long long &sum)
{
	len = 0;
	mn = 0xFFFFFFFFu;
	sum = 0;
	for (;;) {
		if (bb_degree<NW>(tbl, rcur, cur, val, K, mask, rule.live, back) >= 2) return true;
		Key<NW> y, ry;
		uint64_t yval;
		uint32_t ycount, yb;
		if (bb_succ<NW>(tbl, cur, rcur, val, K, mask, rule.live, BB_NO_BASE, y, ry, yval, ycount, yb) != 1 || len == rule.max_len) return false;
		len++;
		mn = count < mn ? count : mn;
		sum += count;
		back = (uint32_t)rcur.w[NW - 1] & 3u;
		cur = y; rcur = ry; val = yval; count = ycount;
	}
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_bb_forks(Table<NW> tbl, int K, BubbleRule rule, unsigned long long *__restrict__ list, ApOut ap, unsigned long long *ctr)
{
	__shared__ WaveApp s_app[TPB / 64];
	ap_init(s_app);
	const uint64_t slots = tbl.slots();
	const Key<NW> mask = cl_mask<NW>(K);
	uint32_t n_live = 0, n_forks = 0;
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		uint64_t key0, val;
		uint32_t count;
		cl_load<NW>(tbl, s, key0, val);
		if (!cl_live(key0, val, tbl.aux[s], rule.live, count)) continue;
		n_live++;
		// (a side with fewer than two counters that qualify is no fork whatever its neighbours are: nearly every node leaves here
		// without a probe, and the scan is the stream of the table)
		uint32_t q_right = 0, q_left = 0;
#pragma unroll
		for (uint32_t b = 0; b < 4; b++) {
			q_right += bb_link(val, true, b) >= rule.live.min_link;
			q_left += bb_link(val, false, b) >= rule.live.min_link;
		}
		if (q_right < 2 && q_left < 2) continue;
		const Key<NW> me = cl_key_at<NW>(tbl, s), rme = key_revcomp<NW>(me, K);
		if (q_right >= 2 && bb_degree<NW>(tbl, me, rme, val, K, mask, rule.live) >= 2) {
			n_forks++;
			const unsigned long long r = ap_append(s_app, ap);
			if (r != AP_NONE) list[r] = s << 1;
		}
		if (q_left >= 2 && !key_eq<NW>(me, rme) && bb_degree<NW>(tbl, rme, me, val, K, mask, rule.live) >= 2) {
			n_forks++;
			const unsigned long long r = ap_append(s_app, ap);
			if (r != AP_NONE) list[r] = s << 1 | 1ULL;
		}
	}
	ap_finish_mark(s_app, ap);
	n_live = cl_wave_sum(n_live);
	n_forks = cl_wave_sum(n_forks);
	if ((threadIdx.x & 63) == 0) {
		if (n_live) atomicAdd(ctr + BB_N_LIVE, (unsigned long long)n_live);
		if (n_forks) atomicAdd(ctr + BB_N_FORKS, (unsigned long long)n_forks);
	}
}

// list: n_list entries (slot << 1 | orientation, or AP_NONE).  raw: cap records of 2 NW + BB_REC_WORDS words; ctr[BB_N_REC] counts on past cap.
// (t, rt, link ... are indexed by unrolled constants only: registers, not scratch)
template <int NW>
__global__ __launch_bounds__(TPB) void k_bb_walk(Table<NW> tbl, int K, BubbleRule rule, const unsigned long long *__restrict__ list, unsigned long long n_list,
                                                 uint64_t *__restrict__ raw, unsigned long long cap, unsigned long long *ctr)
{
	constexpr int STRIDE = 2 * NW + BB_REC_WORDS;
	const int lane = threadIdx.x & 63;
	const Key<NW> mask = cl_mask<NW>(K);
	uint32_t n_branches = 0, n_reached = 0;
	for (unsigned long long e0 = blockIdx.x * (unsigned long long)TPB; e0 < n_list; e0 += (unsigned long long)gridDim.x * TPB) {      // (uniform)
		const unsigned long long e = e0 + threadIdx.x;
		const unsigned long long f = e < n_list ? list[e] : AP_NONE;
		Key<NW> s = {}, t[4] = {}, rt[4] = {};
		uint32_t link[4] = {}, count[4] = {}, len[4] = {}, mn[4] = {}, src_count = 0;
		unsigned long long sum[4] = {};
		bool reached[4] = {};
		if (f != AP_NONE) {
			const uint64_t slot = f >> 1;
			const Key<NW> me = cl_key_at<NW>(tbl, slot), rme = key_revcomp<NW>(me, K);
			const uint64_t sval = tbl.ent[slot].val;
			const bool fwd = !(f & 1ULL);
			src_count = (uint32_t)(sval >> 48) | ((tbl.aux[slot] & 0xFFFFu) << 16);
			s = fwd ? me : rme;
			const Key<NW> rs = fwd ? rme : me;
#pragma unroll
			for (uint32_t b = 0; b < 4; b++) {
				link[b] = bb_link(sval, fwd, b);
				if (link[b] < rule.live.min_link) continue;
				uint64_t val;
				t[b] = cl_next<NW>(s, b, mask);
				rt[b] = cl_prev<NW>(rs, b ^ 2u, K);
				if (bb_probe<NW>(tbl, t[b], rt[b], rule.live, val, count[b])) {
					n_branches++;
					reached[b] = bb_branch<NW>(tbl, K, mask, rule, t[b], rt[b], val, count[b], (uint32_t)rs.w[NW - 1] & 3u, len[b], mn[b], sum[b]);
					n_reached += reached[b];
				}
			}
		}
		// the six pairs; every lane takes part in the ballots
#pragma unroll
		for (uint32_t a = 0; a < 3; a++)
#pragma unroll
			for (uint32_t b = a + 1; b < 4; b++) {
				const bool emit = reached[a] && reached[b] && key_eq<NW>(t[a], t[b]) && !key_less<NW>(rt[b], s);      // s <= revcomp(t)
				const unsigned long long m = __ballot(emit);
				if (!m) continue;                                // (uniform)
				const int lead = __builtin_ctzll(m);
				unsigned long long at = 0;
				if (lane == lead) at = atomicAdd(ctr + BB_N_REC, (unsigned long long)__popcll(m));
				at = __shfl(at, lead) + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
				if (!emit || at >= cap) continue;
				uint64_t *o = raw + at * STRIDE;
#pragma unroll
				for (int w = 0; w < NW; w++) { o[w] = s.w[w]; o[NW + w] = t[b].w[w]; }
				Bubble r;
				r.sum_a = sum[a]; r.sum_b = sum[b];
				r.len_a = len[a]; r.len_b = len[b];
				r.min_a = len[a] ? mn[a] : 0u; r.min_b = len[b] ? mn[b] : 0u;
				r.src_count = src_count; r.snk_count = count[b];
				r.info = a | b << 2 | link[a] << 8 | link[b] << 16;
				r.reserved = 0;
				*reinterpret_cast<Bubble *>(o + 2 * NW) = r;
			}
	}
	n_branches = cl_wave_sum(n_branches);
	n_reached = cl_wave_sum(n_reached);
	if (lane == 0) {
		if (n_branches) atomicAdd(ctr + BB_N_BRANCHES, (unsigned long long)n_branches);
		if (n_reached) atomicAdd(ctr + BB_N_REACHED, (unsigned long long)n_reached);
	}
}

// w < 0: base_a << 2 | base_b; else word w of s
static __global__ __launch_bounds__(TPB) void k_bb_sortkey(const uint64_t *__restrict__ raw, int stride, int nw, const uint32_t *__restrict__ order, uint64_t n, int w,
                                                           uint64_t *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *r = raw + (uint64_t)order[i] * stride;
		const uint32_t info = reinterpret_cast<const Bubble *>(r + 2 * nw)->info;
		out[i] = w < 0 ? (uint64_t)((info & 3u) << 2 | (info >> 2 & 3u)) : r[w];
	}
}

static __global__ __launch_bounds__(TPB) void k_bb_iota(uint32_t *__restrict__ order, uint64_t n)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) order[i] = (uint32_t)i;
}

static __global__ __launch_bounds__(TPB) void k_bb_permute(const uint64_t *__restrict__ raw, int stride, int nw, const uint32_t *__restrict__ order, uint64_t n,
                                                           uint64_t *__restrict__ keys, Bubble *__restrict__ rec, unsigned long long *ctr)
{
	unsigned long long bytes = 0;
	uint32_t longest = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *r = raw + (uint64_t)order[i] * stride;
		for (int w = 0; w < 2 * nw; w++) keys[i * 2 * nw + w] = r[w];
		const Bubble bb = *reinterpret_cast<const Bubble *>(r + 2 * nw);
		rec[i] = bb;
		bytes += (unsigned long long)bb.len_a + bb.len_b + 2ULL;
		longest = bb.len_a > longest ? bb.len_a : longest;
		longest = bb.len_b > longest ? bb.len_b : longest;
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		bytes += __shfl_xor(bytes, d);
		const uint32_t o = __shfl_xor(longest, d);
		longest = o > longest ? o : longest;
	}
	if ((threadIdx.x & 63) == 0 && bytes) {
		atomicAdd(ctr + BB_PATH_BYTES, bytes);
		atomicMax(ctr + BB_LONGEST, (unsigned long long)longest);
	}
}

// branch j of the n bubbles from `first` on: j >> 1 the bubble, j & 1 side a or b; its len + 1 bytes go to bases[offs[j] ..].  A branch
// that does not walk as it did at begin (the table is the one of begin: it does) stops and counts in *bad.
template <int NW>
__global__ __launch_bounds__(TPB) void k_bb_paths(Table<NW> tbl, int K, BubbleRule rule, const uint64_t *__restrict__ keys, const Bubble *__restrict__ rec, uint64_t first,
                                                  uint64_t n, const uint64_t *__restrict__ offs, uint8_t *__restrict__ bases, unsigned long long *bad)
{
	const Key<NW> mask = cl_mask<NW>(K);
	for (uint64_t j = blockIdx.x * (uint64_t)TPB + threadIdx.x; j < 2 * n; j += (uint64_t)gridDim.x * TPB) {
		const uint64_t i = first + (j >> 1);
		const Bubble bb = rec[i];
		const uint32_t len = j & 1 ? bb.len_b : bb.len_a, b0 = j & 1 ? bb.info >> 2 & 3u : bb.info & 3u;
		Key<NW> s;
#pragma unroll
		for (int w = 0; w < NW; w++) s.w[w] = keys[i * 2 * NW + w];
		Key<NW> cur = cl_next<NW>(s, b0, mask), rcur = cl_prev<NW>(key_revcomp<NW>(s, K), b0 ^ 2u, K);
		uint8_t *o = bases + offs[j];
		o[0] = (uint8_t)b0;
		uint64_t val;
		uint32_t count;
		bool ok = bb_probe<NW>(tbl, cur, rcur, rule.live, val, count);
		for (uint32_t k = 1; ok && k <= len; k++) {
			Key<NW> y, ry;
			uint64_t yval;
			uint32_t ycount, yb;
			ok = bb_succ<NW>(tbl, cur, rcur, val, K, mask, rule.live, BB_NO_BASE, y, ry, yval, ycount, yb) == 1;
			if (!ok) break;
			o[k] = (uint8_t)yb;
			cur = y; rcur = ry; val = yval;
		}
		if (!ok) atomicAdd(bad, 1ULL);
	}
}

} // namespace sdt
