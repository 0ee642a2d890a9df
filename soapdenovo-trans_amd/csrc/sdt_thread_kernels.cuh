// sdt_thread_kernels.cuh -- reads threaded through the unitig list of the counted node table (the rule: include/sdt_gpu.h): a label per
// table slot that says in which unitig and where in it the slot's node lies, and the reads as paths over those labels.  Nothing here
// writes ent or aux.  Liveness, the oriented words and the successors are those of the bubbles and the unitigs (sdt_bubble_kernels.cuh,
// sdt_unitig_kernels.cuh); what is written by slot is one array of the context's own, lab (8 B per slot, all ones = no live node).
//   th_probe / th_succ : bb_probe / bb_succ that also give the slot of the node they found.
//   k_th_label<NW>   : ONE LANE PER UNITIG, grid-stride: the chain again from the kept x0, as k_ug_seqs walks it, one 8-byte store per
//                      node: (id, pos << 1 | s).  The unitigs partition the live nodes, so every slot has one writer: plain stores, no
//                      atomics but the three counters per wavefront.  The ids exist only after the sort inside unitigs_begin, which is
//                      why this is a walk of its own and no part of k_ug_walk.
//   k_th_lookup<NW>  : one lane per query k-mer, either strand, after k_cl_lookup.
//   k_th_reads<NW, WRITE> : ONE WAVEFRONT PER READ, 64 consecutive k-mer positions per step, after k_cl_reads.  A lane builds its k-mer,
//                      finds the canonical node's slot (the link word comes with the same 16 bytes for one key word) and loads the
//                      8-byte label.  The placement, strand and link word of the position before come from the lane below (__shfl_up);
//                      lane 0 takes them from lane 63 of the step before, which is wave-uniform (readlane into scalars).  One ballot
//                      gives the segment starts, one the positions that are not live; the run of the segment that starts at a lane is
//                      the distance to the next bit of either above it.  A segment still open at the end of a step is carried in uniform
//                      registers and written when it closes, at the read's offset plus its number among the read's segments.  No LDS, no
//                      atomics, no limit on the length of a read.  WRITE = false: the read records (with segs) and the segment counts;
//                      WRITE = true, after an exclusive scan of the counts: the segment records at their offsets.
#pragma once
#include "sdt_unitig_kernels.cuh"

namespace sdt {

struct ReadPath {                                        // == sdt_read_path of include/sdt_gpu.h
	uint32_t kmers, live, segs, breaks, first, last;
};
static_assert(sizeof(ReadPath) == 24, "sdt_read_path is six 32-bit words");

struct PathSeg {                                         // == sdt_path_seg
	uint32_t unitig, info, read_pos, unitig_pos, kmers, reserved;
};
static_assert(sizeof(PathSeg) == 24, "sdt_path_seg is six 32-bit words");

struct UnitigPos {                                       // == sdt_unitig_pos
	uint32_t unitig, pos, info, reserved;
};

constexpr uint32_t TH_NONE = 0xFFFFFFFFu;                // SDT_UNITIG_NONE
constexpr uint32_t TH_MAX_NODES = 0x7FFFFFFFu;           // pos << 1 | s is 32-bit, and 0xFFFFFFFF is taken
// counters of unitigs_index
constexpr int TH_N_NODES = 0, TH_N_BROKEN = 1, TH_N_TOO_LONG = 2, TH_COUNTERS = 3;

// bb_probe that also gives the slot
template <int NW>
__device__ inline bool th_probe(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, const ClusterRule &rule, uint64_t &val, uint32_t &count, uint64_t &slot_out)
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
		slot_out = slot;
		return cl_live(0, val, aux, rule, count);
	}
	return false;
}

// bb_succ (no known base) that also gives the slot of the last successor
template <int NW>
__device__ inline uint32_t th_succ(const Table<NW> &tbl, const Key<NW> &x, const Key<NW> &rx, uint64_t val, int K, const Key<NW> &mask, const ClusterRule &rule,
                                   Key<NW> &y, Key<NW> &ry, uint64_t &yval, uint64_t &yslot)
{
	const bool fwd = !key_less<NW>(rx, x);
	uint32_t deg = 0;
	for (uint32_t b = 0; b < 4; b++) {
		if (bb_link(val, fwd, b) < rule.min_link) continue;
		const Key<NW> n = cl_next<NW>(x, b, mask), rn = cl_prev<NW>(rx, b ^ 2u, K);
		uint64_t nval, nslot;
		uint32_t ncount;
		if (!th_probe<NW>(tbl, n, rn, rule, nval, ncount, nslot)) continue;
		deg++;
		y = n; ry = rn; yval = nval; yslot = nslot;
	}
	return deg;
}

// lab: slots entries, all ones.  Unitig i of the n of the list writes (i, pos << 1 | s) at the slot of each of its nodes.
template <int NW>
__global__ __launch_bounds__(TPB) void k_th_label(Table<NW> tbl, int K, ClusterRule rule, const uint64_t *__restrict__ keys, const Unitig *__restrict__ rec, uint64_t n,
                                                  uint2 *__restrict__ lab, unsigned long long *ctr)
{
	const Key<NW> mask = cl_mask<NW>(K);
	unsigned long long written = 0;
	uint32_t broken = 0, too_long = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t *kw = keys + i * 2 * NW;
		const uint32_t nodes = rec[i].nodes;
		if (nodes > TH_MAX_NODES) { too_long++; continue; }
		Key<NW> cur, last;
#pragma unroll
		for (int w = 0; w < NW; w++) { cur.w[w] = kw[w]; last.w[w] = kw[NW + w]; }
		Key<NW> rcur = key_revcomp<NW>(cur, K);
		uint64_t val, slot;
		uint32_t count;
		bool ok = th_probe<NW>(tbl, cur, rcur, rule, val, count, slot);
		for (uint32_t k = 0; ok; k++) {
			lab[slot] = make_uint2((uint32_t)i, k << 1 | (key_less<NW>(rcur, cur) ? 1u : 0u));
			written++;
			if (k + 1 == nodes) break;
			Key<NW> y, ry;
			uint64_t yval, yslot;
			ok = th_succ<NW>(tbl, cur, rcur, val, K, mask, rule, y, ry, yval, yslot) == 1;
			cur = y; rcur = ry; val = yval; slot = yslot;
		}
		if (!ok || !key_eq<NW>(cur, last)) broken++;
	}
	written = ug_wave_sum64(written);
	broken = cl_wave_sum(broken);
	too_long = cl_wave_sum(too_long);
	if ((threadIdx.x & 63) == 0) {
		if (written) atomicAdd(ctr + TH_N_NODES, written);
		if (broken) atomicAdd(ctr + TH_N_BROKEN, (unsigned long long)broken);
		if (too_long) atomicAdd(ctr + TH_N_TOO_LONG, (unsigned long long)too_long);
	}
}

// table_find that brings the node's link word along: for one key word it lies in the 16 bytes that the probe loads
template <int NW> __device__ inline bool th_find(const Table<NW> &tbl, const Key<NW> &key, uint64_t &slot_out, uint64_t &val)
{
	uint64_t slot, lo, n;
	probe_begin<NW>(tbl, key, slot, lo, n);
	for (uint64_t probe = 0; probe < n; probe++, slot = probe_next(slot, lo, n)) {
		uint64_t key0, v;
		cl_load<NW>(tbl, slot, key0, v);
		if (key0 == KEY_EMPTY) return false;
		bool same = key0 == key.w[0];
#pragma unroll
		for (int w = 1; w < NW; w++) same = same && tbl.ent[slot].key[w] == key.w[w];
		if (!same) continue;
		slot_out = slot;
		val = v;
		return true;
	}
	return false;
}

// place(w) of the word fw as given (rc: its reverse complement): the unitig, pos << 1 | o; fwd: fw is its node's stored key; val: the
// node's link word.  false: absent or not live
template <int NW>
__device__ inline bool th_place(const Table<NW> &tbl, const uint2 *__restrict__ lab, const Key<NW> &fw, const Key<NW> &rc, uint32_t &u, uint32_t &io, bool &fwd,
                                uint64_t &val)
{
	fwd = !key_less<NW>(rc, fw);
	uint64_t slot;
	if (!th_find<NW>(tbl, fwd ? fw : rc, slot, val)) return false;
	const uint2 l = lab[slot];
	if (l.x == TH_NONE) return false;
	u = l.x;
	io = l.y ^ (fwd ? 0u : 1u);                          // s is for the stored key: the other strand runs the other way
	return true;
}

template <int NW>
__global__ __launch_bounds__(TPB) void k_th_lookup(const uint64_t *__restrict__ keys, uint64_t n, int K, Table<NW> tbl, const uint2 *__restrict__ lab,
                                                   UnitigPos *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		Key<NW> fw;
#pragma unroll
		for (int w = 0; w < NW; w++) fw.w[w] = keys[i * NW + w];
		const Key<NW> rc = key_revcomp<NW>(fw, K);
		uint32_t u = 0, io = 0;
		bool fwd;
		uint64_t val;
		out[i] = th_place<NW>(tbl, lab, fw, rc, u, io, fwd, val) ? UnitigPos{u, io >> 1, io & 1u, 0u} : UnitigPos{TH_NONE, 0u, 0u, 0u};
	}
}

__device__ inline uint32_t th_lane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ inline uint64_t th_lane64(uint64_t v, int l) { return (uint64_t)th_lane32((uint32_t)(v >> 32), l) << 32 | th_lane32((uint32_t)v, l); }

// WRITE = false: rec[r] and counts[r] = its segments.  WRITE = true: the segments of read r at segs[seg_offs[r] ..] (seg_offs: the
// exclusive scan of counts); rec and counts are not touched.
template <int NW, bool WRITE>
__global__ __launch_bounds__(TPB) void k_th_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads, int K, uint32_t min_link,
                                                  Table<NW> tbl, const uint2 *__restrict__ lab, ReadPath *__restrict__ rec, uint64_t *__restrict__ counts,
                                                  const uint64_t *__restrict__ seg_offs, PathSeg *__restrict__ segs)
{
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t above_me = ~((2ULL << lane) - 1ULL);      // the lanes above this one (lane 63: none)
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + (uint64_t)wave; r < nreads; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		const uint64_t nk = len >= (uint64_t)K ? len - (uint64_t)K + 1 : 0;
		const uint64_t out0 = WRITE ? seg_offs[r] : 0;
		uint32_t nlive = 0, nsegs = 0, nbreaks = 0, first = TH_NONE, last = TH_NONE;
		// lane 63 of the step before (uniform); none before the first step
		uint32_t c_u = TH_NONE, c_io = 0, c_fwd = 0;
		uint64_t c_val = 0;
		// the segment that is open at the end of the step before (uniform)
		bool open = false;
		uint32_t o_u = 0, o_info = 0, o_rpos = 0, o_upos = 0, o_kmers = 0, o_idx = 0;
		for (uint64_t p0 = 0; p0 < nk; p0 += 64) {
			const uint64_t p = p0 + (uint64_t)lane;
			uint32_t u = TH_NONE, io = 0, b = 0;
			bool fwd = false;
			uint64_t val = 0;
			if (p < nk) {
				const Key<NW> fw = global_kmer<NW>(words, start + p, K);
				const Key<NW> rc = key_revcomp<NW>(fw, K);
				b = (uint32_t)fw.w[NW - 1] & 3u;
				if (!th_place<NW>(tbl, lab, fw, rc, u, io, fwd, val)) u = TH_NONE;
			}
			// the position before: the lane below, or the carry
			uint32_t pu = __shfl_up(u, 1), pio = __shfl_up(io, 1), pfwd = __shfl_up((uint32_t)fwd, 1);
			uint64_t pval = __shfl_up(val, 1);
			if (lane == 0) { pu = c_u; pio = c_io; pfwd = c_fwd; pval = c_val; }
			c_u = th_lane32(u, 63);
			c_io = th_lane32(io, 63);
			c_fwd = th_lane32((uint32_t)fwd, 63);
			c_val = th_lane64(val, 63);
			const bool live = u != TH_NONE, plive = pu != TH_NONE;
			const bool cont = live && plive && u == pu && io == ((io & 1u) ? pio - 2u : pio + 2u);
			const bool st = live && !cont;
			const uint32_t join = !plive ? 0u : bb_link(pval, pfwd != 0, b) >= min_link ? 1u : 2u;
			const uint64_t startm = __ballot(st), deadm = __ballot(!live), endm = startm | deadm;
			nlive += (uint32_t)__popcll(~deadm);
			if (open) {                                          // (uniform)
				const uint32_t run = endm ? (uint32_t)__builtin_ctzll(endm) : 64u;
				o_kmers += run;
				if (run < 64u) {
					if (WRITE && lane == 0) segs[out0 + o_idx] = PathSeg{o_u, o_info, o_rpos, o_upos, o_kmers, 0u};
					open = false;
				}
			}
			if (!startm) continue;                               // (uniform)
			const uint64_t ends_above = endm & above_me;
			const uint32_t run = (ends_above ? (uint32_t)__builtin_ctzll(ends_above) : 64u) - (uint32_t)lane;
			const uint32_t idx = nsegs + (uint32_t)__popcll(startm & ((1ULL << lane) - 1ULL));
			const uint32_t info = (io & 1u) | join << 1;
			const int l_first = __builtin_ctzll(startm), l_last = 63 - __builtin_clzll(startm);
			if (WRITE) {
				if (st && ends_above) segs[out0 + idx] = PathSeg{u, info, (uint32_t)p, io >> 1, run, 0u};
			} else {
				if (first == TH_NONE) first = th_lane32(u, l_first);
				last = th_lane32(u, l_last);
				nbreaks += (uint32_t)__popcll(__ballot(st && join != 1u));
			}
			if (!(endm & ~((2ULL << l_last) - 1ULL))) {          // nothing ends the last segment of the step: it stays open
				open = true;
				o_u = th_lane32(u, l_last);
				o_info = th_lane32(info, l_last);
				o_rpos = (uint32_t)p0 + (uint32_t)l_last;
				o_upos = th_lane32(io, l_last) >> 1;
				o_kmers = 64u - (uint32_t)l_last;
				o_idx = nsegs + (uint32_t)__popcll(startm) - 1u;
			}
			nsegs += (uint32_t)__popcll(startm);
		}
		if (WRITE) {
			if (open && lane == 0) segs[out0 + o_idx] = PathSeg{o_u, o_info, o_rpos, o_upos, o_kmers, 0u};
		} else if (lane == 0) {
			// (the first segment has join 0 -- nothing live lies before it -- and is no break)
			rec[r] = ReadPath{(uint32_t)nk, nlive, nsegs, nsegs ? nbreaks - 1u : 0u, first, last};
			counts[r] = nsegs;
		}
	}
}

} // namespace sdt
