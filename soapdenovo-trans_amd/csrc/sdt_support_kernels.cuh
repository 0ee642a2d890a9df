// sdt_support_kernels.cuh -- read support tallied on the unitig list (the rule: include/sdt_gpu.h): the walk of k_th_reads that counts
// instead of writing.  Nothing here writes ent, aux or lab; what is written is the tally of the context's own:
//   us    : 16 B per unitig, (segs, kmers).
//   along : 8 words of 8 B per unitig, by (oriented unitig << 2 | base): the traversals of the link that leaves it with that base.
//   two hash sets, open addressing, a 64-bit key claimed by compare-and-swap, a 64-bit count beside it:
//     junctions, 24 B: key = 1 + (unitig of via << 4 | the base that leaves (via, -) towards the one end << 2 | the base that leaves (via, +)
//                towards the other).  A passage and its mirror make the same key; both ends, in the form whose via has o = 0, are stored
//                beside it by the lane that claims the entry (they are functions of the key where the link ends of the table agree;
//                where they do not, the ends are those of the first passage that came).
//     mate links, 16 B: key = 1 + (from << 32 | to) of the smaller of the pair's two forms (an oriented unitig is below 2^32 - 2).
//   ctr   : the totals, the sets' sizes and their drops, SP_COUNTERS words.
//   k_sp_reads<NW> : ONE WAVEFRONT PER READ OR PER PAIR, 64 consecutive k-mer positions per step, one walk.  Placement, the position before,
//                    the two ballots and the runs are those of k_th_reads.  A start lane with join 1 adds to along of (the oriented unitig
//                    of the position before, its base); a lane whose segment closes within the step adds to us, the segment that stays
//                    open is carried in uniform registers and added by lane 0 when it closes.  What a start needs of THE START BEFORE IT
//                    -- its join, the oriented unitig before it and the base of its link's mirror -- comes through one cross-lane read of
//                    the highest start bit below the lane, or from a uniform carry when that start lies in an earlier step.  The last
//                    segment of each mate is carried the same way; after mate 2 lane 0 inserts the pair.  Every add is a 64-bit atomic
//                    whose result is not used, so it is done at the memory side; the totals are summed per wavefront in uniform
//                    registers and added once when the wavefront has no more reads.  No LDS, no scratch, no limit on the length of a read.
//   k_sp_links<NW> : one lane per link record: along of the record and of its mirror.
#pragma once
#include "sdt_thread_kernels.cuh"

namespace sdt {

struct UnitigSupport {                                   // == sdt_unitig_support of include/sdt_gpu.h
	unsigned long long segs, kmers;
};
struct LinkSupport {                                     // == sdt_link_support
	unsigned long long along, against;
};
struct JunctionEnt {
	unsigned long long key;
	uint32_t from, to;
	unsigned long long count;
};
static_assert(sizeof(JunctionEnt) == 24, "a junction entry is 24 bytes");
struct MateEnt {
	unsigned long long key, count;
};

constexpr unsigned long long SP_EMPTY = 0;               // no key: what is stored is the key + 1, so a cleared block is two empty sets
// ctr: [0 .. 11] the totals of include/sdt_gpu.h ([5] and [11] are made on the host), then the entries of the two sets, and their drops
constexpr int SP_READS = 0, SP_PLACED = 1, SP_SEGS = 2, SP_LIVE = 3, SP_TRAV = 4, SP_NO_RECORD = 5, SP_PASSAGES = 6, SP_PAIRS = 7, SP_PAIRS_PLACED = 8,
              SP_PAIRS_WITHIN = 9, SP_PAIRS_LINKED = 10, SP_DROPPED = 11, SP_N_JUNCTIONS = 12, SP_N_MATES = 13, SP_JUNCTIONS_DROPPED = 16,
              SP_MATES_DROPPED = 32, SP_COUNTERS = 48;    // (the two drop counters in 128-byte lines of their own: every insertion loads one)

struct SupportTally {
	UnitigSupport *us;
	unsigned long long *along;
	JunctionEnt *jn;                                     // nullptr: not kept
	uint64_t jn_mask, jn_cap;                            // slots - 1 (a power of two), the entries it may hold
	MateEnt *mt;
	uint64_t mt_mask, mt_cap;
	unsigned long long *ctr;
};

__device__ inline uint64_t sp_mix(uint64_t x)
{
	x ^= x >> 33; x *= 0xFF51AFD7ED558CCDULL;
	x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ULL;
	return x ^ (x >> 33);
}

// the entry of `key`, claimed if need be (*claimed), or nullptr where the key finds no room.  An entry is claimed before it is counted, so
// *n is the number of distinct keys and the set is FULL exactly when *n > cap, whatever the order the keys came in: that is when
// *dropped leaves 0.  Once it is full its list is lost, so nothing more is looked up: a drop is counted and that is all -- a set that
// is overshot many times over costs one load per key, not a walk over a table without a free slot.  (The load is of *dropped, which
// nobody writes before the set is full, and not of *n: loading the counter that every new key adds to made the add over pairs, where
// nearly every pair is a new key, four times as slow.)  Until then the keys past cap that are in flight stay in the table (there are
// at least twice as many slots as cap)
template <class E>
__device__ inline E *sp_entry(E *ent, uint64_t mask, uint64_t cap, unsigned long long key, unsigned long long *n, unsigned long long *dropped, bool &claimed)
{
	claimed = false;
	if (__hip_atomic_load(dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
		atomicAdd(dropped, 1ULL);
		return nullptr;
	}
	uint64_t s = sp_mix(key) & mask;
	for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
		unsigned long long k = __hip_atomic_load(&ent[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (k == SP_EMPTY) {
			k = atomicCAS(&ent[s].key, SP_EMPTY, key);
			if (k == SP_EMPTY) {
				if (atomicAdd(n, 1ULL) >= cap) atomicAdd(dropped, 1ULL);
				claimed = true;
				return ent + s;
			}
		}
		if (k == key) return ent + s;
	}
	atomicAdd(dropped, 1ULL);
	return nullptr;
}

// per = 1: item i is read i; per = 2: item i is the pair of reads 2 i and 2 i + 1
template <int NW>
__global__ __launch_bounds__(TPB) void k_sp_reads(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nitems, int per, int K,
                                                  uint32_t min_link, Table<NW> tbl, const uint2 *__restrict__ lab, SupportTally out)
{
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t above_me = ~((2ULL << lane) - 1ULL), below_me = (1ULL << lane) - 1ULL;
	unsigned long long t_reads = 0, t_placed = 0, t_segs = 0, t_live = 0, t_trav = 0, t_pass = 0, t_pairs = 0, t_both = 0, t_within = 0, t_linked = 0;
	for (uint64_t item = blockIdx.x * (uint64_t)(TPB / 64) + (uint64_t)wave; item < nitems; item += (uint64_t)gridDim.x * (TPB / 64)) {
		uint32_t mate1 = TH_NONE, mate2 = TH_NONE;               // the last segment of each mate (uniform)
		for (int m = 0; m < per; m++) {
			const uint64_t r = item * (uint64_t)per + (uint64_t)m;
			const uint64_t start = offs[r], len = offs[r + 1] - start;
			const uint64_t nk = len >= (uint64_t)K ? len - (uint64_t)K + 1 : 0;
			uint32_t nsegs = 0, last_ou = TH_NONE;
			// lane 63 of the step before (uniform); none before the first step
			uint32_t c_u = TH_NONE, c_io = 0, c_fwd = 0, c_rb = 0;
			uint64_t c_val = 0;
			// the segment that is open at the end of the step before (uniform)
			bool open = false;
			uint32_t o_u = 0, o_kmers = 0;
			// the latest start of the steps before (uniform): the oriented unitig before it, and its join | the base of its link's mirror << 2
			uint32_t s_f = 0, s_info = 0;
			for (uint64_t p0 = 0; p0 < nk; p0 += 64) {
				const uint64_t p = p0 + (uint64_t)lane;
				uint32_t u = TH_NONE, io = 0, b = 0, rb = 0;
				bool fwd = false;
				uint64_t val = 0;
				if (p < nk) {
					const Key<NW> fw = global_kmer<NW>(words, start + p, K);
					const Key<NW> rc = key_revcomp<NW>(fw, K);
					b = (uint32_t)fw.w[NW - 1] & 3u;
					rb = (uint32_t)rc.w[NW - 1] & 3u;                // the base with which revcomp(w_p) is reached from revcomp(w_p+1)
					if (!th_place<NW>(tbl, lab, fw, rc, u, io, fwd, val)) u = TH_NONE;
				}
				// the position before: the lane below, or the carry
				uint32_t pu = __shfl_up(u, 1), pio = __shfl_up(io, 1), pfwd = __shfl_up((uint32_t)fwd, 1), prb = __shfl_up(rb, 1);
				uint64_t pval = __shfl_up(val, 1);
				if (lane == 0) { pu = c_u; pio = c_io; pfwd = c_fwd; pval = c_val; prb = c_rb; }
				c_u = th_lane32(u, 63);
				c_io = th_lane32(io, 63);
				c_fwd = th_lane32((uint32_t)fwd, 63);
				c_rb = th_lane32(rb, 63);
				c_val = th_lane64(val, 63);
				const bool live = u != TH_NONE, plive = pu != TH_NONE;
				const bool cont = live && plive && u == pu && io == ((io & 1u) ? pio - 2u : pio + 2u);
				const bool st = live && !cont;
				const uint32_t join = !plive ? 0u : bb_link(pval, pfwd != 0, b) >= min_link ? 1u : 2u;
				const uint64_t startm = __ballot(st), deadm = __ballot(!live), endm = startm | deadm;
				t_live += (unsigned long long)__popcll(~deadm);
				if (open) {                                          // (uniform)
					const uint32_t run = endm ? (uint32_t)__builtin_ctzll(endm) : 64u;
					o_kmers += run;
					if (run < 64u) {
						if (lane == 0) {
							atomicAdd(&out.us[o_u].segs, 1ULL);
							atomicAdd(&out.us[o_u].kmers, (unsigned long long)o_kmers);
						}
						open = false;
					}
				}
				if (!startm) continue;                               // (uniform)
				const uint64_t ends_above = endm & above_me;
				const uint32_t run = (ends_above ? (uint32_t)__builtin_ctzll(ends_above) : 64u) - (uint32_t)lane;
				const int l_last = 63 - __builtin_clzll(startm);
				const uint32_t ou = u << 1 | (io & 1u), pou = pu << 1 | (pio & 1u);      // (pou: of the segment before, where join != 0)
				if (st && ends_above) {
					atomicAdd(&out.us[u].segs, 1ULL);
					atomicAdd(&out.us[u].kmers, (unsigned long long)run);
				}
				const bool trav = st && join == 1u;
				if (trav) atomicAdd(out.along + ((uint64_t)pou << 2 | b), 1ULL);
				// the start before this one: the highest start bit below the lane, or the carry
				const uint64_t below = startm & below_me;
				const uint32_t mine = join | prb << 2;
				const int src = below ? 63 - __builtin_clzll(below) : lane;
				uint32_t q_info = __shfl(mine, src), q_f = __shfl(pou, src);
				if (!below) { q_info = s_info; q_f = s_f; }
				const bool pass = trav && (q_info & 3u) == 1u;
				if (pass && out.jn) {
					// (f, v, t) = (q_f, pou, ou); with o(v) = 1 its mirror (t ^ 1, v ^ 1, f ^ 1) is the form that is kept
					const uint32_t rin = q_info >> 2, v = pou;
					const unsigned long long key = (unsigned long long)(v >> 1) << 4 | ((v & 1u) ? b << 2 | rin : rin << 2 | b);      // (+ 1 below)
					bool claimed;
					JunctionEnt *e = sp_entry<JunctionEnt>(out.jn, out.jn_mask, out.jn_cap, key + 1ULL, out.ctr + SP_N_JUNCTIONS, out.ctr + SP_JUNCTIONS_DROPPED, claimed);
					if (e) {
						if (claimed) {                               // (one writer: the two ends are those of one passage that was made)
							e->from = (v & 1u) ? ou ^ 1u : q_f;
							e->to = (v & 1u) ? q_f ^ 1u : ou;
						}
						atomicAdd(&e->count, 1ULL);
					}
				}
				t_trav += (unsigned long long)__popcll(__ballot(trav));
				t_pass += (unsigned long long)__popcll(__ballot(pass));
				s_info = th_lane32(mine, l_last);
				s_f = th_lane32(pou, l_last);
				last_ou = th_lane32(ou, l_last);
				if (!(endm & ~((2ULL << l_last) - 1ULL))) {          // nothing ends the last segment of the step: it stays open
					open = true;
					o_u = th_lane32(u, l_last);
					o_kmers = 64u - (uint32_t)l_last;
				}
				nsegs += (uint32_t)__popcll(startm);
			}
			if (open && lane == 0) {
				atomicAdd(&out.us[o_u].segs, 1ULL);
				atomicAdd(&out.us[o_u].kmers, (unsigned long long)o_kmers);
			}
			t_reads++;
			t_placed += nsegs ? 1u : 0u;
			t_segs += nsegs;
			if (m == 0) mate1 = last_ou;
			else mate2 = last_ou;
		}
		if (per == 2) {
			t_pairs++;
			if (mate1 != TH_NONE && mate2 != TH_NONE) {
				// mate 2 is read against the fragment: its last segment, turned round, is where the fragment goes on
				const uint32_t from = mate1, to = mate2 ^ 1u;
				t_both++;
				if (from == to) t_within++;
				else {
					t_linked++;
					const unsigned long long k1 = (unsigned long long)from << 32 | to, k2 = (unsigned long long)(to ^ 1u) << 32 | (from ^ 1u);
					if (out.mt && lane == 0) {
						bool claimed;
						MateEnt *e = sp_entry<MateEnt>(out.mt, out.mt_mask, out.mt_cap, (k1 < k2 ? k1 : k2) + 1ULL, out.ctr + SP_N_MATES, out.ctr + SP_MATES_DROPPED, claimed);
						if (e) atomicAdd(&e->count, 1ULL);
					}
				}
			}
		}
	}
	if (lane == 0) {
		if (t_reads) atomicAdd(out.ctr + SP_READS, t_reads);
		if (t_placed) atomicAdd(out.ctr + SP_PLACED, t_placed);
		if (t_segs) atomicAdd(out.ctr + SP_SEGS, t_segs);
		if (t_live) atomicAdd(out.ctr + SP_LIVE, t_live);
		if (t_trav) atomicAdd(out.ctr + SP_TRAV, t_trav);
		if (t_pass) atomicAdd(out.ctr + SP_PASSAGES, t_pass);
		if (t_pairs) atomicAdd(out.ctr + SP_PAIRS, t_pairs);
		if (t_both) atomicAdd(out.ctr + SP_PAIRS_PLACED, t_both);
		if (t_within) atomicAdd(out.ctr + SP_PAIRS_WITHIN, t_within);
		if (t_linked) atomicAdd(out.ctr + SP_PAIRS_LINKED, t_linked);
	}
}

// out[i] for link record i: along of (from, o, b), and along of its mirror, the link that leaves (to, o' ^ 1) for (from, o ^ 1): its base
// is the last of the reverse complement of the record's out word.  keys: the list's, 2 NW words per unitig (x0, the last word)
template <int NW>
__global__ __launch_bounds__(TPB) void k_sp_links(const UnitigLink *__restrict__ links, uint64_t n, const uint64_t *__restrict__ keys, int K,
                                                  const unsigned long long *__restrict__ along, LinkSupport *__restrict__ out)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const UnitigLink l = links[i];
		const uint32_t o = l.info & 1u, o2 = l.info >> 1 & 1u, b = l.info >> 2 & 3u;
		const uint64_t *kw = keys + (uint64_t)l.from * 2 * NW + (o ? 0 : NW);
		Key<NW> w;
#pragma unroll
		for (int j = 0; j < NW; j++) w.w[j] = kw[j];
		if (!o) w = key_revcomp<NW>(w, K);                       // (o = 1: the out word is revcomp(x0))
		const uint32_t mb = (uint32_t)w.w[NW - 1] & 3u;
		out[i] = LinkSupport{along[(uint64_t)(l.from << 1 | o) << 2 | b], along[(uint64_t)(l.to << 1 | (o2 ^ 1u)) << 2 | mb]};
	}
}

} // namespace sdt
