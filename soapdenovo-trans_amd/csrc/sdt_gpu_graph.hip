// sdt_gpu_graph.hip -- the graph phases of pregraph on the device mirror of the graph (part of libsdt_gpu.so): the entry points of the
// ABI, their argument and state checks, and the host side of the layout.
//
//   layout      the reference's visiting order.  sdt_gpu_layout_on_device reads as its steps: layout_sort (nodes by set and first
//               occurrence), the growth schedule of every set (sdt_layout_plan.h, pure host arithmetic), the replay of the probing
//               (struct Replay: grow = rehash rounds to the fixed point and strip, put, order), layout_publish (numbering).
//               sdt_gpu_layout_sorted_keys / sdt_gpu_layout_apply are the same two ends around a replay on the host (graph.c).
//   dry runs    the read-only halves of removeMinorOut / removeSingleTips / removeMinorTips (cutTipPreGraph.c) and of
//               kmer2edges (node2edge.c): by host position, and labelled with the connected components the ordered commits may
//               run side by side (union-find over node indices), sorted by (component, node)
// Scratch owns the device buffers of a call, GCHK returns its HIP errors, LAUNCH_NW picks the kernel of the key width.
// The phases that hold node indices are templates over the index form (sdt_graph_phases.hpp): the 32-bit form is instantiated
// here, the 64-bit one in sdt_gpu_graph64.hip; the entry points pick the form the numbering fixed.
// gfx950 only; no CPU fallback.  The context is seen through sdti::GraphView (sdt_internal.hpp).
#include <vector>

#include "sdt_graph_phases.hpp"
#include "sdt_layout_plan.h"

static_assert(sdt::RP_PLAN_DEPTH_BITS == RP_DEPTH_BITS && sdt::RP_PLAN_CHUNK == AP_CH && sdt::RP_PLAN_WAVES == TPB / 64, "sdt_layout_plan.h restates these");

void sdti::graph_ext_free(GraphExt *gx)
{
	if (!gx) return;
	for (void *q : {(void *)gx->d_sval, (void *)gx->d_slot_of, (void *)gx->d_result, (void *)gx->d_wnode, (void *)gx->d_wl, (void *)gx->d_wr, (void *)gx->d_skipped,
	                (void *)gx->mo_dirty, (void *)gx->mo_cnt, (void *)gx->mo_recidx, (void *)gx->mo_cstart, (void *)gx->d_seq, (void *)gx->d_pw})
		if (q) (void)hipFree(q);
	delete gx;
}

int graph_choose_form(sdti::GraphExt *gx, uint64_t n)
{
	gx->wide = gx->want_bits == 64 || n >= 0xFFFFFFF0ULL;
	gx->base = 0;
	// (SDT_NODE_BASE: test hook -- the 64-bit form numbers the nodes from this base, so that a node index cut to 32 bits anywhere on
	// the device changes the output of a small input)
	const char *b = sdt_test_env("SDT_NODE_BASE");
	if (gx->wide && b && *b) gx->base = strtoull(b, nullptr, 0);
	if (gx->base + n >= (1ULL << 55))
		return fail(SDT_EINVAL, "node indices %llu .. %llu do not fit the 56-bit fields of the records", (unsigned long long)gx->base, (unsigned long long)(gx->base + n));
	return SDT_OK;
}

// node indices of records that leave the device are host array positions: base + position -> position (SDT_NODE_BASE only).
// stride 3 (tip walks): node | info << 56, end node, label; stride 14 (minor out): node, 8 x (neighbour << 1 | smaller) or ~0,
// 4 count words, label
static void rebase_records(uint64_t *rec, uint64_t nrec, int stride, uint64_t base)
{
	const uint64_t M = 0x00FFFFFFFFFFFFFFULL;
	for (uint64_t r = 0; r < nrec; r++) {
		uint64_t *R = rec + r * (uint64_t)stride;
		R[0] = (R[0] & ~M) | ((R[0] & M) - base);
		if (stride == 3) R[1] -= base;
		else for (int q = 1; q <= 8; q++) if (R[q] != ~0ULL) R[q] -= 2 * base;
		R[stride - 1] -= base;
	}
}

uint64_t sdti::graph_node_base(const GraphExt *gx) { return gx ? gx->base : 0; }

uint64_t *sdti::graph_take_path_words(GraphExt *gx, uint64_t n)
{
	if (!gx || !gx->d_pw || gx->pw_n != n) return nullptr;
	uint64_t *p = gx->d_pw;
	gx->d_pw = nullptr;
	gx->pw_n = 0;
	return p;
}

// (from ascending, first appearance descending): stable sort by ~first, then stable sort by from
int sdti::sort_arcs_for_output(hipStream_t stream, int cu_count, uint32_t *d_from, uint32_t *d_to, uint32_t *d_mult, uint64_t *d_first, uint64_t n)
{
	if (n < 2) return SDT_OK;
	if (n >= 0xFFFFFFFFULL) return fail(SDT_ELIMIT, "%llu arcs do not fit a 32-bit permutation", (unsigned long long)n);
	Scratch S;
	uint64_t *k0, *k1, *o2;
	uint32_t *p0, *p1, *f0, *f1, *f2, *t2, *m2;
	GCHK(S.alloc(&k0, n * 8)); GCHK(S.alloc(&k1, n * 8)); GCHK(S.alloc(&o2, n * 8));
	GCHK(S.alloc(&p0, n * 4)); GCHK(S.alloc(&p1, n * 4)); GCHK(S.alloc(&f0, n * 4)); GCHK(S.alloc(&f1, n * 4));
	GCHK(S.alloc(&f2, n * 4)); GCHK(S.alloc(&t2, n * 4)); GCHK(S.alloc(&m2, n * 4));
	const dim3 grid(sdti::scan_grid(cu_count, n));
	hipLaunchKernelGGL(k_arc_keys, grid, dim3(TPB), 0, stream, d_first, n, k0, p0);
	size_t tb1 = 0, tb2 = 0;
	GCHK(rocprim::radix_sort_pairs(nullptr, tb1, k0, k1, p0, p1, (size_t)n, 0u, 64u, stream));
	GCHK(rocprim::radix_sort_pairs(nullptr, tb2, f0, f1, p1, p0, (size_t)n, 0u, 32u, stream));
	void *tmp = nullptr;
	GCHK(S.alloc(&tmp, (tb1 > tb2 ? tb1 : tb2) + 16));
	GCHK(rocprim::radix_sort_pairs(tmp, tb1, k0, k1, p0, p1, (size_t)n, 0u, 64u, stream));
	hipLaunchKernelGGL(k_arc_from_of, grid, dim3(TPB), 0, stream, d_from, p1, n, f0);
	GCHK(rocprim::radix_sort_pairs(tmp, tb2, f0, f1, p1, p0, (size_t)n, 0u, 32u, stream));
	hipLaunchKernelGGL(k_arc_gather, grid, dim3(TPB), 0, stream, p0, n, d_from, d_to, d_mult, d_first, f2, t2, m2, o2);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(d_from, f2, n * 4, hipMemcpyDeviceToDevice, stream));
	GCHK(hipMemcpyAsync(d_to, t2, n * 4, hipMemcpyDeviceToDevice, stream));
	GCHK(hipMemcpyAsync(d_mult, m2, n * 4, hipMemcpyDeviceToDevice, stream));
	GCHK(hipMemcpyAsync(d_first, o2, n * 8, hipMemcpyDeviceToDevice, stream));
	GCHK(hipStreamSynchronize(stream));
	return SDT_OK;
}

// ---- layout: the steps sdt_gpu_layout_on_device shares with sdt_gpu_layout_sorted_keys / sdt_gpu_layout_apply ---------------
// what both layouts ask of the context and of their arguments
static int layout_check(const GraphView &v, int p, int nw_variant)
{
	if (!v.d_first) return fail(SDT_ESTATE, "first-occurrence ordinals were not tracked: init with SDT_FLAG_TRACK_FIRST");
	if (p < 1 || p > 256) return fail(SDT_EINVAL, "layout on the device: 1..256 sets, asked for %d", p);
	if (nw_variant < v.nw || nw_variant > 4) return fail(SDT_EINVAL, "a %d-word variant cannot hold %d-word keys", nw_variant, v.nw);
	return SDT_OK;
}

// the n nodes sorted by (set, first occurrence): set_start[0 .. p] on the host; on the device (S owns all of it) the keys in that order
// and v1s, rank -> table slot.  k1, v0s and, for keys of more than one word, k0 are of no use afterwards: the caller may free them
struct SortedNodes { uint64_t *k0, *k1, *v0s, *v1s, *d_keys; };
static int layout_sort(sdt_ctx *c, const GraphView &v, Scratch &S, int p, int nw_variant, uint64_t n, uint64_t *set_start, const CallTimer &T, SortedNodes &o)
{
	const uint64_t m = n ? n : 1;
	uint64_t *d_ss;
	unsigned long long *d_cur;
	GCHK(S.alloc(&o.k0, m * 8)); GCHK(S.alloc(&o.k1, m * 8)); GCHK(S.alloc(&o.v0s, m * 8)); GCHK(S.alloc(&o.v1s, m * 8));
	GCHK(S.alloc(&d_cur, 8)); GCHK(S.alloc(&d_ss, (size_t)(p + 1) * 8));
	GCHK(hipMemsetAsync(d_cur, 0, 8, v.stream));
	LAUNCH_NW(v, k_layout_keys, sdti::scan_grid(v.cu_count, v.slots), (uint32_t)p, nw_variant, o.k0, o.v0s, (unsigned long long)n, d_cur, v.d_stats);
	GCHK(hipGetLastError());
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "layout: %llu nodes without a usable first-occurrence ordinal (>= 2^56, or more nodes than counted)", (unsigned long long)v.h_stats->probe_fail);
	T.tick("sort keys made");
	unsigned end_bit = 56;
	for (int q = p - 1; q > 0; q >>= 1) end_bit++;
	const int rc = sort_pairs<uint64_t>(v, o.k0, o.k1, o.v0s, o.v1s, n, end_bit);
	if (rc != SDT_OK) return rc;
	T.tick("sorted");
	hipLaunchKernelGGL(k_layout_set_starts, dim3((p + 1 + 63) / 64), dim3(64), 0, v.stream, o.k1, n, (uint32_t)p, d_ss);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(set_start, d_ss, (size_t)(p + 1) * 8, hipMemcpyDeviceToHost, v.stream));
	// k0 is free again: the keys in sorted order go there (NW words each: reuse needs NW * n words)
	if (v.nw == 1) o.d_keys = o.k0; else GCHK(S.alloc(&o.d_keys, m * v.nw * 8));
	LAUNCH_NW(v, k_layout_gather_keys, sdti::scan_grid(v.cu_count, m), o.v1s, n, o.d_keys);
	GCHK(hipGetLastError());
	GCHK(hipStreamSynchronize(v.stream));
	T.tick("keys gathered");
	return SDT_OK;
}

// number the n nodes: idx[slot of the node at visiting position i] = i, slot_of[i] = that slot (order[i] = its rank in sval), and make
// that the numbering of the context.  The order is on the device already (d_order), or it is uploaded here from h_order.  first_done:
// the first-occurrence ordinals have done their work.  not_ranks() is the caller's refusal of an order that is no permutation
template <class Refusal>
static int layout_publish(sdt_ctx *c, const GraphView &v, Scratch &S, const uint64_t *sval, uint64_t *d_order, const uint64_t *h_order, uint64_t n, bool first_done,
                          Refusal not_ranks)
{
	sdti::GraphExt *gx = ext_of(v);
	if (*v.d_idx) { (void)hipFree(*v.d_idx); *v.d_idx = nullptr; }
	*v.idx_slots = *v.idx_n = 0;
	if (gx->d_slot_of) { (void)hipFree(gx->d_slot_of); gx->d_slot_of = nullptr; gx->n_nodes = 0; }
	// after a replay on the device every limit it can run into lies behind: the first-occurrence ordinals go, and the node index is
	// exactly as large -- 8 bytes per table slot that it finds in the arena instead of asking the driver
	if (first_done && !sdt_test_env("SDT_KEEP_FIRST")) { const int rc = sdti::drop_first(c); if (rc != SDT_OK) return rc; }
	uint64_t *d_idx, *d_slot_of;
	const uint64_t m = n ? n : 1;
	const bool from_host = !d_order;
	if (from_host) GCHK(S.alloc(&d_order, m * 8));
	GCHK(S.alloc(&d_idx, v.slots * 8)); GCHK(S.alloc(&d_slot_of, m * 8));
	GCHK(hipMemsetAsync(d_idx, 0xFF, v.slots * 8, v.stream));
	int rc = from_host ? sdti::h2d_big(v.copy_stream, d_order, h_order, n * 8) : SDT_OK;
	if (rc != SDT_OK) return rc;
	rc = gx->wide ? sdti::layout_number(v, ix64_of(gx), sval, d_order, n, d_idx, d_slot_of) : sdti::layout_number(v, Ix32(), sval, d_order, n, d_idx, d_slot_of);
	if (rc != SDT_OK) return rc;
	if (sdti::sync_stats(c) != SDT_OK) return not_ranks();
	*v.d_idx = (uint64_t *)S.release(d_idx);
	*v.idx_slots = v.slots;
	*v.idx_n = n;
	gx->d_slot_of = (uint64_t *)S.release(d_slot_of);
	gx->n_nodes = n;
	return SDT_OK;
}

// ---- the replay of the probing: every set's generations side by side (sdt_layout_plan.h), a growth as a fixed point of insertion
// times (sdt_graph_kernels.cuh; tools/replay_fixed_point.c is the proof on the CPU) ----------------------------------------
struct Replay {
	const GraphView &v;
	const sdt::RpSchedule &sch;
	const CallTimer &T;
	const int p;
	const uint64_t *d_keys;                                   // the keys by rank (layout_sort)
	std::vector<RpSet> sets;                                  // the sets as the next kernels see them, and the prefix sums of their items
	std::vector<unsigned long long> pre;
	// per OLD slot of a growth: time and home; per new slot: the word a round took out of it; per entry: the two lists of the rounds
	// (an entry whose time changed is listed once); the two table buffers, every set's region at its final size
	unsigned long long *tab[2], *d_time, *d_saved, *d_list[2], *d_pre, list_chunks;
	uint32_t *d_home, *d_home_slot;
	RpSet *d_sets;
	unsigned int *d_flags;
	RpRound *d_round;
	int cur = 0, total_rounds = 0;
	double t_rehash = 0, t_strip = 0, t_put = 0;              // (SDT_TIMING)

	Replay(const GraphView &v_, const sdt::RpSchedule &sch_, const CallTimer &T_, int p_, const uint64_t *set_start, const uint64_t *d_keys_)
	    : v(v_), sch(sch_), T(T_), p(p_), d_keys(d_keys_), sets(p_), pre(p_ + 1)
	{
		for (int s = 0; s < p; s++) { sets[s].key0 = set_start[s]; sets[s].tab0 = sch.tab0[s]; sets[s].m = (uint32_t)(set_start[s + 1] - set_start[s]); }
	}
	dim3 grid(unsigned long long items) const { return dim3(sdti::scan_grid(v.cu_count, items ? items : 1)); }
	bool has(int s, size_t gen) const { return gen < sch.gens[s].size(); }
	int alloc(Scratch &S, uint64_t n)
	{
		const uint64_t m = n ? n : 1, slots = sch.tab_total + 1;
		list_chunks = sdt::rp_list_chunks(n, v.cu_count);
		const unsigned long long list_cap = list_chunks * AP_CH;
		GCHK(S.alloc(&tab[0], slots * 8)); GCHK(S.alloc(&tab[1], slots * 8));
		GCHK(S.alloc(&d_time, slots * 8)); GCHK(S.alloc(&d_home_slot, slots * 4)); GCHK(S.alloc(&d_saved, slots * 8));
		GCHK(S.alloc(&d_list[0], list_cap * 8)); GCHK(S.alloc(&d_list[1], list_cap * 8)); GCHK(S.alloc(&d_round, sizeof(RpRound)));
		GCHK(S.alloc(&d_home, m * 4)); GCHK(S.alloc(&d_sets, (size_t)p * sizeof(RpSet))); GCHK(S.alloc(&d_pre, (size_t)(p + 1) * 8)); GCHK(S.alloc(&d_flags, 4));
		GCHK(hipMemsetAsync(tab[0], 0, slots * 8, v.stream));
		return SDT_OK;
	}
	int upload(const std::vector<RpSet> &h_sets)
	{
		GCHK(hipStreamSynchronize(v.stream));                  // (kernels in flight read the old copies; the host vectors change right after)
		GCHK(hipMemcpy(d_sets, h_sets.data(), (size_t)p * sizeof(RpSet), hipMemcpyHostToDevice));
		GCHK(hipMemcpy(d_pre, pre.data(), (size_t)(p + 1) * 8, hipMemcpyHostToDevice));
		return SDT_OK;
	}
	int grow(size_t gen);
	int put(size_t gen);
	int order(Scratch &S, bool wide, uint64_t n, uint64_t **d_order);
};

// the growth into generation gen's size of every set that has one: rehash init, round 0, rounds to the fixed point, strip
int Replay::grow(size_t gen)
{
	unsigned long long old_total = 0;
	for (int s = 0; s < p; s++) {
		sets[s].old_size = has(s, gen) ? sch.gens[s][gen - 1].size : 0;
		if (has(s, gen)) sets[s].size = sch.gens[s][gen].size;
		sets[s].lo = 0; sets[s].hi = has(s, gen) ? sch.gens[s][gen].lo : 0;            // ids [0, lo) are in the table
		pre[s] = old_total;
		old_total += sets[s].old_size;
	}
	pre[p] = old_total;
	int rc = upload(sets); if (rc != SDT_OK) return rc;
	const int nxt = cur ^ 1, rounds0 = total_rounds;
	const double t_g0 = T.ms();
	// time (q, 0) and the home in the new geometry, per old slot
	LAUNCH_NW_NOTAB(v, k_rp_rehash_init, grid(old_total), d_keys, d_sets, d_pre, p, tab[cur], d_time, d_home_slot);
	for (int s = 0; s < p; s++)                           // (only the regions of the sets that grow, at their new size: the early growths are tiny)
		if (sets[s].old_size) GCHK(hipMemsetAsync(tab[nxt] + sets[s].tab0, 0, (size_t)sets[s].size * 8, v.stream));
	GCHK(hipMemsetAsync(d_round, 0, sizeof(RpRound), v.stream));
	// round 0: everybody
	hipLaunchKernelGGL(k_rp_ins_all, grid(old_total), dim3(TPB), 0, v.stream, d_sets, d_pre, p, sch.qbits, tab[cur], tab[nxt], d_home_slot, d_time, d_round);
	hipLaunchKernelGGL(k_rp_eval_all, grid(old_total), dim3(TPB), 0, v.stream, d_sets, d_pre, p, sch.qbits, tab[cur], tab[nxt], d_home_slot, d_time,
	                   d_list[0], list_chunks, d_round);
	GCHK(hipGetLastError());
	// (SDT_RP_MAX_ROUNDS: test hook -- a cap that real data passes, so that the caller's other path is exercised)
	static const int max_rounds = sdt_test_env("SDT_RP_MAX_ROUNDS") ? atoi(sdt_test_env("SDT_RP_MAX_ROUNDS")) : 60;
	int lc = 0;
	for (int round = 0;; round++) {
		RpRound h_round;
		GCHK(hipMemcpyAsync(&h_round, d_round, sizeof(RpRound), hipMemcpyDeviceToHost, v.stream));
		GCHK(hipStreamSynchronize(v.stream));
		total_rounds++;
		if (h_round.flags) return fail(SDT_ELIMIT, "layout on the device: %s", (h_round.flags & 2u) ? "an insertion found no slot" :
		                               (h_round.flags & 4u) ? "an eviction chain or a stretch of slots past its field" : "the list of a round is full");
		if (!h_round.n_next) break;
		if (round >= max_rounds) return fail(SDT_ELIMIT, "layout on the device: a growth did not settle in %d rounds", max_rounds);
		// from the home of every changed entry to the end of its cluster: taken out, laid out again, the old slots in there evaluated again
		const unsigned long long n_list = h_round.n_next * AP_CH;
		GCHK(hipMemsetAsync(d_round, 0, sizeof(RpRound), v.stream));
		hipLaunchKernelGGL(k_rp_collect, grid(n_list), dim3(TPB), 0, v.stream, d_sets, tab[nxt], d_saved, d_list[lc], n_list, d_round);
		hipLaunchKernelGGL(k_rp_ins_list, grid(n_list), dim3(TPB), 0, v.stream, d_sets, d_pre, sch.qbits, tab[nxt], d_saved, d_home_slot, d_time, d_list[lc], n_list, d_round);
		hipLaunchKernelGGL(k_rp_eval_list, grid(n_list), dim3(TPB), 0, v.stream, d_sets, d_pre, sch.qbits, tab[cur], tab[nxt], d_home_slot, d_time,
		                   d_list[lc], n_list, d_list[lc ^ 1], list_chunks, d_round);
		GCHK(hipGetLastError());
		lc ^= 1;
	}
	const double t_g1 = T.ms();
	t_rehash += t_g1 - t_g0;
	if (T.on && old_total > (1u << 24)) fprintf(stderr, "[device]     growth %zu: %llu old slots, %d rounds, %.1f ms\n", gen, old_total, total_rounds - rounds0, t_g1 - t_g0);
	// the settled layout without its times is the table of this generation
	unsigned long long new_total = 0;
	for (int s = 0; s < p; s++) { pre[s] = new_total; new_total += has(s, gen) ? sets[s].size : 0; }
	pre[p] = new_total;
	// (sets without this generation keep their table: copy their region over unchanged)
	for (int s = 0; s < p; s++)
		if (!has(s, gen)) GCHK(hipMemcpyAsync(tab[nxt] + sets[s].tab0, tab[cur] + sets[s].tab0, (size_t)sets[s].size * 8, hipMemcpyDeviceToDevice, v.stream));
	rc = upload(sets); if (rc != SDT_OK) return rc;
	// slots of the sets that grew: pre counts only those (others have size 0 in the prefix)
	std::vector<RpSet> grown = sets;
	for (int s = 0; s < p; s++) if (!has(s, gen)) grown[s].size = 0;
	GCHK(hipMemcpy(d_sets, grown.data(), (size_t)p * sizeof(RpSet), hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_rp_slots, grid(new_total), dim3(TPB), 0, v.stream, d_sets, d_pre, p, 0, sch.qbits, tab[cur], tab[nxt], (uint32_t *)nullptr);
	GCHK(hipGetLastError());
	GCHK(hipStreamSynchronize(v.stream));
	cur = nxt;
	t_strip += T.ms() - t_g1;
	return SDT_OK;
}

// the puts of generation gen: ids [lo, hi) of every set that has one, into its table as it is
int Replay::put(size_t gen)
{
	const double t_p0 = T.ms();
	unsigned long long put_total = 0;
	for (int s = 0; s < p; s++) {
		sets[s].lo = has(s, gen) ? sch.gens[s][gen].lo : 0;
		sets[s].hi = has(s, gen) ? sch.gens[s][gen].hi : 0;
		if (has(s, gen)) sets[s].size = sch.gens[s][gen].size;
		pre[s] = put_total;
		put_total += sets[s].hi - sets[s].lo;
	}
	pre[p] = put_total;
	const int rc = upload(sets); if (rc != SDT_OK) return rc;
	unsigned int h_flags = 0;
	GCHK(hipMemsetAsync(d_flags, 0, 4, v.stream));
	LAUNCH_NW_NOTAB(v, k_rp_home, grid(put_total), d_keys, d_sets, d_pre, p, 0, d_home);
	hipLaunchKernelGGL(k_rp_put, grid(put_total), dim3(TPB), 0, v.stream, d_sets, d_pre, p, d_home, tab[cur], d_flags);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h_flags, d_flags, 4, hipMemcpyDeviceToHost, v.stream));
	GCHK(hipStreamSynchronize(v.stream));
	if (h_flags) return fail(SDT_ELIMIT, "layout on the device: a put found no slot");
	t_put += T.ms() - t_p0;
	return SDT_OK;
}

// the visiting order from the settled tables: the sets one after the other, every set's slots in order; *d_order[i] = rank of the node at
// visiting position i.  The buffers of the replay go as soon as they are not needed
int Replay::order(Scratch &S, bool wide, uint64_t n, uint64_t **d_order)
{
	unsigned long long slot_total = 0;
	for (int s = 0; s < p; s++) { sets[s].size = sch.gens[s].back().size; pre[s] = slot_total; slot_total += sets[s].size; }
	pre[p] = slot_total;
	int rc = upload(sets); if (rc != SDT_OK) return rc;
	// (the buffers of the replay that are free now make room for the flags and their prefix sum)
	for (void *q : {(void *)tab[cur ^ 1], (void *)d_time, (void *)d_home_slot, (void *)d_saved, (void *)d_list[0], (void *)d_list[1]}) (void)hipFree(S.release(q));
	uint32_t *d_occ;
	GCHK(S.alloc(&d_occ, (slot_total + 1) * 4)); GCHK(S.alloc(d_order, (n ? n : 1) * 8));
	hipLaunchKernelGGL(k_rp_slots, grid(slot_total), dim3(TPB), 0, v.stream, d_sets, d_pre, p, 1, sch.qbits, (const unsigned long long *)nullptr, tab[cur], d_occ);
	GCHK(hipGetLastError());
	rc = wide ? sdti::layout_order<Ix64>(v, d_sets, d_pre, p, tab[cur], d_occ, slot_total, *d_order)
	          : sdti::layout_order<Ix32>(v, d_sets, d_pre, p, tab[cur], d_occ, slot_total, *d_order);
	if (rc != SDT_OK) return rc;
	(void)hipFree(S.release(tab[cur])); (void)hipFree(S.release(d_occ)); (void)hipFree(S.release(d_home));
	return SDT_OK;
}

extern "C" {

// ---- layout ---------------------------------------------------------------------------------------------------------
int sdt_gpu_layout_on_device(sdt_ctx *c, int p, int nw_variant, int small_init, uint64_t *set_start, uint64_t *n_out)
{
	if (!c || !n_out || !set_start) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v0 = sdti::graph_view(c);
	GRAPH_ENTER(v0);
	const CallTimer T;
	int rc = sdti::release_pass1(c);
	if (rc != SDT_OK) return rc;
	T.tick("pass 1 released");
	const GraphView v = sdti::graph_view(c);
	const uint64_t n = v.h_stats->distinct;
	*n_out = n;
	rc = layout_check(v, p, nw_variant);
	if (rc != SDT_OK) return rc;
	sdti::GraphExt *gx = ext_of(v);
	rc = graph_choose_form(gx, n);                           // (the ranks of the numbering below: 32-bit below 2^32 - 16 nodes, else 64-bit)
	if (rc != SDT_OK) return rc;
	if (gx->d_sval) { (void)hipFree(gx->d_sval); gx->d_sval = nullptr; gx->n_sorted = 0; }
	Scratch S;
	SortedNodes sorted;
	rc = layout_sort(c, v, S, p, nw_variant, n, set_start, T, sorted);
	if (rc != SDT_OK) return rc;
	(void)hipFree(S.release(sorted.k1));                      // (the sorted sort keys are not needed any more)
	if (v.nw != 1) (void)hipFree(S.release(sorted.k0));
	(void)hipFree(S.release(sorted.v0s));
	// every set's growth schedule (a function of its number of keys only)
	std::vector<uint64_t> set_size(p);
	for (int s = 0; s < p; s++) set_size[s] = set_start[s + 1] - set_start[s];
	sdt::RpSchedule sch;
	const sdt::RpPlanStatus plan = sdt::rp_schedule(set_size.data(), p, nw_variant, small_init, sch);
	if (plan == sdt::RP_PLAN_SLOTS) return fail(SDT_EINVAL, "layout on the device: a set's table passes 2^32 slots");
	if (plan == sdt::RP_PLAN_BITS) return fail(SDT_ELIMIT, "layout on the device: twice %d slot bits do not fit the table word (or %d sets the list entry)", sch.qbits, p);
	T.tick("schedule made");
	Replay R(v, sch, T, p, set_start, sorted.d_keys);
	rc = R.alloc(S, n);
	if (rc != SDT_OK) return rc;
	T.tick("buffers made");
	const double t_start = T.ms();
	if (T.on) fprintf(stderr, "[device]     layout: release + sort + gather + schedule + buffers %.1f ms\n", t_start);
	for (size_t gen = 0; gen < sch.max_gens; gen++) {
		if (gen > 0) { rc = R.grow(gen); if (rc != SDT_OK) return rc; }
		rc = R.put(gen);
		if (rc != SDT_OK) return rc;
	}
	if (T.on) fprintf(stderr, "[device]     layout replay so far %.1f ms: rehash rounds %.1f, strip + copies %.1f, puts %.1f ms\n", T.ms() - t_start, R.t_rehash, R.t_strip, R.t_put);
	uint64_t *d_order;
	rc = R.order(S, gx->wide, n, &d_order);
	if (rc != SDT_OK) return rc;
	if (T.on) fprintf(stderr, "[device]     layout: order extracted at %.1f ms\n", T.ms());
	rc = layout_publish(c, v, S, sorted.v1s, d_order, nullptr, n, true, [&] {
		return fail(SDT_ESTATE, "layout on the device: %llu positions of the order are not ranks", (unsigned long long)v.h_stats->probe_fail);
	});
	if (rc != SDT_OK) return rc;
	if (T.on) fprintf(stderr, "[device]     layout: whole call %.1f ms\n[device]   layout replay: %zu generations, %d rounds of timed insertion in all, %llu table slots\n", T.ms(),
	                  sch.max_gens, R.total_rounds, (unsigned long long)sch.tab_total);
	return SDT_OK;
}

int sdt_gpu_layout_sorted_keys(sdt_ctx *c, int p, int nw_variant, uint64_t *keys, uint64_t max_nodes, uint64_t *set_start, uint64_t *n_out)
{
	if (!c || !n_out) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v0 = sdti::graph_view(c);
	GRAPH_ENTER(v0);
	int rc = sdti::release_pass1(c);                          // drains pass 1; its pools are not needed any more
	if (rc != SDT_OK) return rc;
	const GraphView v = sdti::graph_view(c);                  // (the drain may have grown the table)
	const uint64_t n = v.h_stats->distinct;
	*n_out = n;
	if (!keys && !set_start) return SDT_OK;
	if (!keys || !set_start) return fail(SDT_EINVAL, "NULL argument");
	rc = layout_check(v, p, nw_variant);
	if (rc != SDT_OK) return rc;
	if (max_nodes < n) return fail(SDT_EINVAL, "key array holds %llu nodes, the table has %llu", (unsigned long long)max_nodes, (unsigned long long)n);
	sdti::GraphExt *gx = ext_of(v);
	if (gx->d_sval) { (void)hipFree(gx->d_sval); gx->d_sval = nullptr; gx->n_sorted = 0; }
	Scratch S;
	SortedNodes sorted;
	rc = layout_sort(c, v, S, p, nw_variant, n, set_start, CallTimer(false), sorted);
	if (rc != SDT_OK) return rc;
	rc = sdti::d2h_big(v.copy_stream, keys, sorted.d_keys, n * v.nw * 8);
	if (rc != SDT_OK) return rc;
	gx->d_sval = (uint64_t *)S.release(sorted.v1s);
	gx->n_sorted = n;
	return SDT_OK;
}

int sdt_gpu_layout_apply(sdt_ctx *c, const uint64_t *order, uint64_t n)
{
	if (!c || (n && !order)) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->d_sval || gx->n_sorted != n) return fail(SDT_ESTATE, "call sdt_gpu_layout_sorted_keys first (it sorted %llu nodes, the order has %llu)", (unsigned long long)gx->n_sorted, (unsigned long long)n);
	GRAPH_ENTER(v);
	int rc = graph_choose_form(gx, n);
	if (rc != SDT_OK) return rc;
	Scratch S;
	rc = layout_publish(c, v, S, gx->d_sval, nullptr, order, n, false, [&] {
		return fail(SDT_EINVAL, "layout order: %llu entries are not ranks below %llu", (unsigned long long)v.h_stats->probe_fail, (unsigned long long)n);
	});
	if (rc != SDT_OK) return rc;
	(void)hipFree(gx->d_sval);
	gx->d_sval = nullptr;
	gx->n_sorted = 0;
	return SDT_OK;
}

int sdt_gpu_export_ordered(sdt_ctx *c, uint64_t *keys, uint32_t *l_links, uint32_t *r_flags, uint32_t *count, uint64_t n)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->d_slot_of || gx->n_nodes != n) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply first (it numbered %llu nodes, the arrays hold %llu)", (unsigned long long)gx->n_nodes, (unsigned long long)n);
	GRAPH_ENTER(v);
	// in pieces of 32 M nodes, double buffered: the kernel of piece k + 1 runs while piece k is on the link
	const uint64_t PIECE = (uint64_t)32 << 20;
	Scratch S;
	uint64_t *dk[2] = {};
	uint32_t *dl[2] = {}, *dr[2] = {}, *dc[2] = {};
	hipEvent_t ev[2] = {};
	for (int b = 0; b < 2; b++) {
		if (keys) GCHK(S.alloc(&dk[b], PIECE * v.nw * 8));
		if (l_links) GCHK(S.alloc(&dl[b], PIECE * 4));
		if (r_flags) GCHK(S.alloc(&dr[b], PIECE * 4));
		if (count) GCHK(S.alloc(&dc[b], PIECE * 4));
		GCHK(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
	}
	int rc = SDT_OK;
	uint64_t prev0 = 0, prevn = 0;
	int prevb = -1;
	for (uint64_t v0 = 0, k = 0; rc == SDT_OK && (v0 < n || prevb >= 0); v0 += PIECE, k++) {
		const int b = (int)(k & 1);
		const uint64_t cnt = v0 < n ? (n - v0 < PIECE ? n - v0 : PIECE) : 0;
		if (cnt) {
			LAUNCH_NW(v, k_export_ordered, sdti::scan_grid(v.cu_count, cnt), gx->d_slot_of, v0, cnt, dk[b], dl[b], dr[b], dc[b]);
			if (hipGetLastError() != hipSuccess || hipEventRecord(ev[b], v.stream) != hipSuccess) { rc = fail(SDT_EHIP, "export: launch failed"); break; }
		}
		if (prevb >= 0) {
			if (hipEventSynchronize(ev[prevb]) != hipSuccess) { rc = fail(SDT_EHIP, "export: event wait failed"); break; }
			if (keys && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, keys + prev0 * v.nw, dk[prevb], prevn * v.nw * 8);
			if (l_links && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, l_links + prev0, dl[prevb], prevn * 4);
			if (r_flags && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, r_flags + prev0, dr[prevb], prevn * 4);
			if (count && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, count + prev0, dc[prevb], prevn * 4);
		}
		prevb = cnt ? b : -1;
		prev0 = v0;
		prevn = cnt;
	}
	for (int b = 0; b < 2; b++) if (ev[b]) (void)hipEventDestroy(ev[b]);
	return rc;
}

int sdt_gpu_update_nodes_by_index(sdt_ctx *c, const uint64_t *node, const uint32_t *l_links, const uint32_t *r_flags, uint64_t n)
{
	if (!c || (n && (!node || !l_links || !r_flags))) return fail(SDT_EINVAL, "NULL argument");
	if (!n) return SDT_OK;
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->d_slot_of) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply first");
	GRAPH_ENTER(v);
	Scratch S;
	uint64_t *d_n;
	uint32_t *d_l, *d_r;
	GCHK(S.alloc(&d_n, n * 8)); GCHK(S.alloc(&d_l, n * 4)); GCHK(S.alloc(&d_r, n * 4));
	int rc = sdti::h2d_big(v.copy_stream, d_n, node, n * 8);
	if (rc == SDT_OK) rc = sdti::h2d_big(v.copy_stream, d_l, l_links, n * 4);
	if (rc == SDT_OK) rc = sdti::h2d_big(v.copy_stream, d_r, r_flags, n * 4);
	if (rc != SDT_OK) return rc;
	LAUNCH_NW(v, k_update_by_index, sdti::scan_grid(v.cu_count, n), gx->d_slot_of, gx->n_nodes, d_n, d_l, d_r, n, v.d_stats);
	GCHK(hipGetLastError());
	rc = sdti::sync_stats(c);
	if (rc != SDT_OK) return fail(SDT_EINVAL, "sdt_gpu_update_nodes_by_index: %llu indices past the last node", (unsigned long long)v.h_stats->probe_fail);
	return SDT_OK;
}

// ---- labelled dry runs, the minor-out commit, kmer2edges: entry points of the templates of sdt_graph_phases.hpp ------------
int sdt_gpu_tip_walks_labelled(sdt_ctx *c, int thin, int cut_len, uint64_t *n_records)
{
	if (!c || !n_records) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	if (!*v.d_idx || *v.idx_slots != v.slots) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply (or sdt_gpu_set_node_index) first");
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->wide && *v.idx_n >= 0xFFFFFFF0ULL) return fail(SDT_ESTATE, "%llu nodes numbered in the 32-bit form", (unsigned long long)*v.idx_n);
	GRAPH_ENTER(v);
	return gx->wide ? sdti::tip_walks_labelled(c, ix64_of(gx), thin, cut_len, n_records) : sdti::tip_walks_labelled(c, Ix32(), thin, cut_len, n_records);
}

int sdt_gpu_minor_out_labelled(sdt_ctx *c, double threshold, uint64_t *n_junctions, uint64_t *n_records)
{
	if (!c || !n_junctions || !n_records) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	if (!*v.d_idx || *v.idx_slots != v.slots) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply (or sdt_gpu_set_node_index) first");
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->wide && *v.idx_n >= 0xFFFFFFF0ULL) return fail(SDT_ESTATE, "%llu nodes numbered in the 32-bit form", (unsigned long long)*v.idx_n);
	GRAPH_ENTER(v);
	return gx->wide ? sdti::minor_out_labelled(c, ix64_of(gx), threshold, n_junctions, n_records) : sdti::minor_out_labelled(c, Ix32(), threshold, n_junctions, n_records);
}

// removeMinorOut's commit on the records sdt_gpu_minor_out_labelled left on the device (sdt_graph_phases.hpp; _finish below)
int sdt_gpu_minor_out_commit_begin(sdt_ctx *c, double threshold, uint64_t max_component, uint64_t *largest, uint64_t *n_skipped, uint64_t *n_skipped_records)
{
	if (!c || !largest || !n_skipped || !n_skipped_records) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->d_slot_of || !*v.d_idx || *v.idx_slots != v.slots || *v.idx_n != gx->n_nodes) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply first");
	if (!gx->d_result || gx->result_stride != 14) return fail(SDT_ESTATE, "call sdt_gpu_minor_out_labelled first (its records must still be on the device)");
	const uint64_t nn = gx->n_nodes, nr = gx->result_words / 14;
	if (nr >= 0xFFFFFFF0ULL) return fail(SDT_EINVAL, "commit on the device: 32-bit record indices, %llu records", (unsigned long long)nr);
	if (!gx->wide && nn >= 0xFFFFFFF0ULL) return fail(SDT_ESTATE, "%llu nodes numbered in the 32-bit form", (unsigned long long)nn);
	GRAPH_ENTER(v);
	return gx->wide ? sdti::minor_out_commit_begin(c, ix64_of(gx), threshold, max_component, largest, n_skipped, n_skipped_records)
	                : sdti::minor_out_commit_begin(c, Ix32(), threshold, max_component, largest, n_skipped, n_skipped_records);
}

int sdt_gpu_minor_out_commit_finish(sdt_ctx *c, uint64_t *off, uint64_t *linear, uint64_t *n_written)
{
	if (!c || !off || !linear || !n_written) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->mo_pending) return fail(SDT_ESTATE, "call sdt_gpu_minor_out_commit_begin first");
	GRAPH_ENTER(v);
	*off = *linear = *n_written = 0;
	const uint64_t nn = gx->n_nodes;
	unsigned long long h_cnt[5] = {0, 0, 0, 0, 0};
	GCHK(hipMemcpyAsync(h_cnt, gx->mo_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, v.stream));
	GCHK(hipStreamSynchronize(v.stream));
	if (h_cnt[1]) { sdti::mo_pending_free(gx); return fail(SDT_ESTATE, "sdt_gpu_minor_out_commit: %llu cuts found no record of the node they cut", h_cnt[1]); }
	const uint64_t nw = h_cnt[3];
	Scratch S;
	unsigned long long *d_cur;
	GCHK(S.alloc(&d_cur, 8));
	GCHK(hipMemsetAsync(d_cur, 0, 8, v.stream));
	uint64_t *wn; uint32_t *wl, *wr;
	GCHK(S.alloc(&wn, (nw + 1) * 8)); GCHK(S.alloc(&wl, (nw + 1) * 4)); GCHK(S.alloc(&wr, (nw + 1) * 4));
	if (nw) {
		LAUNCH_NW(v, k_mo_emit, sdti::scan_grid(v.cu_count, nn), gx->d_slot_of, nn, gx->mo_dirty, d_cur, nw, wn, wl, wr);
		GCHK(hipGetLastError());
	}
	GCHK(hipStreamSynchronize(v.stream));
	sdti::mo_pending_free(gx);
	gx->d_wnode = (uint64_t *)S.release(wn); gx->d_wl = (uint32_t *)S.release(wl); gx->d_wr = (uint32_t *)S.release(wr);
	gx->n_written = nw;
	*off = h_cnt[0];
	*linear = h_cnt[2];
	*n_written = nw;
	return SDT_OK;
}

int sdt_gpu_minor_out_commit(sdt_ctx *c, double threshold, uint64_t max_component, uint64_t *largest, uint64_t *off, uint64_t *linear, uint64_t *n_written,
                             uint64_t *n_skipped, uint64_t *n_skipped_records)
{
	if (!off || !linear || !n_written) return fail(SDT_EINVAL, "NULL argument");
	const int rc = sdt_gpu_minor_out_commit_begin(c, threshold, max_component, largest, n_skipped, n_skipped_records);
	return rc != SDT_OK ? rc : sdt_gpu_minor_out_commit_finish(c, off, linear, n_written);
}

int sdt_gpu_fetch_skipped(sdt_ctx *c, uint64_t *dst, uint64_t n_records)
{
	if (!c || (n_records && !dst)) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (n_records != gx->n_skipped) return fail(SDT_EINVAL, "the last commit left %llu records to the host, asked for %llu", (unsigned long long)gx->n_skipped, (unsigned long long)n_records);
	GRAPH_ENTER(v);
	int rc = SDT_OK;
	if (n_records) rc = sdti::d2h_big(v.copy_stream, dst, gx->d_skipped, n_records * 14 * 8);
	if (rc == SDT_OK && gx->base) rebase_records(dst, n_records, 14, gx->base);
	// (no hipFree here: freeing waits for the device, and the visits of _begin may be running -- _begin / the context let go of it)
	return rc;
}

int sdt_gpu_fetch_written(sdt_ctx *c, uint64_t *node, uint32_t *l_links, uint32_t *r_flags, uint64_t n)
{
	if (!c || (n && (!node || !l_links || !r_flags))) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (n != gx->n_written) return fail(SDT_EINVAL, "the last commit wrote %llu nodes, asked for %llu", (unsigned long long)gx->n_written, (unsigned long long)n);
	GRAPH_ENTER(v);
	int rc = SDT_OK;
	if (n) rc = sdti::d2h_big(v.copy_stream, node, gx->d_wnode, n * 8);
	if (n && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, l_links, gx->d_wl, n * 4);
	if (n && rc == SDT_OK) rc = sdti::d2h_big(v.copy_stream, r_flags, gx->d_wr, n * 4);
	if (gx->d_wnode) (void)hipFree(gx->d_wnode);
	if (gx->d_wl) (void)hipFree(gx->d_wl);
	if (gx->d_wr) (void)hipFree(gx->d_wr);
	gx->d_wnode = nullptr; gx->d_wl = gx->d_wr = nullptr;
	gx->n_written = 0;
	return rc;
}

// ---- kmer2edges on the device (node2edge.c:46-561; sdt_graph_phases.hpp) ------------------------------------------------
int sdt_gpu_build_edges(sdt_ctx *c, uint64_t *n_edges, uint64_t *num_ed, uint64_t *n_bases)
{
	if (!c || !n_edges || !num_ed || !n_bases) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (!gx->d_slot_of || !*v.d_idx || *v.idx_slots != v.slots || *v.idx_n != gx->n_nodes) return fail(SDT_ESTATE, "call sdt_gpu_layout_apply first");
	if (!gx->wide && gx->n_nodes >= 0xFFFFFFF0ULL) return fail(SDT_ESTATE, "%llu nodes numbered in the 32-bit form", (unsigned long long)gx->n_nodes);
	GRAPH_ENTER(v);
	return gx->wide ? sdti::build_edges(c, ix64_of(gx), n_edges, num_ed, n_bases) : sdti::build_edges(c, Ix32(), n_edges, num_ed, n_bases);
}

int sdt_gpu_fetch_edge_bases(sdt_ctx *c, char *dst, uint64_t nbytes)
{
	if (!c || (nbytes && !dst)) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (nbytes != gx->seq_bytes) return fail(SDT_EINVAL, "the edges have %llu bases, asked for %llu", (unsigned long long)gx->seq_bytes, (unsigned long long)nbytes);
	GRAPH_ENTER(v);
	int rc = SDT_OK;
	if (nbytes) rc = sdti::d2h_big(v.copy_stream, dst, gx->d_seq, nbytes);
	if (gx->d_seq) (void)hipFree(gx->d_seq);
	gx->d_seq = nullptr;
	gx->seq_bytes = 0;
	return rc;
}

int sdt_gpu_fetch_records(sdt_ctx *c, uint64_t *dst, uint64_t nwords)
{
	if (!c || (nwords && !dst)) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	if (nwords != gx->result_words) return fail(SDT_EINVAL, "the last dry run left %llu words, asked for %llu", (unsigned long long)gx->result_words, (unsigned long long)nwords);
	GRAPH_ENTER(v);
	int rc = SDT_OK;
	if (nwords) rc = sdti::d2h_big(v.copy_stream, dst, gx->d_result, nwords * 8);
	if (rc == SDT_OK && gx->result_nodes && gx->base) rebase_records(dst, nwords / gx->result_stride, gx->result_stride, gx->base);
	if (gx->d_result) (void)hipFree(gx->d_result);
	gx->d_result = nullptr;
	gx->result_words = 0;
	return rc;
}

// ---- graph-cleaning dry runs on the device mirror of the host graph, indexed by host position ---------------------------------
static int upload_keys(const GraphView &v, Scratch &S, const uint64_t *keys, uint64_t n, uint64_t **d_k)
{
	GCHK(S.alloc(d_k, (n ? n : 1) * v.nw * sizeof(uint64_t)));
	return sdti::h2d_big(v.copy_stream, *d_k, keys, n * v.nw * sizeof(uint64_t));
}

int sdt_gpu_set_node_index(sdt_ctx *c, const uint64_t *keys, uint64_t n)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	if (n && !keys) return fail(SDT_EINVAL, "NULL argument");
	GRAPH_ENTER(v);
	GCHK(hipStreamSynchronize(v.stream));
	if (*v.d_idx) GCHK(hipFree(*v.d_idx));
	*v.d_idx = nullptr;
	*v.idx_slots = *v.idx_n = 0;
	GCHK(hipMalloc(v.d_idx, v.slots * sizeof(uint64_t)));
	GCHK(hipMemsetAsync(*v.d_idx, 0xFF, v.slots * sizeof(uint64_t), v.stream));
	sdti::GraphExt *gx = ext_of(v);
	int rc = graph_choose_form(gx, n);
	if (rc != SDT_OK) return rc;
	Scratch S;
	uint64_t *d_k;
	rc = upload_keys(v, S, keys, n, &d_k);
	if (rc != SDT_OK) return rc;
	rc = gx->wide ? sdti::set_index(v, ix64_of(gx), d_k, n) : sdti::set_index(v, Ix32(), d_k, n);
	if (rc != SDT_OK || sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_set_node_index: %llu nodes are not in the table", (unsigned long long)v.h_stats->probe_fail);
	*v.idx_slots = v.slots;
	*v.idx_n = n;
	return SDT_OK;
}

int sdt_gpu_update_nodes(sdt_ctx *c, const uint64_t *keys, const uint32_t *l_links, const uint32_t *r_flags, uint64_t n)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	if (n && (!keys || !l_links || !r_flags)) return fail(SDT_EINVAL, "NULL argument");
	if (!n) return SDT_OK;
	GRAPH_ENTER(v);
	Scratch S;
	uint64_t *d_k;
	uint32_t *d_l, *d_r;
	const int rc = upload_keys(v, S, keys, n, &d_k);
	if (rc != SDT_OK) return rc;
	GCHK(S.alloc(&d_l, n * 4)); GCHK(S.alloc(&d_r, n * 4));
	GCHK(hipMemcpyAsync(d_l, l_links, n * 4, hipMemcpyHostToDevice, v.stream));
	GCHK(hipMemcpyAsync(d_r, r_flags, n * 4, hipMemcpyHostToDevice, v.stream));
	LAUNCH_NW(v, k_update_nodes, sdti::scan_grid(v.cu_count, n), d_k, d_l, d_r, n, v.d_stats);
	GCHK(hipGetLastError());
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_update_nodes: %llu nodes are not in the table", (unsigned long long)v.h_stats->probe_fail);
	return SDT_OK;
}

// what the dry runs by host position ask of the context: no node base, a node index (`bad` = the call has a NULL argument)
static int dry_run_check(const GraphView &v, const char *who, bool bad)
{
	if (ext_of(v)->base) return fail(SDT_ESTATE, "%s reads host positions straight from the node index: no node base (SDT_NODE_BASE)", who);
	if (bad) return fail(SDT_EINVAL, "NULL argument");
	if (!*v.d_idx || *v.idx_slots != v.slots) return fail(SDT_ESTATE, "call sdt_gpu_set_node_index first");
	return SDT_OK;
}

int sdt_gpu_tip_walks(sdt_ctx *c, int thin, int cut_len, uint64_t *end_idx, uint8_t *info, uint64_t n)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	const int rc = dry_run_check(v, "sdt_gpu_tip_walks", !end_idx || !info);
	if (rc != SDT_OK) return rc;
	if (n != *v.idx_n)
		return fail(SDT_EINVAL, "the node index holds %llu nodes, the output arrays %llu", (unsigned long long)*v.idx_n, (unsigned long long)n);
	GRAPH_ENTER(v);
	Scratch S;
	uint64_t *d_e;
	uint8_t *d_i;
	GCHK(S.alloc(&d_e, (n ? n : 1) * sizeof(uint64_t))); GCHK(S.alloc(&d_i, n ? n : 1));
	LAUNCH_NW(v, k_tip_walks, sdti::scan_grid(v.cu_count, v.slots), *v.d_idx, v.K, thin, cut_len, d_e, d_i, v.d_stats, (uint64_t *)nullptr, 0ULL, (unsigned long long *)nullptr, 2);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(end_idx, d_e, n * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream));
	GCHK(hipMemcpyAsync(info, d_i, n, hipMemcpyDeviceToHost, v.stream));
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_tip_walks: %llu walks left the graph (a link points at a k-mer that is not a node)", (unsigned long long)v.h_stats->probe_fail);
	return SDT_OK;
}

int sdt_gpu_minor_out_dry(sdt_ctx *c, double threshold, uint64_t *records, uint64_t max_records, uint64_t *n_junctions, uint64_t *n_records)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	const int rc = dry_run_check(v, "sdt_gpu_minor_out_dry", (!records && max_records) || !n_junctions || !n_records);
	if (rc != SDT_OK) return rc;
	GRAPH_ENTER(v);
	Scratch S;
	uint8_t *d_need, *d_flag;
	uint64_t *d_rec;
	unsigned long long *d_cur, h1 = 0, h2 = 0;
	const uint64_t n = *v.idx_n ? *v.idx_n : 1, m = max_records ? max_records : 1;
	GCHK(S.alloc(&d_need, n)); GCHK(S.alloc(&d_flag, n)); GCHK(S.alloc(&d_rec, m * 9 * sizeof(uint64_t))); GCHK(S.alloc(&d_cur, sizeof(unsigned long long)));
	GCHK(hipMemsetAsync(d_need, 0, n, v.stream));
	GCHK(hipMemsetAsync(d_flag, 0, n, v.stream));
	GCHK(hipMemsetAsync(d_cur, 0, sizeof(unsigned long long), v.stream));
	const int g = sdti::scan_grid(v.cu_count, v.slots);
	LAUNCH_NW(v, k_minor_out_junctions, g, *v.d_idx, v.K, threshold, d_need, d_flag, d_rec, (unsigned long long)max_records, d_cur, v.d_stats, 9);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h1, d_cur, sizeof h1, hipMemcpyDeviceToHost, v.stream));
	LAUNCH_NW(v, k_minor_out_candidates, g, *v.d_idx, v.K, d_need, d_flag, d_rec, (unsigned long long)max_records, d_cur, v.d_stats, 9);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h2, d_cur, sizeof h2, hipMemcpyDeviceToHost, v.stream));
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_minor_out_dry: %llu links point at k-mers that are not nodes", (unsigned long long)v.h_stats->probe_fail);
	*n_junctions = h1;
	*n_records = h2;
	if (h2 > max_records) return fail(SDT_EFULL, "record array holds %llu, the pass needs %llu", (unsigned long long)max_records, h2);
	if (h2) GCHK(hipMemcpy(records, d_rec, h2 * 9 * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return SDT_OK;
}

int sdt_gpu_edge_ports(sdt_ctx *c, uint64_t *records, uint64_t max_records, uint64_t *n_records)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	const int rc = dry_run_check(v, "sdt_gpu_edge_ports", (!records && max_records) || !n_records);
	if (rc != SDT_OK) return rc;
	GRAPH_ENTER(v);
	Scratch S;
	uint64_t *d_rec;
	unsigned long long *d_cur, h = 0;
	GCHK(S.alloc(&d_rec, (max_records ? max_records : 1) * 17 * sizeof(uint64_t))); GCHK(S.alloc(&d_cur, sizeof(unsigned long long)));
	GCHK(hipMemsetAsync(d_cur, 0, sizeof(unsigned long long), v.stream));
	LAUNCH_NW(v, k_edge_ports, sdti::scan_grid(v.cu_count, v.slots), *v.d_idx, v.K, *v.idx_n + 1, d_rec, (unsigned long long)max_records, d_cur, v.d_stats);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h, d_cur, sizeof h, hipMemcpyDeviceToHost, v.stream));
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_edge_ports: %llu chains leave the graph or never end", (unsigned long long)v.h_stats->probe_fail);
	*n_records = h;
	if (h > max_records) return fail(SDT_EFULL, "record array holds %llu, the graph has %llu non-linear nodes", (unsigned long long)max_records, h);
	if (h) GCHK(hipMemcpy(records, d_rec, h * 17 * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return SDT_OK;
}

int sdt_gpu_tip_walks_compact(sdt_ctx *c, int thin, int cut_len, uint64_t *records, uint64_t max_records, uint64_t *n_records)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	const int rc = dry_run_check(v, "sdt_gpu_tip_walks_compact", (!records && max_records) || !n_records);
	if (rc != SDT_OK) return rc;
	if (*v.idx_n >= (1ULL << 56)) return fail(SDT_EINVAL, "node indices do not fit 56 bits");
	GRAPH_ENTER(v);
	Scratch S;
	uint64_t *d_rec;
	unsigned long long *d_cur, h = 0;
	GCHK(S.alloc(&d_rec, (max_records ? max_records : 1) * 2 * sizeof(uint64_t))); GCHK(S.alloc(&d_cur, sizeof(unsigned long long)));
	GCHK(hipMemsetAsync(d_cur, 0, sizeof(unsigned long long), v.stream));
	LAUNCH_NW(v, k_tip_walks, sdti::scan_grid(v.cu_count, v.slots), *v.d_idx, v.K, thin, cut_len, (uint64_t *)nullptr, (uint8_t *)nullptr, v.d_stats, d_rec,
	          (unsigned long long)max_records, d_cur, 2);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h, d_cur, sizeof h, hipMemcpyDeviceToHost, v.stream));
	if (sdti::sync_stats(c) != SDT_OK)
		return fail(SDT_ESTATE, "sdt_gpu_tip_walks_compact: %llu walks left the graph", (unsigned long long)v.h_stats->probe_fail);
	*n_records = h;
	if (h > max_records) return fail(SDT_EFULL, "record array holds %llu, %llu nodes have a walk", (unsigned long long)max_records, h);
	if (h) GCHK(hipMemcpy(records, d_rec, h * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return SDT_OK;
}

}  // extern "C"

// the host's look-up index with entries E (32- or 64-bit), built on the device in the form of the numbering and copied to `index`
template <class E>
static int host_index_entries(const GraphView &v, E *index, uint64_t index_slots)
{
	sdti::GraphExt *gx = ext_of(v);
	Scratch S;
	E *d_index;
	GCHK(S.alloc(&d_index, index_slots * sizeof(E)));
	GCHK(hipMemsetAsync(d_index, 0, index_slots * sizeof(E), v.stream));
	const int rc = gx->wide ? sdti::host_index(v, ix64_of(gx), d_index, index_slots - 1) : sdti::host_index(v, Ix32(), d_index, index_slots - 1);
	if (rc != SDT_OK) return rc;
	GCHK(hipStreamSynchronize(v.stream));
	return sdti::d2h_big(v.copy_stream, index, d_index, index_slots * sizeof(E));      // (pageable destination of gigabytes: staged copies)
}

extern "C" {

int sdt_gpu_build_host_index(sdt_ctx *c, uint32_t *index, uint64_t index_slots)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view(c);
	if (!index) return fail(SDT_EINVAL, "NULL argument");
	if (!*v.d_idx || *v.idx_slots != v.slots) return fail(SDT_ESTATE, "call sdt_gpu_set_node_index first");
	if (index_slots < 2 * *v.idx_n || (index_slots & (index_slots - 1))) return fail(SDT_EINVAL, "index_slots must be a power of two >= 2 x nodes");
	if (*v.idx_n >= 0xFFFFFFFEULL) return fail(SDT_EINVAL, "%llu nodes do not fit 32-bit index entries", (unsigned long long)*v.idx_n);
	GRAPH_ENTER(v);
	return host_index_entries<unsigned int>(v, index, index_slots);
}

int sdt_gpu_build_host_index64(sdt_ctx *c, uint64_t *index, uint64_t index_slots)
{
	if (!c || !index) return fail(SDT_EINVAL, "NULL argument");
	const GraphView v = sdti::graph_view(c);
	if (!*v.d_idx || *v.idx_slots != v.slots) return fail(SDT_ESTATE, "call sdt_gpu_set_node_index first");
	if (index_slots < 2 * *v.idx_n || (index_slots & (index_slots - 1))) return fail(SDT_EINVAL, "index_slots must be a power of two >= 2 x nodes");
	GRAPH_ENTER(v);
	return host_index_entries<unsigned long long>(v, (unsigned long long *)index, index_slots);
}

int sdt_gpu_set_graph_index_bits(sdt_ctx *c, int bits)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	if (bits != 0 && bits != 64) return fail(SDT_EINVAL, "graph index bits: 0 (by node count) or 64, asked for %d", bits);
	ext_of(sdti::graph_view(c))->want_bits = bits;
	return SDT_OK;
}

int sdt_gpu_graph_index_bits(const sdt_ctx *c)
{
	if (!c) return fail(SDT_EINVAL, "ctx is NULL");
	const GraphView v = sdti::graph_view((sdt_ctx *)c);
	const sdti::GraphExt *gx = ext_of(v);
	if (*v.d_idx) return gx->wide ? 64 : 32;                  // (numbered: the form of that numbering; before: the one asked for)
	return gx->want_bits == 64 ? 64 : 32;
}

}  // extern "C"
