// sdt_unitig.hip -- the unitigs of the counted k-mer graph and their links (the rule: include/sdt_gpu.h).  unitigs_begin = k_ug_starts (the
// first words of the chains, listed), k_ug_walk (one lane per start; the record from the end with x0 <= revcomp(last)), where the chains
// do not cover the live nodes k_ug_mark and k_ug_cycles, a radix sort of the records by x0, k_ug_permute, and the second order by
// revcomp(last) that unitigs_links searches (sdt_unitig_kernels.cuh); unitigs_seqs walks the requested chains again.  Nothing here writes
// the table, the kept reads or a cache of the context.  What the context keeps from unitigs_begin to unitigs_end is the sorted list -- N
// records and their two words each -- and that second order, and nothing per table slot; it is tied to the state of the table it was found
// on as the bubble list is (search_cache_drop, delow, the graph phases mark it stale).  State rules are those of the read stages.
// (sdt_thread.hip adds its index to this state when asked: 8 B per slot, freed where the list is.)
#include "sdt_readstage.hpp"
#include "sdt_unitig_kernels.cuh"
#include <rocprim/rocprim.hpp>
#include <cstddef>
#include <utility>

static_assert(sizeof(sdt_unitig) == sizeof(Unitig) && offsetof(sdt_unitig, nodes) == 8 && offsetof(sdt_unitig, info) == 20, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_unitig_link) == sizeof(UnitigLink) && offsetof(sdt_unitig_link, info) == 8, "include/sdt_gpu.h and the kernel agree");

static int unitigs_open(const sdt_ctx *c, const char *what)
{
	if (!c->ug.open)
		return fail(SDT_ESTATE, "%s: no unitig list: call sdt_gpu_unitigs_begin first", what);
	if (c->ug.stale || c->ug.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_unitigs_begin", what);
	return SDT_OK;
}

static void unitigs_free(sdt_ctx *c)
{
	if (c->ug.keys) (void)hipFree(c->ug.keys);
	if (c->ug.rec) (void)hipFree(c->ug.rec);
	if (c->ug.idx_keys) (void)hipFree(c->ug.idx_keys);
	if (c->ug.idx_id) (void)hipFree(c->ug.idx_id);
	if (c->ug.lab) (void)hipFree(c->ug.lab);                 // (the index of sdt_thread.hip goes with the list)
	if (c->ug.sup) (void)hipFree(c->ug.sup);                 // (... and the tally of sdt_support.hip)
	c->ug = sdt_ctx::Unitigs();
}

static int unitig_params_ok(const sdt_unitig_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_unitig_params is NULL");
	if (p->flags)
		return fail(SDT_EINVAL, "sdt_unitig_params.flags = 0x%x: no flag is defined", p->flags);
	if (p->min_link < 1 || p->min_link > 63)
		return fail(SDT_EINVAL, "sdt_unitig_params.min_link = %u: 1 to 63 (a link counter saturates at 63)", p->min_link);
	const uint32_t mc = p->min_count > 1 ? p->min_count : 1u;
	if (p->max_count && p->max_count < mc)
		return fail(SDT_EINVAL, "sdt_unitig_params.max_count = %u is below min_count = %u: 0 (no upper bound) or at least that", p->max_count, mc);
	return SDT_OK;
}

static ClusterRule rule_of(const sdt_ctx *c) { return ClusterRule{c->ug.min_count, c->ug.max_count, c->ug.min_link}; }

// the n records of `stride` words in src put in the order of their first nw words: stable passes from the last word; *sorted: the order
static int sort_by_words(sdt_ctx *c, const uint64_t *src, int stride, uint64_t n, DevBuf &o_a, DevBuf &o_b, DevBuf &k_a, DevBuf &k_b, uint32_t **sorted)
{
	size_t tb = 0;
	HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, (uint64_t *)k_a.p, (uint64_t *)k_b.p, (uint32_t *)o_a.p, (uint32_t *)o_b.p, (size_t)n, 0, 64, c->stream));
	DevBuf d_tmp;
	int rc = d_tmp.get(tb, "sdt_gpu_unitigs_begin: sort");
	if (rc != SDT_OK) return rc;
	uint32_t *in = (uint32_t *)o_a.p, *out = (uint32_t *)o_b.p;
	const int g = scan_grid(c, n);
	hipLaunchKernelGGL(k_bb_iota, dim3(g), dim3(TPB), 0, c->stream, in, n);
	hipError_t e = hipGetLastError();
	for (int w = c->nw - 1; w >= 0 && e == hipSuccess; w--) {
		hipLaunchKernelGGL(k_ug_sortkey, dim3(g), dim3(TPB), 0, c->stream, src, stride, (const uint32_t *)in, n, w, (uint64_t *)k_a.p);
		e = hipGetLastError();
		if (e == hipSuccess)
			e = rocprim::radix_sort_pairs(d_tmp.p, tb, (uint64_t *)k_a.p, (uint64_t *)k_b.p, in, out, (size_t)n, 0, 64, c->stream);
		uint32_t *t = in; in = out; out = t;
	}
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (the scratch goes when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	*sorted = in;
	return SDT_OK;
}

// the counters, read back; waits
static int read_counters(sdt_ctx *c, const unsigned long long *ctr, unsigned long long h[UG_COUNTERS])
{
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, UG_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);
	HIPCHK(e);
	HIPCHK(e2);
	if (h[UG_TOO_LONG])
		return fail(SDT_ELIMIT, "sdt_gpu_unitigs_begin: a unitig of 2^32 nodes or more: sdt_unitig.nodes is 32-bit");
	if (h[UG_BROKEN])
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_begin: %llu chains do not walk twice alike", h[UG_BROKEN]);
	return SDT_OK;
}

// checked arguments, the context entered, no list held; on failure the caller frees what is in c->ug
static int unitigs_build(sdt_ctx *c, const ClusterRule &rule, uint64_t info[8])
{
	const uint64_t slots = c->slots;
	const int stride = 2 * c->nw + UG_REC_WORDS;
	DevBuf d_ctr, d_list, d_cur, d_raw, d_oa, d_ob, d_ka, d_kb;
	int rc = d_ctr.get(UG_COUNTERS * sizeof(unsigned long long), "sdt_gpu_unitigs_begin: counters");
	if (rc == SDT_OK) rc = d_cur.get(sizeof(unsigned long long), "sdt_gpu_unitigs_begin: counters");
	if (rc != SDT_OK) return rc;
	unsigned long long *ctr = (unsigned long long *)d_ctr.p, h[UG_COUNTERS] = {}, n_chunks = 0;
	const int g = scan_grid(c, slots);
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	// the start words: a first guess of one per 16 slots, and once more with the chunks that were asked for when they did not fit
	uint64_t cap_chunks = (slots / 16 + 4096) / (AP_CH - 64) + 1 + (uint64_t)g * (TPB / 64);
	for (int attempt = 0;; attempt++) {
		rc = d_list.get(cap_chunks * AP_CH * sizeof(unsigned long long), "sdt_gpu_unitigs_begin: the list of start words");
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemsetAsync(ctr, 0, UG_COUNTERS * sizeof(unsigned long long), c->stream));
		HIPCHK(hipMemsetAsync(d_cur.p, 0, sizeof(unsigned long long), c->stream));
		const ApOut ap = {(unsigned long long *)d_cur.p, cap_chunks, nullptr, (unsigned long long *)d_list.p};
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_ug_starts<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (unsigned long long *)d_list.p, ap, ctr);
		});
		hipError_t e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(&n_chunks, d_cur.p, sizeof n_chunks, hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = hipStreamSynchronize(c->stream);   // (the buffers go when this returns)
		HIPCHK(e);
		HIPCHK(e2);
		if (n_chunks <= cap_chunks) break;
		if (attempt)
			return fail(SDT_ESTATE, "sdt_gpu_unitigs_begin: the number of start words changed between two scans");
		cap_chunks = n_chunks;
	}
	const uint64_t n_live = h[UG_N_LIVE], n_starts = h[UG_N_STARTS], n_list = n_chunks * AP_CH;
	// the walks: a chain has two start words and gives one record (a palindromic single word has one: never more records than starts)
	uint64_t cap = n_starts, n = 0;
	if (n_starts) {
		rc = d_raw.get(cap * stride * sizeof(uint64_t), "sdt_gpu_unitigs_begin: the unitigs as they are found, one per start word at the most");
		if (rc != SDT_OK) return rc;
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_ug_walk<NW>, dim3(scan_grid(c, n_list)), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const unsigned long long *)d_list.p,
			                   (unsigned long long)n_list, (uint64_t *)d_raw.p, (unsigned long long)cap, ctr);
		});
		rc = read_counters(c, ctr, h);
		if (rc != SDT_OK) return rc;
		n = h[UG_N_REC];
		if (n > cap)
			return fail(SDT_ESTATE, "sdt_gpu_unitigs_begin: %llu unitigs from %llu start words", (unsigned long long)n, (unsigned long long)n_starts);
	}
	if (h[UG_NODES] < n_live) {
		// live nodes that no chain holds lie on cycles (two nodes at the least each): a bit per slot says which they are
		const uint64_t n_lin = n, left = n_live - h[UG_NODES];
		DevBuf d_bits, d_more;
		cap = n_lin + left / 2;
		rc = d_bits.get((slots + 31) / 32 * sizeof(uint32_t), "sdt_gpu_unitigs_begin: one bit per table slot for the nodes on cycles");
		if (rc == SDT_OK) rc = d_more.get(cap * stride * sizeof(uint64_t), "sdt_gpu_unitigs_begin: the unitigs as they are found, with the cycles");
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemsetAsync(d_bits.p, 0, (slots + 31) / 32 * sizeof(uint32_t), c->stream));
		if (n_lin) HIPCHK(hipMemcpyAsync(d_more.p, d_raw.p, n_lin * stride * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			if (n_lin)
				hipLaunchKernelGGL(k_ug_mark<NW>, dim3(scan_grid(c, n_lin)), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint64_t *)d_more.p, n_lin,
				                   (uint32_t *)d_bits.p, ctr);
			hipLaunchKernelGGL(k_ug_cycles<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint32_t *)d_bits.p, (uint64_t *)d_more.p,
			                   (unsigned long long)cap, ctr);
		});
		rc = read_counters(c, ctr, h);                           // (the bits go when this returns)
		if (rc != SDT_OK) return rc;
		n = h[UG_N_REC];
		if (n > cap)
			return fail(SDT_ESTATE, "sdt_gpu_unitigs_begin: %llu unitigs, %llu of them cycles, from %llu nodes on cycles", (unsigned long long)n,
			            (unsigned long long)(n - n_lin), (unsigned long long)left);
		std::swap(d_raw.p, d_more.p);
		std::swap(d_raw.cap, d_more.cap);
	}
	if (h[UG_NODES] != n_live)
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_begin: the unitigs hold %llu nodes, the table has %llu live ones", h[UG_NODES], (unsigned long long)n_live);
	if (n > 0xFFFFFFFFULL)
		return fail(SDT_ELIMIT, "sdt_gpu_unitigs_begin: %llu unitigs: the sort's indices and the ids of a link are 32-bit", (unsigned long long)n);
	if (n) {
		const size_t kb = (size_t)c->nw * sizeof(uint64_t);
		DevBuf d_rl;
		rc = d_oa.get(n * sizeof(uint32_t), "sdt_gpu_unitigs_begin: sort order");
		if (rc == SDT_OK) rc = d_ob.get(n * sizeof(uint32_t), "sdt_gpu_unitigs_begin: sort order");
		if (rc == SDT_OK) rc = d_ka.get(n * sizeof(uint64_t), "sdt_gpu_unitigs_begin: sort keys");
		if (rc == SDT_OK) rc = d_kb.get(n * sizeof(uint64_t), "sdt_gpu_unitigs_begin: sort keys");
		if (rc == SDT_OK) rc = d_rl.get(n * kb, "sdt_gpu_unitigs_begin: the last words, reverse-complemented");
		if (rc != SDT_OK) return rc;
		hipError_t e = hipMalloc((void **)&c->ug.keys, n * 2 * kb);
		if (e != hipSuccess) c->ug.keys = nullptr;
		if (e == hipSuccess && (e = hipMalloc(&c->ug.rec, n * sizeof(Unitig))) != hipSuccess) c->ug.rec = nullptr;
		if (e == hipSuccess && (e = hipMalloc((void **)&c->ug.idx_keys, n * kb)) != hipSuccess) c->ug.idx_keys = nullptr;
		if (e == hipSuccess && (e = hipMalloc((void **)&c->ug.idx_id, n * sizeof(uint32_t))) != hipSuccess) c->ug.idx_id = nullptr;
		if (e != hipSuccess)
			return fail(SDT_ENOMEM, "the unitig list: %llu records of %zu bytes: %s", (unsigned long long)n, sizeof(Unitig) + 3 * kb + sizeof(uint32_t), hipGetErrorString(e));
		uint32_t *sorted = nullptr;
		rc = sort_by_words(c, (const uint64_t *)d_raw.p, stride, n, d_oa, d_ob, d_ka, d_kb, &sorted);
		if (rc != SDT_OK) return rc;
		const int gn = scan_grid(c, n);
		hipLaunchKernelGGL(k_ug_permute, dim3(gn), dim3(TPB), 0, c->stream, (const uint64_t *)d_raw.p, stride, c->nw, c->K, (const uint32_t *)sorted, n, c->ug.keys,
		                   (Unitig *)c->ug.rec, ctr);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_ug_rlast<NW>, dim3(gn), dim3(TPB), 0, c->stream, (const uint64_t *)c->ug.keys, n, c->K, (uint64_t *)d_rl.p);
		});
		HIPCHK(hipGetLastError());
		rc = sort_by_words(c, (const uint64_t *)d_rl.p, c->nw, n, d_oa, d_ob, d_ka, d_kb, &sorted);
		if (rc != SDT_OK) return rc;
		hipLaunchKernelGGL(k_ug_gather, dim3(gn), dim3(TPB), 0, c->stream, (const uint64_t *)d_rl.p, c->nw, (const uint32_t *)sorted, n, c->ug.idx_keys, c->ug.idx_id);
		rc = read_counters(c, ctr, h);
		if (rc != SDT_OK) return rc;
	}
	c->ug.n = n;
	c->ug.live = n_live;
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = slots;                                   // (slots scanned, not k-mers)
	}
	if (info) {
		const uint64_t out[8] = {n_live, n_starts, n, h[UG_N_CIRC], h[UG_NODES], h[UG_SEQ_BYTES], h[UG_LONGEST], 0};
		memcpy(info, out, sizeof out);
	}
	return SDT_OK;
}

static int range_ok(const sdt_ctx *c, const char *what, uint64_t first, uint64_t n)
{
	if (first > c->ug.n || n > c->ug.n - first)
		return fail(SDT_EINVAL, "%s: unitigs %llu .. %llu of %llu", what, (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)c->ug.n);
	return SDT_OK;
}

extern "C" {

int sdt_gpu_unitigs_begin(sdt_ctx *c, const sdt_unitig_params *params, uint64_t info[8])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	int rc = unitig_params_ok(params);
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_begin");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	unitigs_free(c);                                         // (a second begin replaces the first)
	c->ug.min_count = params->min_count > 1 ? params->min_count : 1u;
	c->ug.max_count = params->max_count;
	c->ug.min_link = params->min_link;
	rc = unitigs_build(c, rule_of(c), info);
	if (rc != SDT_OK) {
		(void)hipStreamSynchronize(c->stream);
		unitigs_free(c);
		return rc;
	}
	c->ug.slots = c->slots;
	c->ug.stale = false;
	c->ug.open = true;
	return SDT_OK;
}

int sdt_gpu_unitigs_fetch(sdt_ctx *c, uint64_t first, uint64_t n, uint64_t *keys, sdt_unitig *rec)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	int rc = unitigs_open(c, "sdt_gpu_unitigs_fetch");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_unitigs_fetch", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const size_t kw = 2 * (size_t)c->nw;
	if (keys) HIPCHK(hipMemcpyAsync(keys, c->ug.keys + first * kw, n * kw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	if (rec) HIPCHK(hipMemcpyAsync(rec, (const Unitig *)c->ug.rec + first, n * sizeof(Unitig), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

int sdt_gpu_unitigs_seqs(sdt_ctx *c, uint64_t first, uint64_t n, uint8_t *bases, uint64_t capacity, uint64_t *offsets)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!offsets || (!bases && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = unitigs_open(c, "sdt_gpu_unitigs_seqs");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_seqs");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_unitigs_seqs", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	std::vector<Unitig> rec((size_t)n);
	HIPCHK(hipMemcpyAsync(rec.data(), (const Unitig *)c->ug.rec + first, n * sizeof(Unitig), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	offsets[0] = 0;
	for (uint64_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + rec[i].nodes + (uint64_t)(c->K - 1);
	const uint64_t total = offsets[n];
	if (!bases && capacity == 0)
		return SDT_OK;                                       // (the offsets only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_seqs: %llu bases, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	DevBuf d_offs, d_bases, d_bad;
	rc = d_offs.get((n + 1) * sizeof(uint64_t), "sdt_gpu_unitigs_seqs: offsets");
	if (rc == SDT_OK) rc = d_bases.get(total, "sdt_gpu_unitigs_seqs: bases");
	if (rc == SDT_OK) rc = d_bad.get(sizeof(unsigned long long), "sdt_gpu_unitigs_seqs: counter");
	if (rc != SDT_OK) return rc;
	unsigned long long bad = 0;
	HIPCHK(hipMemcpyAsync(d_offs.p, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(d_bad.p, 0, sizeof bad, c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	const ClusterRule rule = rule_of(c);
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_ug_seqs<NW>, dim3(scan_grid(c, n)), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint64_t *)c->ug.keys,
		                   (const Unitig *)c->ug.rec, first, n, (const uint64_t *)d_offs.p, (uint8_t *)d_bases.p, (unsigned long long *)d_bad.p);
	});
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && ev) {
		e = hipEventRecord(ev->b, c->stream);
		ev->kmers = total;                                   // (bases written, not k-mers)
	}
	if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(bases, d_bases.p, total, hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (the buffers go when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	if (bad)
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_seqs: %llu unitigs do not walk as they did at sdt_gpu_unitigs_begin", bad);
	return SDT_OK;
}

int sdt_gpu_unitigs_links(sdt_ctx *c, uint64_t first, uint64_t n, sdt_unitig_link *links, uint64_t capacity, uint64_t *n_links, uint64_t *n_dangling)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!n_links || (!links && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = unitigs_open(c, "sdt_gpu_unitigs_links");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_links");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_unitigs_links", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf d_counts, d_offs, d_links, d_ctr;
	rc = d_counts.get(2 * n * sizeof(uint32_t), "sdt_gpu_unitigs_links: counts");
	if (rc == SDT_OK) rc = d_ctr.get(2 * sizeof(unsigned long long), "sdt_gpu_unitigs_links: counters");
	if (rc != SDT_OK) return rc;
	unsigned long long h[2] = {0, 0};                        // the dangling link ends; the out words that are not live
	std::vector<uint32_t> counts((size_t)(2 * n));
	std::vector<uint64_t> offs((size_t)(2 * n + 1));
	const ClusterRule rule = rule_of(c);
	const int g = scan_grid(c, 2 * n);
	auto launch = [&](const uint64_t *d_o, UnitigLink *d_l) {
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_ug_links<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint64_t *)c->ug.keys, c->ug.n,
			                   (const uint64_t *)c->ug.idx_keys, (const uint32_t *)c->ug.idx_id, first, n, (uint32_t *)d_counts.p, d_o, d_l, (unsigned long long *)d_ctr.p);
		});
		return hipGetLastError();
	};
	HIPCHK(hipMemsetAsync(d_ctr.p, 0, sizeof h, c->stream));
	hipError_t e = launch(nullptr, nullptr);
	if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_counts.p, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = hipStreamSynchronize(c->stream);
	HIPCHK(e);
	HIPCHK(e2);
	if (h[1])
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_links: %llu end words are not live as they were at sdt_gpu_unitigs_begin", h[1]);
	offs[0] = 0;
	for (uint64_t j = 0; j < 2 * n; j++) offs[j + 1] = offs[j] + counts[j];
	const uint64_t total = offs[2 * n];
	*n_links = total;
	if (n_dangling) *n_dangling = h[0];
	if (!links && capacity == 0)
		return SDT_OK;                                       // (the size only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_links: %llu links, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	if (total == 0)
		return SDT_OK;
	rc = d_offs.get((2 * n + 1) * sizeof(uint64_t), "sdt_gpu_unitigs_links: offsets");
	if (rc == SDT_OK) rc = d_links.get(total * sizeof(UnitigLink), "sdt_gpu_unitigs_links: links");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(d_offs.p, offs.data(), (2 * n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	e = launch((const uint64_t *)d_offs.p, (UnitigLink *)d_links.p);
	if (e == hipSuccess && ev) {
		e = hipEventRecord(ev->b, c->stream);
		ev->kmers = total;                                   // (links written, not k-mers)
	}
	if (e == hipSuccess) e = hipMemcpyAsync(links, d_links.p, total * sizeof(UnitigLink), hipMemcpyDeviceToHost, c->stream);
	e2 = hipStreamSynchronize(c->stream);                        // (the buffers go when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	return SDT_OK;
}

int sdt_gpu_unitigs_end(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	unitigs_free(c);
	return SDT_OK;
}

} // extern "C"
