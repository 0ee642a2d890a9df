// sdt_bubble.hip -- the bubbles of the counted k-mer graph (the rule: include/sdt_gpu.h).  bubbles_begin = k_bb_forks (the fork sides,
// listed), k_bb_walk (one lane per fork, its branches in turn; the pairs that meet), a radix sort of the records by (s, base_a, base_b),
// k_bb_permute (sdt_bubble_kernels.cuh); bubbles_paths walks the requested branches again.  Nothing here writes the table, the kept reads or
// a cache of the context.  What the context keeps from bubbles_begin to bubbles_end is the sorted list -- N records and their two words
// each -- and nothing per table slot; it is tied to the state of the table it was found on as the clustering is (search_cache_drop,
// delow, the graph phases mark it stale), because the paths are read from the table.  State rules are those of the read stages.
#include "sdt_readstage.hpp"
#include "sdt_bubble_kernels.cuh"
#include <rocprim/rocprim.hpp>
#include <cstddef>

static_assert(sizeof(sdt_bubble) == sizeof(Bubble) && offsetof(sdt_bubble, len_a) == 16 && offsetof(sdt_bubble, info) == 40, "include/sdt_gpu.h and the kernel agree");

static int bubbles_open(const sdt_ctx *c, const char *what)
{
	if (!c->bb.open)
		return fail(SDT_ESTATE, "%s: no bubble list: call sdt_gpu_bubbles_begin first", what);
	if (c->bb.stale || c->bb.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_bubbles_begin", what);
	return SDT_OK;
}

static void bubbles_free(sdt_ctx *c)
{
	if (c->bb.keys) (void)hipFree(c->bb.keys);
	if (c->bb.rec) (void)hipFree(c->bb.rec);
	c->bb = sdt_ctx::Bubbles();
}

static int bubble_params_ok(const sdt_bubble_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_bubble_params is NULL");
	if (p->flags)
		return fail(SDT_EINVAL, "sdt_bubble_params.flags = 0x%x: no flag is defined", p->flags);
	if (p->reserved)
		return fail(SDT_EINVAL, "sdt_bubble_params.reserved = %u: must be 0", p->reserved);
	if (p->min_link < 1 || p->min_link > 63)
		return fail(SDT_EINVAL, "sdt_bubble_params.min_link = %u: 1 to 63 (a link counter saturates at 63)", p->min_link);
	const uint32_t mc = p->min_count > 1 ? p->min_count : 1u;
	if (p->max_count && p->max_count < mc)
		return fail(SDT_EINVAL, "sdt_bubble_params.max_count = %u is below min_count = %u: 0 (no upper bound) or at least that", p->max_count, mc);
	if (p->max_len < 1 || p->max_len > SDT_BUBBLE_MAX_LEN)
		return fail(SDT_EINVAL, "sdt_bubble_params.max_len = %u: 1 to %u inner nodes", p->max_len, SDT_BUBBLE_MAX_LEN);
	return SDT_OK;
}

static BubbleRule rule_of(const sdt_ctx *c) { return BubbleRule{{c->bb.min_count, c->bb.max_count, c->bb.min_link}, c->bb.max_len}; }

// the records in raw put in the order of (s, base_a, base_b): stable passes from the least significant part; *sorted: the order
static int sort_records(sdt_ctx *c, const uint64_t *raw, int stride, uint64_t n, DevBuf &o_a, DevBuf &o_b, DevBuf &k_a, DevBuf &k_b, uint32_t **sorted)
{
	size_t tb = 0;
	HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, (uint64_t *)k_a.p, (uint64_t *)k_b.p, (uint32_t *)o_a.p, (uint32_t *)o_b.p, (size_t)n, 0, 64, c->stream));
	DevBuf d_tmp;
	int rc = d_tmp.get(tb, "sdt_gpu_bubbles_begin: sort");
	if (rc != SDT_OK) return rc;
	uint32_t *in = (uint32_t *)o_a.p, *out = (uint32_t *)o_b.p;
	const int g = scan_grid(c, n);
	hipLaunchKernelGGL(k_bb_iota, dim3(g), dim3(TPB), 0, c->stream, in, n);
	hipError_t e = hipGetLastError();
	for (int w = c->nw; w >= 0 && e == hipSuccess; w--) {        // (w == nw: the two bases; then the words of s from the last)
		hipLaunchKernelGGL(k_bb_sortkey, dim3(g), dim3(TPB), 0, c->stream, raw, stride, c->nw, (const uint32_t *)in, n, w == c->nw ? -1 : w, (uint64_t *)k_a.p);
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

// checked arguments, the context entered, no list held; on failure the caller frees what is in c->bb
static int bubbles_build(sdt_ctx *c, const BubbleRule &rule, uint64_t info[8])
{
	const uint64_t slots = c->slots;
	const int stride = 2 * c->nw + BB_REC_WORDS;
	DevBuf d_ctr, d_list, d_cur, d_raw, d_oa, d_ob, d_ka, d_kb;
	int rc = d_ctr.get(BB_COUNTERS * sizeof(unsigned long long), "sdt_gpu_bubbles_begin: counters");
	if (rc == SDT_OK) rc = d_cur.get(sizeof(unsigned long long), "sdt_gpu_bubbles_begin: counters");
	if (rc != SDT_OK) return rc;
	unsigned long long *ctr = (unsigned long long *)d_ctr.p, h[BB_COUNTERS] = {}, n_chunks = 0;
	const int g = scan_grid(c, slots);
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	// the fork sides: a first guess of one per 64 slots, and once more with the chunks that were asked for when they did not fit
	uint64_t cap_chunks = (slots / 64 + 4096) / (AP_CH - 64) + 1 + (uint64_t)g * (TPB / 64);
	for (int attempt = 0;; attempt++) {
		rc = d_list.get(cap_chunks * AP_CH * sizeof(unsigned long long), "sdt_gpu_bubbles_begin: the fork list");
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemsetAsync(ctr, 0, BB_COUNTERS * sizeof(unsigned long long), c->stream));
		HIPCHK(hipMemsetAsync(d_cur.p, 0, sizeof(unsigned long long), c->stream));
		const ApOut ap = {(unsigned long long *)d_cur.p, cap_chunks, nullptr, (unsigned long long *)d_list.p};
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_bb_forks<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (unsigned long long *)d_list.p, ap, ctr);
		});
		hipError_t e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(&n_chunks, d_cur.p, sizeof n_chunks, hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = hipStreamSynchronize(c->stream);   // (the buffers go when this returns)
		HIPCHK(e);
		HIPCHK(e2);
		if (n_chunks <= cap_chunks) break;
		if (attempt)
			return fail(SDT_ESTATE, "sdt_gpu_bubbles_begin: the number of fork sides changed between two scans");
		cap_chunks = n_chunks;
	}
	const uint64_t n_live = h[BB_N_LIVE], n_forks = h[BB_N_FORKS], n_list = n_chunks * AP_CH;
	// the walks: a fork side has four branches at the most, and so six pairs
	const uint64_t cap = 6 * n_forks;
	uint64_t n = 0;
	if (n_forks) {
		rc = d_raw.get(cap * stride * sizeof(uint64_t), "sdt_gpu_bubbles_begin: the bubbles as they are found, six per fork side at the most");
		if (rc != SDT_OK) return rc;
		const int gw = scan_grid(c, n_list);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_bb_walk<NW>, dim3(gw), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const unsigned long long *)d_list.p,
			                   (unsigned long long)n_list, (uint64_t *)d_raw.p, (unsigned long long)cap, ctr);
		});
		hipError_t e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = hipStreamSynchronize(c->stream);
		HIPCHK(e);
		HIPCHK(e2);
		n = h[BB_N_REC];
		if (n > cap)
			return fail(SDT_ESTATE, "sdt_gpu_bubbles_begin: %llu bubbles from %llu fork sides", (unsigned long long)n, (unsigned long long)n_forks);
		if (n > 0xFFFFFFFFULL)
			return fail(SDT_ENOMEM, "sdt_gpu_bubbles_begin: %llu bubbles: the sort's indices are 32-bit", (unsigned long long)n);
	}
	if (n) {
		rc = d_oa.get(n * sizeof(uint32_t), "sdt_gpu_bubbles_begin: sort order");
		if (rc == SDT_OK) rc = d_ob.get(n * sizeof(uint32_t), "sdt_gpu_bubbles_begin: sort order");
		if (rc == SDT_OK) rc = d_ka.get(n * sizeof(uint64_t), "sdt_gpu_bubbles_begin: sort keys");
		if (rc == SDT_OK) rc = d_kb.get(n * sizeof(uint64_t), "sdt_gpu_bubbles_begin: sort keys");
		if (rc != SDT_OK) return rc;
		hipError_t e = hipMalloc((void **)&c->bb.keys, n * 2 * c->nw * sizeof(uint64_t));
		if (e != hipSuccess) c->bb.keys = nullptr;
		if (e == hipSuccess) {
			e = hipMalloc(&c->bb.rec, n * sizeof(Bubble));
			if (e != hipSuccess) c->bb.rec = nullptr;
		}
		if (e != hipSuccess)
			return fail(SDT_ENOMEM, "the bubble list: %llu records of %zu bytes: %s", (unsigned long long)n, sizeof(Bubble) + 2 * c->nw * sizeof(uint64_t), hipGetErrorString(e));
		uint32_t *sorted = nullptr;
		rc = sort_records(c, (const uint64_t *)d_raw.p, stride, n, d_oa, d_ob, d_ka, d_kb, &sorted);
		if (rc != SDT_OK) return rc;
		hipLaunchKernelGGL(k_bb_permute, dim3(scan_grid(c, n)), dim3(TPB), 0, c->stream, (const uint64_t *)d_raw.p, stride, c->nw, (const uint32_t *)sorted, n, c->bb.keys,
		                   (Bubble *)c->bb.rec, ctr);
		e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = hipStreamSynchronize(c->stream);
		HIPCHK(e);
		HIPCHK(e2);
	}
	c->bb.n = n;
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = slots;                                   // (slots scanned, not k-mers)
	}
	if (info) {
		const uint64_t out[8] = {n_live, n_forks, h[BB_N_BRANCHES], h[BB_N_REACHED], n, h[BB_PATH_BYTES], h[BB_LONGEST], 0};
		memcpy(info, out, sizeof out);
	}
	return SDT_OK;
}

static int range_ok(const sdt_ctx *c, const char *what, uint64_t first, uint64_t n)
{
	if (first > c->bb.n || n > c->bb.n - first)
		return fail(SDT_EINVAL, "%s: bubbles %llu .. %llu of %llu", what, (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)c->bb.n);
	return SDT_OK;
}

extern "C" {

int sdt_gpu_bubbles_begin(sdt_ctx *c, const sdt_bubble_params *params, uint64_t info[8])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	int rc = bubble_params_ok(params);
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_bubbles_begin");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	bubbles_free(c);                                         // (a second begin replaces the first)
	c->bb.min_count = params->min_count > 1 ? params->min_count : 1u;
	c->bb.max_count = params->max_count;
	c->bb.min_link = params->min_link;
	c->bb.max_len = params->max_len;
	rc = bubbles_build(c, rule_of(c), info);
	if (rc != SDT_OK) {
		(void)hipStreamSynchronize(c->stream);
		bubbles_free(c);
		return rc;
	}
	c->bb.slots = c->slots;
	c->bb.stale = false;
	c->bb.open = true;
	return SDT_OK;
}

int sdt_gpu_bubbles_fetch(sdt_ctx *c, uint64_t first, uint64_t n, uint64_t *keys, sdt_bubble *rec)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	int rc = bubbles_open(c, "sdt_gpu_bubbles_fetch");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_bubbles_fetch", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const size_t kw = 2 * (size_t)c->nw;
	if (keys) HIPCHK(hipMemcpyAsync(keys, c->bb.keys + first * kw, n * kw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	if (rec) HIPCHK(hipMemcpyAsync(rec, (const Bubble *)c->bb.rec + first, n * sizeof(Bubble), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

int sdt_gpu_bubbles_paths(sdt_ctx *c, uint64_t first, uint64_t n, uint8_t *bases, uint64_t capacity, uint64_t *offsets)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!offsets || (!bases && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = bubbles_open(c, "sdt_gpu_bubbles_paths");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_bubbles_paths");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_bubbles_paths", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	std::vector<Bubble> rec((size_t)n);
	HIPCHK(hipMemcpyAsync(rec.data(), (const Bubble *)c->bb.rec + first, n * sizeof(Bubble), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	offsets[0] = 0;
	for (uint64_t i = 0; i < n; i++) {
		offsets[2 * i + 1] = offsets[2 * i] + rec[i].len_a + 1;
		offsets[2 * i + 2] = offsets[2 * i + 1] + rec[i].len_b + 1;
	}
	const uint64_t total = offsets[2 * n];
	if (!bases && capacity == 0)
		return SDT_OK;                                       // (the offsets only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_bubbles_paths: %llu bases, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	DevBuf d_offs, d_bases, d_bad;
	rc = d_offs.get((2 * n + 1) * sizeof(uint64_t), "sdt_gpu_bubbles_paths: offsets");
	if (rc == SDT_OK) rc = d_bases.get(total, "sdt_gpu_bubbles_paths: bases");
	if (rc == SDT_OK) rc = d_bad.get(sizeof(unsigned long long), "sdt_gpu_bubbles_paths: counter");
	if (rc != SDT_OK) return rc;
	unsigned long long bad = 0;
	HIPCHK(hipMemcpyAsync(d_offs.p, offsets, (2 * n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(d_bad.p, 0, sizeof bad, c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	const BubbleRule rule = rule_of(c);
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_bb_paths<NW>, dim3(scan_grid(c, 2 * n)), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint64_t *)c->bb.keys,
		                   (const Bubble *)c->bb.rec, first, n, (const uint64_t *)d_offs.p, (uint8_t *)d_bases.p, (unsigned long long *)d_bad.p);
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
		return fail(SDT_ESTATE, "sdt_gpu_bubbles_paths: %llu branches do not walk as they did at sdt_gpu_bubbles_begin", bad);
	return SDT_OK;
}

int sdt_gpu_bubbles_end(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	bubbles_free(c);
	return SDT_OK;
}

} // extern "C"
