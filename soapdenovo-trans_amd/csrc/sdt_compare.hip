// sdt_compare.hip -- two counted node tables compared on the device (the rule: include/sdt_gpu.h): the joint count spectrum with its
// totals = k_cmp_scan twice, A walked and B probed, then B walked and A probed; and the k-mers of A whose two counts lie in given
// ranges = k_cmp_select, k_ap_compact (sdt_compare_kernels.cuh, sdt_append.cuh).  The one call of the library that takes two contexts:
// both pass search_ready, both are entered, the work runs on A's stream after B's has been drained, and each context's high halves
// come through its own hi_prepare.  Nothing here writes ent or aux of either table, and neither the search cache (beyond preparing
// it) nor the assembly tally of either context is touched.  The time of a pass is booked on the context whose table it walks
// (sdt_gpu_kernel_time): pass 1 and the selection on A, pass 2 on B.
#include "sdt_readstage.hpp"
#include "sdt_compare_kernels.cuh"
#include <rocprim/rocprim.hpp>

static_assert(SDT_CMP_MAX_CELLS == CMP_MAX_CELLS, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_cmp_range) == sizeof(CmpRange), "include/sdt_gpu.h and the kernel agree");

// records of one call of compare_select: k_ap_compact's offsets are 32-bit
static const uint64_t CMP_SELECT_MAX = 1ULL << 31;

// both contexts can be asked, and asked together; the message names the call and the context
static int pair_ready(sdt_ctx *a, sdt_ctx *b, const char *what)
{
	char who[96];
	snprintf(who, sizeof who, "%s: context A", what);
	int rc = search_ready(a, who);
	if (rc != SDT_OK) return rc;
	snprintf(who, sizeof who, "%s: context B", what);
	rc = search_ready(b, who);
	if (rc != SDT_OK) return rc;
	if (a->K != b->K)
		return fail(SDT_EINVAL, "%s: context A has K = %d, context B has K = %d: tables of different K are not compared", what, a->K, b->K);
	if (a->device != b->device)
		return fail(SDT_EINVAL, "%s: context A is on device %d, context B on device %d", what, a->device, b->device);
	return SDT_OK;
}

// the workgroups of a scan over c's slots: scan_grid, raised until no workgroup visits 2^32 slots (the LDS counters are 32-bit)
static int cmp_grid(const sdt_ctx *c)
{
	uint64_t g = (uint64_t)scan_grid(c, c->slots);
	const uint64_t most = (1ULL << 32) - TPB;
	while ((c->slots / (g * TPB) + 1) * TPB > most) g *= 2;
	return (int)g;
}

// B's stream is drained (a count_reads_device queued on it is seen), both HiViews are ready, and what follows on A's stream sees them
static int pair_views(sdt_ctx *a, sdt_ctx *b, HiView *hva, HiView *hvb)
{
	int rc = flags_reserve(b);
	if (rc == SDT_OK) rc = hi_prepare(b, hvb);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipStreamSynchronize(b->stream));
	rc = flags_reserve(a);
	if (rc == SDT_OK) rc = hi_prepare(a, hva);
	return rc;
}

template <bool ONLY_ABSENT>
static int launch_scan(sdt_ctx *walked, sdt_ctx *other, const HiView &hv_other, hipStream_t stream, uint32_t rows, uint32_t cols,
                       unsigned long long *d_matrix, unsigned long long *d_totals)
{
	const int g = cmp_grid(walked);
	EventPair *ev = next_event(walked);
	if (ev) HIPCHK(hipEventRecord(ev->a, stream));
	by_key_width(walked, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cmp_scan<NW, ONLY_ABSENT>), dim3(g), dim3(TPB), (size_t)rows * cols * sizeof(uint32_t), stream, table_of<NW>(walked),
		                   table_of<NW>(other), hv_other, rows, cols, d_matrix, d_totals);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, stream));
		ev->kmers = walked->slots;                           // (slots walked, not k-mers: the occupied ones are known on the device only)
	}
	return SDT_OK;
}

// checked arguments, both contexts entered
static int compare_tables(sdt_ctx *a, sdt_ctx *b, uint32_t rows, uint32_t cols, uint64_t *matrix, uint64_t *totals)
{
	HiView hva, hvb;
	int rc = pair_views(a, b, &hva, &hvb);
	if (rc != SDT_OK) return rc;
	const size_t cells = (size_t)rows * cols, bytes = (CMP_TOTALS + cells) * sizeof(unsigned long long);
	DevBuf d;
	rc = d.get(bytes, "sdt_gpu_compare_tables: totals and matrix");
	if (rc != SDT_OK) return rc;
	unsigned long long *d_totals = (unsigned long long *)d.p, *d_matrix = d_totals + CMP_TOTALS;
	HIPCHK(hipMemsetAsync(d.p, 0, bytes, a->stream));
	rc = launch_scan<false>(a, b, hvb, a->stream, rows, cols, d_matrix, d_totals);
	if (rc == SDT_OK) rc = launch_scan<true>(b, a, hva, a->stream, rows, cols, d_matrix, d_totals);
	if (rc != SDT_OK) {
		(void)hipStreamSynchronize(a->stream);               // (the buffer goes when this returns)
		return rc;
	}
	if (totals) HIPCHK(hipMemcpyAsync(totals, d_totals, CMP_TOTALS * sizeof(unsigned long long), hipMemcpyDeviceToHost, a->stream));
	if (matrix) HIPCHK(hipMemcpyAsync(matrix, d_matrix, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, a->stream));
	HIPCHK(hipStreamSynchronize(a->stream));
	return SDT_OK;
}

// checked arguments, both contexts entered
static int compare_select(sdt_ctx *a, sdt_ctx *b, const sdt_cmp_range *range, uint64_t *keys, uint32_t *count_a, uint32_t *count_b, uint64_t capacity,
                          uint64_t *n)
{
	HiView hva, hvb;
	int rc = pair_views(a, b, &hva, &hvb);
	if (rc != SDT_OK) return rc;
	const int g = cmp_grid(a), stride = a->nw + 1;
	// a closed chunk holds more than AP_CH - 64 records and every wavefront has one open chunk: at least `capacity` records are kept
	const uint64_t cap_chunks = capacity ? capacity / (AP_CH - 64) + 1 + (uint64_t)g * (TPB / 64) : 0;
	DevBuf d_chunks, d_fill, d_off, d_cnt, d_dense, d_tmp;
	rc = d_cnt.get(2 * sizeof(unsigned long long), "sdt_gpu_compare_select: counters");
	if (rc == SDT_OK && cap_chunks) rc = d_chunks.get((size_t)cap_chunks * AP_CH * stride * sizeof(uint64_t), "sdt_gpu_compare_select: the list in chunks");
	if (rc == SDT_OK && cap_chunks) rc = d_fill.get((size_t)(cap_chunks + 1) * sizeof(uint32_t), "sdt_gpu_compare_select: chunk fills");
	if (rc == SDT_OK && cap_chunks) rc = d_off.get((size_t)(cap_chunks + 1) * sizeof(uint32_t), "sdt_gpu_compare_select: chunk fills");
	if (rc != SDT_OK) return rc;
	unsigned long long *d_cursor = (unsigned long long *)d_cnt.p, *d_matched = d_cursor + 1;
	HIPCHK(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), a->stream));
	if (cap_chunks) HIPCHK(hipMemsetAsync(d_fill.p, 0, (size_t)(cap_chunks + 1) * sizeof(uint32_t), a->stream));
	const ApOut out = {d_cursor, cap_chunks, (uint32_t *)d_fill.p, nullptr};
	const CmpRange rg = {range->min_a, range->max_a, range->min_b, range->max_b};
	EventPair *ev = next_event(a);
	if (ev) HIPCHK(hipEventRecord(ev->a, a->stream));
	by_key_width(a, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_cmp_select<NW>, dim3(g), dim3(TPB), 0, a->stream, table_of<NW>(a), table_of<NW>(b), hvb, rg, (uint64_t *)d_chunks.p, out, d_matched);
	});
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && ev) {
		e = hipEventRecord(ev->b, a->stream);
		ev->kmers = a->slots;
	}
	unsigned long long cnt[2] = {0, 0};
	if (e == hipSuccess) e = hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, a->stream);
	const hipError_t e2 = hipStreamSynchronize(a->stream);       // (the buffers go when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	if (n) *n = cnt[1];
	const uint64_t n_chunks = cnt[0] < cap_chunks ? cnt[0] : cap_chunks;
	if (!n_chunks) return SDT_OK;
	// the chunks packed into one dense list: an exclusive scan of the fills, k_ap_compact
	size_t tb = 0;
	uint32_t total = 0;
	HIPCHK(rocprim::exclusive_scan(nullptr, tb, (uint32_t *)d_fill.p, (uint32_t *)d_off.p, uint32_t(0), (size_t)n_chunks + 1, rocprim::plus<uint32_t>(), a->stream));
	rc = d_tmp.get(tb, "sdt_gpu_compare_select: scan");
	if (rc != SDT_OK) return rc;
	e = rocprim::exclusive_scan(d_tmp.p, tb, (uint32_t *)d_fill.p, (uint32_t *)d_off.p, uint32_t(0), (size_t)n_chunks + 1, rocprim::plus<uint32_t>(), a->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&total, (uint32_t *)d_off.p + n_chunks, sizeof total, hipMemcpyDeviceToHost, a->stream);
	const hipError_t e3 = hipStreamSynchronize(a->stream);
	HIPCHK(e);
	HIPCHK(e3);
	if (!total) return SDT_OK;
	rc = d_dense.get((size_t)total * stride * sizeof(uint64_t), "sdt_gpu_compare_select: the dense list");
	if (rc != SDT_OK) return rc;
	hipLaunchKernelGGL(k_ap_compact, dim3(scan_grid(a, n_chunks * AP_CH)), dim3(256), 0, a->stream, (const uint64_t *)d_chunks.p, (const uint32_t *)d_fill.p,
	                   (const uint32_t *)d_off.p, (unsigned long long)n_chunks, stride, (uint64_t *)d_dense.p);
	e = hipGetLastError();
	const uint64_t take = total < capacity ? total : capacity;
	uint64_t *rec = (uint64_t *)malloc((size_t)take * stride * sizeof(uint64_t));
	if (e == hipSuccess && rec) e = hipMemcpyAsync(rec, d_dense.p, (size_t)take * stride * sizeof(uint64_t), hipMemcpyDeviceToHost, a->stream);
	const hipError_t e4 = hipStreamSynchronize(a->stream);
	if (e != hipSuccess || e4 != hipSuccess || !rec) {
		free(rec);
		HIPCHK(e);
		HIPCHK(e4);
		return fail(SDT_ENOMEM, "sdt_gpu_compare_select: %llu bytes of host memory for the list", (unsigned long long)take * stride * sizeof(uint64_t));
	}
	const int nw = a->nw;
	for (uint64_t i = 0; i < take; i++) {
		const uint64_t *r = rec + i * stride;
		if (keys) memcpy(keys + i * nw, r, (size_t)nw * sizeof(uint64_t));
		if (count_a) count_a[i] = (uint32_t)r[nw];
		if (count_b) count_b[i] = (uint32_t)(r[nw] >> 32);
	}
	free(rec);
	return SDT_OK;
}

extern "C" {

int sdt_gpu_compare_tables(sdt_ctx *a, sdt_ctx *b, const sdt_cmp_params *params, uint64_t *matrix, uint64_t totals[8])
{
	if (!a || !b)
		return fail(SDT_EINVAL, "sdt_gpu_compare_tables: context %s is NULL", !a ? "A" : "B");
	if (!params)
		return fail(SDT_EINVAL, "sdt_gpu_compare_tables: sdt_cmp_params is NULL");
	if (params->rows < 2)
		return fail(SDT_EINVAL, "sdt_cmp_params.rows = %u: 2 at least", params->rows);
	if (params->cols < 2)
		return fail(SDT_EINVAL, "sdt_cmp_params.cols = %u: 2 at least", params->cols);
	if ((uint64_t)params->rows * params->cols > SDT_CMP_MAX_CELLS)
		return fail(SDT_EINVAL, "sdt_cmp_params: rows x cols = %u x %u = %llu cells: %u at most", params->rows, params->cols,
		            (unsigned long long)params->rows * params->cols, SDT_CMP_MAX_CELLS);
	if (params->flags)
		return fail(SDT_EINVAL, "sdt_cmp_params.flags = 0x%x: no flag is defined", params->flags);
	if (params->reserved)
		return fail(SDT_EINVAL, "sdt_cmp_params.reserved = %u: it must be 0", params->reserved);
	if (!matrix && !totals)
		return fail(SDT_EINVAL, "sdt_gpu_compare_tables: matrix and totals are both NULL");
	const int rc = pair_ready(a, b, "sdt_gpu_compare_tables");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(a);
	SDT_ENTER(b);
	return compare_tables(a, b, params->rows, params->cols, matrix, totals);
}

int sdt_gpu_compare_select(sdt_ctx *a, sdt_ctx *b, const sdt_cmp_range *range, uint64_t *keys, uint32_t *count_a, uint32_t *count_b, uint64_t capacity,
                           uint64_t *n)
{
	if (!a || !b)
		return fail(SDT_EINVAL, "sdt_gpu_compare_select: context %s is NULL", !a ? "A" : "B");
	if (!range)
		return fail(SDT_EINVAL, "sdt_gpu_compare_select: sdt_cmp_range is NULL");
	if (range->min_a > range->max_a)
		return fail(SDT_EINVAL, "sdt_cmp_range: min_a = %u is above max_a = %u", range->min_a, range->max_a);
	if (range->min_b > range->max_b)
		return fail(SDT_EINVAL, "sdt_cmp_range: min_b = %u is above max_b = %u", range->min_b, range->max_b);
	if (capacity && !keys && !count_a && !count_b)
		return fail(SDT_EINVAL, "sdt_gpu_compare_select: capacity = %llu and every array is NULL", (unsigned long long)capacity);
	if (capacity > CMP_SELECT_MAX)
		return fail(SDT_EINVAL, "sdt_gpu_compare_select: capacity = %llu: %llu at most in one call (narrow the ranges)", (unsigned long long)capacity,
		            (unsigned long long)CMP_SELECT_MAX);
	const int rc = pair_ready(a, b, "sdt_gpu_compare_select");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(a);
	SDT_ENTER(b);
	return compare_select(a, b, range, keys, count_a, count_b, capacity, n);
}

} // extern "C"
