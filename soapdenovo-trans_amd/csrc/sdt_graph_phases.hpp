// sdt_graph_phases.hpp -- what the two translation units of the graph phases share (sdt_gpu_graph.hip: the ABI entry points, the
// host side of the layout and the Ix32 form, sdt_gpu_graph64.hip: the Ix64 form): the unit's state, the idiom of its host code
// (LAUNCH_NW*: dispatch by key width, Scratch: the device buffers of a call, GCHK: HIP errors, CallTimer: the SDT_TIMING lines),
// and the phases whose node indices take one of the two forms of sdt_graph_kernels.cuh as a template parameter.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <rocprim/rocprim.hpp>

#include "sdt_internal.hpp"

using namespace sdt;

#include "sdt_append.cuh"
#include "sdt_graph_kernels.cuh"

using sdti::fail;
using sdti::GraphView;

struct sdti::GraphExt {
	uint64_t *d_sval = nullptr;       // rank in (set, first-occurrence) order -> table slot   (layout_sorted_keys .. layout_apply)
	uint64_t n_sorted = 0;
	uint64_t *d_slot_of = nullptr;    // node index (visiting order) -> table slot
	uint64_t n_nodes = 0;
	uint64_t *d_result = nullptr;     // records of the last labelled dry run, waiting for sdt_gpu_fetch_records
	uint64_t result_words = 0;
	uint64_t result_labelled = 0;     // the first so many of them are sorted by (component, node)
	int result_stride = 0;
	uint64_t *d_wnode = nullptr;      // nodes the last sdt_gpu_minor_out_commit wrote, waiting for sdt_gpu_fetch_written
	uint32_t *d_wl = nullptr, *d_wr = nullptr;
	uint64_t n_written = 0;
	uint64_t *d_skipped = nullptr;    // records of the components that commit left to the host, waiting for sdt_gpu_fetch_skipped
	uint64_t n_skipped = 0;
	bool mo_pending = false;          // between sdt_gpu_minor_out_commit_begin and _finish: what the launched kernels work on
	uint8_t *mo_dirty = nullptr;
	unsigned long long *mo_cnt = nullptr;
	uint32_t *mo_recidx = nullptr, *mo_cstart = nullptr;
	unsigned char *d_seq = nullptr;   // bases of the edges of sdt_gpu_build_edges, waiting for sdt_gpu_fetch_edge_bases
	uint64_t seq_bytes = 0;
	uint64_t *d_pw = nullptr;         // path word of every node after sdt_gpu_build_edges (taken by sdt_gpu_load_paths)
	uint64_t pw_n = 0;
	// node-index form (sdt_graph_kernels.cuh), fixed when the nodes are numbered: Ix64 past 2^32 - 16 nodes or when asked for
	int want_bits = 0;                // sdt_gpu_set_graph_index_bits: 0 = by node count, 64 = wide
	bool wide = false;                // the form of the numbering in effect
	uint64_t base = 0;                // Ix64 only: node index of position 0 (0; SDT_NODE_BASE under the test hooks)
	bool result_nodes = false;        // d_result holds node indices (the labelled dry runs; not the edge records)
};

// the node indices of a graph of n nodes in the form the context asks for: chosen when the nodes are numbered
int graph_choose_form(sdti::GraphExt *gx, uint64_t n);
inline Ix64 ix64_of(const sdti::GraphExt *gx) { return Ix64{gx->base}; }

static sdti::GraphExt *ext_of(const GraphView &v)
{
	if (!*v.gx) *v.gx = new sdti::GraphExt();
	return *v.gx;
}

#define LAUNCH_NW(v, kernel, grid, ...)                                                                                      \
	do {                                                                                                                     \
		if ((v).nw == 1) hipLaunchKernelGGL(kernel<1>, dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<1>(v), __VA_ARGS__);      \
		else if ((v).nw == 2) hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<2>(v), __VA_ARGS__); \
		else hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<4>(v), __VA_ARGS__);                  \
	} while (0)
// the same for the kernels that take the node-index form IX as their second template parameter
#define LAUNCH_NW_IX(v, kernel, IXT, grid, ...)                                                                                    \
	do {                                                                                                                     \
		if ((v).nw == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<1, IXT>), dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<1>(v), __VA_ARGS__);      \
		else if ((v).nw == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<2, IXT>), dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<2>(v), __VA_ARGS__); \
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<4, IXT>), dim3(grid), dim3(TPB), 0, (v).stream, sdti::table_of<4>(v), __VA_ARGS__);                  \
	} while (0)

// the same for the kernels that are templates over the key words but take no table (the layout replay's k_rp_rehash_init, k_rp_home)
#define LAUNCH_NW_NOTAB(v, kernel, grid, ...)                                                                                \
	do {                                                                                                                     \
		if ((v).nw == 1) hipLaunchKernelGGL(kernel<1>, dim3(grid), dim3(TPB), 0, (v).stream, __VA_ARGS__);                   \
		else if ((v).nw == 2) hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(TPB), 0, (v).stream, __VA_ARGS__);              \
		else hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(TPB), 0, (v).stream, __VA_ARGS__);                               \
	} while (0)

// SDT_TIMING: where the time of a call goes, on stderr (tools/e2e_pregraph.py collects the "[device]" lines).  One per call; without
// SDT_TIMING no clock is read
struct CallTimer {
	const bool on;
	const double t0;
	explicit CallTimer(bool wanted = true) : on(wanted && sdt_env("SDT_TIMING") != nullptr), t0(on ? now() : 0) {}
	static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
	double ms() const { return on ? now() - t0 : 0; }          // since the call began
	void tick(const char *what) const { if (on) fprintf(stderr, "[device]       %s at %.1f ms\n", what, ms()); }
};

// every device buffer of a call in one place: freed when the call returns, whatever the path
struct Scratch {
	void *p[96] = {};
	int n = 0;
	template <class T> hipError_t alloc(T **out, size_t bytes)
	{
		void *q = nullptr;
		if (n == (int)(sizeof p / sizeof p[0])) { *out = nullptr; return hipErrorOutOfMemory; }
		const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
		if (e == hipSuccess) p[n++] = q;
		*out = (T *)q;
		return e;
	}
	void *release(void *q)                                    // the caller keeps q
	{
		for (int i = 0; i < n; i++) if (p[i] == q) p[i] = nullptr;
		return q;
	}
	~Scratch() { for (int i = 0; i < n; i++) if (p[i]) (void)hipFree(p[i]); }
};

#define GCHK(expr) do { hipError_t e9_ = (expr); if (e9_ != hipSuccess) return fail(e9_ == hipErrorOutOfMemory ? SDT_ENOMEM : SDT_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e9_), __FILE__, __LINE__); } while (0)

// device-wide sort of (key, value) pairs by the key bits [0, end_bit): rocPRIM's radix sort ping-pongs between the caller's input and
// output arrays (double buffers: the INPUT arrays are scratch afterwards), so its own temporary storage stays small -- with separate
// in / out arrays it asked for as much again as the pairs (10 GiB at 678 M nodes, from the driver)
template <class V>
static int sort_pairs(const GraphView &v, uint64_t *k_in, uint64_t *k_out, V *v_in, V *v_out, uint64_t n, unsigned end_bit)
{
	rocprim::double_buffer<uint64_t> dk(k_in, k_out);
	rocprim::double_buffer<V> dv(v_in, v_out);
	size_t tmp_bytes = 0;
	GCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, dk, dv, (size_t)n, 0u, end_bit, v.stream));
	void *tmp = nullptr;
	GCHK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
	hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, dk, dv, (size_t)n, 0u, end_bit, v.stream);
	if (e == hipSuccess && dk.current() != k_out) e = hipMemcpyAsync(k_out, dk.current(), n * sizeof(uint64_t), hipMemcpyDeviceToDevice, v.stream);
	if (e == hipSuccess && dv.current() != v_out) e = hipMemcpyAsync(v_out, dv.current(), n * sizeof(V), hipMemcpyDeviceToDevice, v.stream);
	const hipError_t e2 = hipStreamSynchronize(v.stream);
	(void)hipFree(tmp);
	if (e != hipSuccess || e2 != hipSuccess) return fail(SDT_EHIP, "radix sort of %llu pairs: %s", (unsigned long long)n, hipGetErrorString(e != hipSuccess ? e : e2));
	return SDT_OK;
}

template <class T, class TIn = T>
static int exclusive_scan(const GraphView &v, const TIn *in, T *out, uint64_t n)
{
	size_t tmp_bytes = 0;
	GCHK(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), v.stream));
	void *tmp = nullptr;
	GCHK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
	const hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), v.stream);
	const hipError_t e2 = hipStreamSynchronize(v.stream);
	(void)hipFree(tmp);
	if (e != hipSuccess || e2 != hipSuccess) return fail(SDT_EHIP, "prefix sum over %llu items: %s", (unsigned long long)n, hipGetErrorString(e != hipSuccess ? e : e2));
	return SDT_OK;
}

// ---- records appended in chunks per wave (sdt_append.cuh): storage, and packing into one dense array ---------------------
struct ApBuf {
	uint64_t *chunks = nullptr;
	uint32_t *fill = nullptr, *off = nullptr;
	unsigned long long *cursor = nullptr;
	uint64_t cap_chunks = 0;
	int stride = 0;
};
static ApOut ap_out(const ApBuf &B) { return ApOut{B.cursor, B.cap_chunks, B.fill, nullptr}; }
// room for `records` records of `stride` words (a closed chunk holds more than AP_CH - 64 records, every wave has one open chunk)
static int ap_alloc(Scratch &S, const GraphView &v, ApBuf &B, uint64_t records, int stride)
{
	B.cap_chunks = records / (AP_CH - 64) + 1 + (uint64_t)v.cu_count * 8 * (TPB / 64);
	B.stride = stride;
	GCHK(S.alloc(&B.chunks, B.cap_chunks * AP_CH * (size_t)stride * 8));
	GCHK(S.alloc(&B.fill, (B.cap_chunks + 1) * 4)); GCHK(S.alloc(&B.off, (B.cap_chunks + 1) * 4)); GCHK(S.alloc(&B.cursor, 8));
	GCHK(hipMemsetAsync(B.fill, 0, (B.cap_chunks + 1) * 4, v.stream));
	GCHK(hipMemsetAsync(B.cursor, 0, 8, v.stream));
	return SDT_OK;
}
static void ap_free(Scratch &S, ApBuf &B)
{
	(void)hipFree(S.release(B.chunks)); (void)hipFree(S.release(B.fill)); (void)hipFree(S.release(B.off)); (void)hipFree(S.release(B.cursor));
	B = ApBuf();
}
// the records of chunks [0, n_chunks) packed in chunk order into a new array (the caller's Scratch owns it); *n_split = the records
// of the chunks before split_chunk (what an earlier kernel wrote)
static int ap_compact(Scratch &S, const GraphView &v, const ApBuf &B, uint64_t n_chunks, uint64_t split_chunk, uint64_t **out, uint64_t *n_out, uint64_t *n_split)
{
	if (n_chunks > B.cap_chunks) return fail(SDT_ESTATE, "records in chunks: %llu chunks taken, room for %llu", (unsigned long long)n_chunks, (unsigned long long)B.cap_chunks);
	const int rc = exclusive_scan<uint32_t>(v, B.fill, B.off, n_chunks + 1);          // (fill[n_chunks] is 0: off[n_chunks] = all records)
	if (rc != SDT_OK) return rc;
	uint32_t tot = 0, spl = 0;
	GCHK(hipMemcpy(&tot, B.off + n_chunks, 4, hipMemcpyDeviceToHost));
	GCHK(hipMemcpy(&spl, B.off + (split_chunk < n_chunks ? split_chunk : n_chunks), 4, hipMemcpyDeviceToHost));
	GCHK(S.alloc(out, ((size_t)tot + 1) * (size_t)B.stride * 8));
	if (n_chunks) hipLaunchKernelGGL(k_ap_compact, dim3(sdti::scan_grid(v.cu_count, n_chunks * AP_CH)), dim3(256), 0, v.stream, B.chunks, B.fill, B.off,
	                                 (unsigned long long)n_chunks, B.stride, *out);
	GCHK(hipGetLastError());
	*n_out = tot;
	if (n_split) *n_split = spl;
	return SDT_OK;
}

// ---- labelled dry runs ------------------------------------------------------------------------------------------------
// label the first n_label records (stride words each, node in the low 56 bits of word 0, label into word stride - 1) with the
// roots of `parent`, sort them by (label, node) and leave all n records in gx->d_result
template <class IX>
static int label_sort_keep(sdt_ctx *c, const GraphView &v, IX ix, typename IX::T *parent, uint64_t *d_rec, uint64_t n, uint64_t n_label, int stride)
{
	constexpr bool W = sizeof(typename IX::T) == 8;
	sdti::GraphExt *gx = ext_of(v);
	if (gx->d_result) { (void)hipFree(gx->d_result); gx->d_result = nullptr; gx->result_words = 0; }
	Scratch S;
	uint64_t *k0, *k1, *d_out;
	uint32_t *p0, *p1;
	const uint64_t m = n_label ? n_label : 1;
	GCHK(S.alloc(&k0, m * 8)); GCHK(S.alloc(&k1, m * 8)); GCHK(S.alloc(&p0, m * 4)); GCHK(S.alloc(&p1, m * 4));
	GCHK(S.alloc(&d_out, (n ? n : 1) * (size_t)stride * 8));
	if constexpr (!W) {
		if (n_label) {
			hipLaunchKernelGGL(k_uf_label, dim3(sdti::scan_grid(v.cu_count, n_label)), dim3(TPB), 0, v.stream, parent, d_rec, n_label, stride, stride - 1, k0, p0);
			GCHK(hipGetLastError());
			const int rc = sort_pairs<uint32_t>(v, k0, k1, p0, p1, n_label, 64);
			if (rc != SDT_OK) return rc;
		}
	} else if (n_label) {
		// two stable passes over the bits node indices use: by node, then by the label of the records in that order
		unsigned end_bit = 1;
		while (end_bit < 64 && (ix.base() + *v.idx_n) >> end_bit) end_bit++;
		const dim3 gl(sdti::scan_grid(v.cu_count, n_label));
		hipLaunchKernelGGL(k_uf_label_wide, gl, dim3(TPB), 0, v.stream, parent, d_rec, n_label, stride, stride - 1, k0, p0, ix);
		GCHK(hipGetLastError());
		int rc = sort_pairs<uint32_t>(v, k0, k1, p0, p1, n_label, end_bit);
		if (rc != SDT_OK) return rc;
		hipLaunchKernelGGL(k_uf_label_keys, gl, dim3(TPB), 0, v.stream, d_rec, p1, n_label, stride, stride - 1, k0);
		GCHK(hipGetLastError());
		rc = sort_pairs<uint32_t>(v, k0, k1, p1, p0, n_label, end_bit);
		if (rc != SDT_OK) return rc;
		std::swap(p0, p1);                                        // (the permutation is in p1 below, as after the one pass)
	}
	if (n_label) {
		hipLaunchKernelGGL(k_gather_records, dim3(sdti::scan_grid(v.cu_count, n_label * stride)), dim3(TPB), 0, v.stream, d_rec, p1, n_label, stride, d_out);
		GCHK(hipGetLastError());
	}
	if (n > n_label) {                                        // (the records behind the sorted ones keep their order; they get their label too)
		hipLaunchKernelGGL(k_uf_label_only<IX>, dim3(sdti::scan_grid(v.cu_count, n - n_label)), dim3(TPB), 0, v.stream, parent, d_rec, n_label, n, stride, stride - 1, ix);
		GCHK(hipGetLastError());
		GCHK(hipMemcpyAsync(d_out + n_label * stride, d_rec + n_label * stride, (n - n_label) * (size_t)stride * 8, hipMemcpyDeviceToDevice, v.stream));
	}
	GCHK(hipStreamSynchronize(v.stream));
	(void)c;
	gx->d_result = (uint64_t *)S.release(d_out);
	gx->result_words = n * (uint64_t)stride;
	gx->result_labelled = n_label;
	gx->result_stride = stride;
	gx->result_nodes = true;
	return SDT_OK;
}

// ---- the phases in the node-index form IX (instantiated for Ix32 in sdt_gpu_graph.hip, for Ix64 in sdt_gpu_graph64.hip; the entry
// points of sdt_gpu_graph.hip check their arguments and the context's state first)
namespace sdti {

template <class IX>
int tip_walks_labelled(sdt_ctx *c, IX ix, int thin, int cut_len, uint64_t *n_records)
{
	using T = typename IX::T;
	const GraphView v = sdti::graph_view(c);
	const uint64_t nn = *v.idx_n;
	Scratch S;
	T *parent;
	unsigned long long *d_cur, h = 0;
	GCHK(S.alloc(&parent, (nn + 1) * sizeof(T))); GCHK(S.alloc(&d_cur, 8));
	hipLaunchKernelGGL(k_uf_init<IX>, dim3(sdti::scan_grid(v.cu_count, nn + 1)), dim3(TPB), 0, v.stream, parent, nn + 1, ix);
	const int g = sdti::scan_grid(v.cu_count, v.slots);
	uint64_t cap = nn / 8 + 4096;
	uint64_t *d_rec = nullptr;
	ApBuf B;
	for (int attempt = 0; attempt < 2; attempt++) {
		// the dead ends first (a list of slots), then one lane per walk
		unsigned long long *d_list, *d_lcur, n_lchunks = 0;
		const unsigned long long l_chunks = cap / (AP_CH - 64) + 1 + (unsigned long long)v.cu_count * 8 * (TPB / 64);
		GCHK(S.alloc(&d_list, l_chunks * AP_CH * 8)); GCHK(S.alloc(&d_lcur, 8));
		GCHK(hipMemsetAsync(d_lcur, 0, 8, v.stream));
		int rc = ap_alloc(S, v, B, cap, 3);
		if (rc != SDT_OK) return rc;
		LAUNCH_NW(v, k_tip_starts, g, thin, d_list, ApOut{d_lcur, l_chunks, nullptr, d_list});
		GCHK(hipGetLastError());
		GCHK(hipMemcpyAsync(&n_lchunks, d_lcur, 8, hipMemcpyDeviceToHost, v.stream));
		GCHK(hipStreamSynchronize(v.stream));
		if (n_lchunks <= l_chunks) {
			const unsigned long long n_list = n_lchunks * AP_CH;
			LAUNCH_NW(v, k_tip_walks_list, sdti::scan_grid(v.cu_count, n_list), *v.d_idx, v.K, thin, cut_len, d_list, n_list, v.d_stats, B.chunks, 3, ap_out(B));
			GCHK(hipGetLastError());
			GCHK(hipMemcpyAsync(&h, B.cursor, 8, hipMemcpyDeviceToHost, v.stream));
			rc = sdti::sync_stats(c);
			if (rc != SDT_OK) return fail(SDT_ESTATE, "sdt_gpu_tip_walks_labelled: %llu walks left the graph", (unsigned long long)v.h_stats->probe_fail);
		}
		(void)hipFree(S.release(d_list)); (void)hipFree(S.release(d_lcur));
		if (n_lchunks <= l_chunks && h <= B.cap_chunks) break;
		if (attempt) return fail(SDT_ESTATE, "sdt_gpu_tip_walks_labelled: the number of walks changed between two runs");
		ap_free(S, B);
		cap = (n_lchunks > l_chunks ? n_lchunks : h) * AP_CH;          // (every walk has a start: the starts bound the records)
	}
	{
		uint64_t n_rec = 0;
		const int rc = ap_compact(S, v, B, h, h, &d_rec, &n_rec, nullptr);
		if (rc != SDT_OK) return rc;
		GCHK(hipStreamSynchronize(v.stream));
		ap_free(S, B);
		h = n_rec;
	}
	// components: removeSingleTips -- tip and end node of every walk; removeMinorTips -- the chains a walk can cross
	if (thin) {
		if (h) hipLaunchKernelGGL(k_uf_records<IX>, dim3(sdti::scan_grid(v.cu_count, h)), dim3(TPB), 0, v.stream, parent, d_rec, (uint64_t)h, 3, 1, 2, 0, ix);
	} else {
		// every live port of every node that is neither linear nor deleted: listed, then walked one lane per port
		unsigned long long *d_list = nullptr, *d_lcur, n_lchunks = 0;
		GCHK(S.alloc(&d_lcur, 8));
		unsigned long long l_chunks = nn / (AP_CH - 64) + 1 + (unsigned long long)v.cu_count * 8 * (TPB / 64);
		for (int attempt = 0; attempt < 2; attempt++) {
			GCHK(S.alloc(&d_list, l_chunks * AP_CH * 8));
			GCHK(hipMemsetAsync(d_lcur, 0, 8, v.stream));
			LAUNCH_NW(v, k_port_starts, g, d_list, ApOut{d_lcur, l_chunks, nullptr, d_list});
			GCHK(hipGetLastError());
			GCHK(hipMemcpyAsync(&n_lchunks, d_lcur, 8, hipMemcpyDeviceToHost, v.stream));
			GCHK(hipStreamSynchronize(v.stream));
			if (n_lchunks <= l_chunks) break;
			if (attempt) return fail(SDT_ESTATE, "sdt_gpu_tip_walks_labelled: the number of ports changed between two runs");
			(void)hipFree(S.release(d_list));
			l_chunks = n_lchunks;
		}
		const unsigned long long n_list = n_lchunks * AP_CH;
		if (n_list) LAUNCH_NW_IX(v, k_port_union_list, IX, sdti::scan_grid(v.cu_count, n_list), *v.d_idx, v.K, cut_len, d_list, n_list, parent, v.d_stats, ix);
		GCHK(hipGetLastError());
		GCHK(hipStreamSynchronize(v.stream));
		(void)hipFree(S.release(d_list)); (void)hipFree(S.release(d_lcur));
	}
	GCHK(hipGetLastError());
	int rc = sdti::sync_stats(c);
	if (rc != SDT_OK) return fail(SDT_ESTATE, "sdt_gpu_tip_walks_labelled: %llu chains left the graph", (unsigned long long)v.h_stats->probe_fail);
	rc = label_sort_keep<IX>(c, v, ix, parent, d_rec, h, h, 3);
	if (rc != SDT_OK) return rc;
	*n_records = h;
	return SDT_OK;
}

template <class IX>
int minor_out_labelled(sdt_ctx *c, IX ix, double threshold, uint64_t *n_junctions, uint64_t *n_records)
{
	using T = typename IX::T;
	const GraphView v = sdti::graph_view(c);
	const uint64_t nn = *v.idx_n;
	Scratch S;
	T *parent;
	uint8_t *d_need, *d_flag;
	unsigned long long *d_cur, h1 = 0, h2 = 0;
	GCHK(S.alloc(&parent, (nn + 1) * sizeof(T))); GCHK(S.alloc(&d_cur, 8));
	GCHK(S.alloc(&d_need, nn + 1)); GCHK(S.alloc(&d_flag, nn + 1));
	hipLaunchKernelGGL(k_uf_init<IX>, dim3(sdti::scan_grid(v.cu_count, nn + 1)), dim3(TPB), 0, v.stream, parent, nn + 1, ix);
	const int g = sdti::scan_grid(v.cu_count, v.slots);
	// (one node in twenty has a record in the transcriptome jobs measured; the chunks add a third: room for one in sixteen, a second
	// attempt with what the first one counted otherwise)
	uint64_t cap = nn / 16 + 4096;
	uint64_t *d_rec = nullptr;
	ApBuf B;
	for (int attempt = 0; attempt < 2; attempt++) {
		int rc = ap_alloc(S, v, B, cap, 14);
		if (rc != SDT_OK) return rc;
		GCHK(hipMemsetAsync(d_need, 0, nn + 1, v.stream));
		GCHK(hipMemsetAsync(d_flag, 0, nn + 1, v.stream));
		LAUNCH_NW_IX(v, k_minor_out_junctions, IX, g, *v.d_idx, v.K, threshold, d_need, d_flag, B.chunks, 0ULL, (unsigned long long *)nullptr, v.d_stats, 14, ap_out(B), ix);
		GCHK(hipGetLastError());
		GCHK(hipMemcpyAsync(&h1, B.cursor, 8, hipMemcpyDeviceToHost, v.stream));
		LAUNCH_NW_IX(v, k_minor_out_candidates, IX, g, *v.d_idx, v.K, d_need, d_flag, B.chunks, 0ULL, (unsigned long long *)nullptr, v.d_stats, 14, ap_out(B), ix);
		GCHK(hipGetLastError());
		GCHK(hipMemcpyAsync(&h2, B.cursor, 8, hipMemcpyDeviceToHost, v.stream));
		rc = sdti::sync_stats(c);
		if (rc != SDT_OK) return fail(SDT_ESTATE, "sdt_gpu_minor_out_labelled: %llu links point at k-mers that are not nodes", (unsigned long long)v.h_stats->probe_fail);
		if (h2 <= B.cap_chunks) break;
		if (attempt) return fail(SDT_ESTATE, "sdt_gpu_minor_out_labelled: the number of records changed between two runs");
		ap_free(S, B);
		cap = h2 * AP_CH;
	}
	{
		// (h1, h2 are chunk counts so far: the junctions' chunks come first, packing keeps the chunk order)
		uint64_t n_rec = 0, n_junc = 0;
		const int rc = ap_compact(S, v, B, h2, h1, &d_rec, &n_rec, &n_junc);
		if (rc != SDT_OK) return rc;
		GCHK(hipStreamSynchronize(v.stream));
		ap_free(S, B);
		h1 = n_junc; h2 = n_rec;
	}
	// a visit reads and writes its junction, the junction's neighbours and the neighbours of those it may cut: unite every record's
	// node with its eight neighbours (junction records and the records of the neighbours to cut alike)
	if (h2) hipLaunchKernelGGL(k_uf_records<IX>, dim3(sdti::scan_grid(v.cu_count, h2)), dim3(TPB), 0, v.stream, parent, d_rec, (uint64_t)h2, 14, 1, 9, 1, ix);
	GCHK(hipGetLastError());
	const int rc = label_sort_keep<IX>(c, v, ix, parent, d_rec, h2, h1, 14);
	if (rc != SDT_OK) return rc;
	*n_junctions = h1;
	*n_records = h2;
	return SDT_OK;
}

// removeMinorOut's commit on the records sdt_gpu_minor_out_labelled left on the device (they stay there: sdt_gpu_fetch_records still
// works afterwards).  One lane walks a component, at about a microsecond per dependent access (most are first touches of a node:
// HBM latency); components of more than max_component visits are left alone -- their records wait for sdt_gpu_fetch_skipped, the
// host's threads are the better place for them.  Two halves, so that the host can work on those while the device walks the rest:
// _begin finds the components, gathers the records of the long ones and LAUNCHES the visits; _finish waits, re-marks and lists
// the written nodes.
static void mo_pending_free(sdti::GraphExt *gx)
{
	for (void **q : {(void **)&gx->mo_dirty, (void **)&gx->mo_cnt, (void **)&gx->mo_recidx, (void **)&gx->mo_cstart})
		if (*q) { (void)hipFree(*q); *q = nullptr; }
	gx->mo_pending = false;
}

template <class IX>
int minor_out_commit_begin(sdt_ctx *c, IX ix, double threshold, uint64_t max_component, uint64_t *largest, uint64_t *n_skipped, uint64_t *n_skipped_records)
{
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	const uint64_t nn = gx->n_nodes, nj = gx->result_labelled, nr = gx->result_words / 14;
	*largest = *n_skipped = *n_skipped_records = 0;
	const CallTimer T;
	auto tick = [&](const char *what) { if (T.on) { (void)hipStreamSynchronize(v.stream); T.tick(what); } };      // (waits for the stream)
	if (gx->mo_pending) { (void)hipStreamSynchronize(v.stream); mo_pending_free(gx); }
	if (gx->d_wnode) { (void)hipFree(gx->d_wnode); gx->d_wnode = nullptr; }
	if (gx->d_wl) { (void)hipFree(gx->d_wl); gx->d_wl = nullptr; }
	if (gx->d_wr) { (void)hipFree(gx->d_wr); gx->d_wr = nullptr; }
	if (gx->d_skipped) { (void)hipFree(gx->d_skipped); gx->d_skipped = nullptr; }
	gx->n_written = gx->n_skipped = 0;
	Scratch S;
	uint32_t *flag, *rank, *cstart, *recidx;
	uint8_t *dirty;
	unsigned long long *d_cnt, h_largest = 0;                    // d_cnt: off, errors, marked, written, largest
	GCHK(S.alloc(&d_cnt, 5 * 8));
	GCHK(hipMemsetAsync(d_cnt, 0, 5 * 8, v.stream));
	GCHK(S.alloc(&recidx, (nn + 1) * 4)); GCHK(S.alloc(&dirty, nn + 1));
	GCHK(hipMemsetAsync(dirty, 0, nn + 1, v.stream));
	tick("commit: buffers");
	if (!nj) {                                                   // nothing to visit: _finish reports zeros
		GCHK(S.alloc(&cstart, 8));
		gx->mo_dirty = (uint8_t *)S.release(dirty); gx->mo_cnt = (unsigned long long *)S.release(d_cnt);
		gx->mo_recidx = (uint32_t *)S.release(recidx); gx->mo_cstart = (uint32_t *)S.release(cstart);
		gx->mo_pending = true;
		return SDT_OK;
	}
	uint64_t ncomp = 0;
	{
	// (the temporaries of this block are let go BEFORE the visits are launched: freeing a block waits for the device, and at the
	// end of the call that would be a wait for the visits -- the host would start on the long components a quarter of a second late)
	Scratch T;
	GCHK(T.alloc(&flag, (nj + 1) * 4)); GCHK(T.alloc(&rank, (nj + 1) * 4));
	hipLaunchKernelGGL(k_mo_comp_flags, dim3(sdti::scan_grid(v.cu_count, nj + 1)), dim3(TPB), 0, v.stream, gx->d_result, nj, 14, flag);
	GCHK(hipGetLastError());
	int rc = exclusive_scan<uint32_t>(v, flag, rank, nj + 1);                   // rank[nj] = number of components
	if (rc != SDT_OK) return rc;
	uint32_t ncomp32 = 0;
	GCHK(hipMemcpyAsync(&ncomp32, rank + nj, 4, hipMemcpyDeviceToHost, v.stream));
	GCHK(hipStreamSynchronize(v.stream));
	ncomp = ncomp32;
	GCHK(S.alloc(&cstart, (ncomp + 1) * 4));
	hipLaunchKernelGGL(k_mo_comp_starts, dim3(sdti::scan_grid(v.cu_count, nj)), dim3(TPB), 0, v.stream, flag, rank, nj, cstart);
	GCHK(hipGetLastError());
	const uint32_t nj32 = (uint32_t)nj;
	GCHK(hipMemcpyAsync(cstart + ncomp, &nj32, 4, hipMemcpyHostToDevice, v.stream));
	hipLaunchKernelGGL(k_mo_comp_largest, dim3(sdti::scan_grid(v.cu_count, ncomp)), dim3(TPB), 0, v.stream, cstart, ncomp, d_cnt + 4);
	GCHK(hipGetLastError());
	GCHK(hipMemcpyAsync(&h_largest, d_cnt + 4, 8, hipMemcpyDeviceToHost, v.stream));
	GCHK(hipMemsetAsync(recidx, 0, (nn + 1) * 4, v.stream));
	hipLaunchKernelGGL(k_mo_recidx<IX>, dim3(sdti::scan_grid(v.cu_count, nr)), dim3(TPB), 0, v.stream, gx->d_result, nr, 14, recidx, ix);
	GCHK(hipGetLastError());
	GCHK(hipStreamSynchronize(v.stream));
	*largest = h_largest;
	tick("commit: components + record index");
	if (h_largest > max_component) {
		// the records of the components that are left alone: their junction records in order, then the records of the neighbours
		// they may cut (the host's commit finds the neighbours of a cut node there instead of looking them up)
		uint32_t *sel, *pos, *size_of, *sel2, *pos2, nsk = 0, nsk2 = 0;
		GCHK(T.alloc(&sel, (nj + 1) * 4)); GCHK(T.alloc(&pos, (nj + 1) * 4));
		hipLaunchKernelGGL(k_mo_skipped_sel, dim3(sdti::scan_grid(v.cu_count, nj + 1)), dim3(TPB), 0, v.stream, flag, rank, cstart, nj, max_component, sel);
		GCHK(hipGetLastError());
		rc = exclusive_scan<uint32_t>(v, sel, pos, nj + 1);
		if (rc != SDT_OK) return rc;
		GCHK(hipMemcpyAsync(&nsk, pos + nj, 4, hipMemcpyDeviceToHost, v.stream));
		const uint64_t nc = nr - nj;
		GCHK(T.alloc(&size_of, (nn + 1) * 4)); GCHK(T.alloc(&sel2, (nc + 1) * 4)); GCHK(T.alloc(&pos2, (nc + 1) * 4));
		GCHK(hipMemsetAsync(size_of, 0, (nn + 1) * 4, v.stream));
		hipLaunchKernelGGL(k_mo_label_sizes<IX>, dim3(sdti::scan_grid(v.cu_count, ncomp)), dim3(TPB), 0, v.stream, gx->d_result, 14, cstart, ncomp, size_of, ix);
		GCHK(hipGetLastError());
		hipLaunchKernelGGL(k_mo_skipped_sel2<IX>, dim3(sdti::scan_grid(v.cu_count, nc + 1)), dim3(TPB), 0, v.stream, gx->d_result, 14, nj, nr, size_of, max_component, sel2, ix);
		GCHK(hipGetLastError());
		rc = exclusive_scan<uint32_t>(v, sel2, pos2, nc + 1);
		if (rc != SDT_OK) return rc;
		GCHK(hipMemcpyAsync(&nsk2, pos2 + nc, 4, hipMemcpyDeviceToHost, v.stream));
		GCHK(hipStreamSynchronize(v.stream));
		uint64_t *sk;
		GCHK(S.alloc(&sk, ((uint64_t)nsk + nsk2 + 1) * 14 * 8));
		hipLaunchKernelGGL(k_mo_skipped_gather, dim3(sdti::scan_grid(v.cu_count, nj * 14)), dim3(TPB), 0, v.stream, gx->d_result, 14, sel, pos, nj, sk);
		GCHK(hipGetLastError());
		if (nc) hipLaunchKernelGGL(k_mo_skipped_gather, dim3(sdti::scan_grid(v.cu_count, nc * 14)), dim3(TPB), 0, v.stream, gx->d_result + nj * 14, 14, sel2, pos2, nc, sk + (uint64_t)nsk * 14);
		GCHK(hipGetLastError());
		GCHK(hipStreamSynchronize(v.stream));                // (sdt_gpu_fetch_skipped copies on the other stream)
		gx->d_skipped = (uint64_t *)S.release(sk);
		gx->n_skipped = (uint64_t)nsk + nsk2;
		*n_skipped = nsk;
		*n_skipped_records = (uint64_t)nsk + nsk2;
		tick("commit: long components gathered");
	}
	}
	// the visits and the re-marking: launched, not waited for
	{
		const uint64_t blocks = (ncomp + TPB - 1) / TPB;
		const int g = (int)(blocks < (uint64_t)v.cu_count * 32 ? (blocks ? blocks : 1) : (uint64_t)v.cu_count * 32);
		LAUNCH_NW_IX(v, k_mo_commit, IX, g, gx->d_slot_of, v.K, threshold, gx->d_result, 14, cstart, ncomp, recidx, dirty, d_cnt, max_component, ix);
		GCHK(hipGetLastError());
	}
	LAUNCH_NW(v, k_mo_mark, sdti::scan_grid(v.cu_count, nn), gx->d_slot_of, nn, dirty, d_cnt);
	GCHK(hipGetLastError());
	gx->mo_dirty = (uint8_t *)S.release(dirty); gx->mo_cnt = (unsigned long long *)S.release(d_cnt);
	gx->mo_recidx = (uint32_t *)S.release(recidx); gx->mo_cstart = (uint32_t *)S.release(cstart);
	gx->mo_pending = true;
	return SDT_OK;
}

// ---- kmer2edges on the device (node2edge.c:46-561) ----------------------------------------------------------------------
template <class IX>
int build_edges(sdt_ctx *c, IX ix, uint64_t *n_edges, uint64_t *num_ed, uint64_t *n_bases)
{
	using T = typename IX::T;
	const GraphView v = sdti::graph_view(c);
	sdti::GraphExt *gx = ext_of(v);
	const uint64_t n = gx->n_nodes;
	if (gx->d_result) { (void)hipFree(gx->d_result); gx->d_result = nullptr; gx->result_words = 0; }
	if (gx->d_seq) { (void)hipFree(gx->d_seq); gx->d_seq = nullptr; gx->seq_bytes = 0; }
	if (gx->d_pw) { (void)hipFree(gx->d_pw); gx->d_pw = nullptr; gx->pw_n = 0; }
	Scratch S;
	const uint64_t m = n ? n : 1;
	uint32_t *flag;
	T *srank, *start_node;
	uint64_t *pw;
	unsigned int *d_asym;
	GCHK(S.alloc(&flag, (m + 1) * 4)); GCHK(S.alloc(&srank, (m + 1) * sizeof(T))); GCHK(S.alloc(&pw, m * 8)); GCHK(S.alloc(&d_asym, 4));
	GCHK(hipMemsetAsync(flag, 0, (m + 1) * 4, v.stream));
	GCHK(hipMemsetAsync(d_asym, 0, 4, v.stream));
	LAUNCH_NW(v, k_edge_starts, sdti::scan_grid(v.cu_count, m), gx->d_slot_of, n, flag, pw);
	GCHK(hipGetLastError());
	int rc = exclusive_scan<T, uint32_t>(v, flag, srank, n + 1);               // srank[n] = number of start nodes
	if (rc != SDT_OK) return rc;
	T nstarts = 0;
	GCHK(hipMemcpy(&nstarts, srank + n, sizeof(T), hipMemcpyDeviceToHost));
	const uint64_t nports = (uint64_t)nstarts * 8;
	PortRec *ports;
	uint32_t *w_edge, *w_id, *e_scan, *id_scan;
	uint64_t *w_len, *len_scan;
	GCHK(S.alloc(&start_node, ((uint64_t)nstarts + 1) * sizeof(T))); GCHK(S.alloc(&ports, (nports + 1) * sizeof(PortRec)));
	GCHK(S.alloc(&w_edge, (nports + 1) * 4)); GCHK(S.alloc(&w_id, (nports + 1) * 4)); GCHK(S.alloc(&w_len, (nports + 1) * 8));
	GCHK(S.alloc(&e_scan, (nports + 1) * 4)); GCHK(S.alloc(&id_scan, (nports + 1) * 4)); GCHK(S.alloc(&len_scan, (nports + 1) * 8));
	GCHK(hipMemsetAsync(w_edge + nports, 0, 4, v.stream)); GCHK(hipMemsetAsync(w_id + nports, 0, 4, v.stream)); GCHK(hipMemsetAsync(w_len + nports, 0, 8, v.stream));
	hipLaunchKernelGGL(k_edge_start_nodes<IX>, dim3(sdti::scan_grid(v.cu_count, m)), dim3(TPB), 0, v.stream, flag, srank, n, start_node, ix);
	if (nports) LAUNCH_NW_IX(v, k_edge_ports_ordered, IX, sdti::scan_grid(v.cu_count, nports), *v.d_idx, gx->d_slot_of, start_node, nports, v.K, n + 1, ports, v.d_stats, ix);
	GCHK(hipGetLastError());
	rc = sdti::sync_stats(c);
	if (rc != SDT_OK) return fail(SDT_ESTATE, "sdt_gpu_build_edges: %llu chains leave the graph or never end", (unsigned long long)v.h_stats->probe_fail);
	if (nports) hipLaunchKernelGGL(k_edge_emit<IX>, dim3(sdti::scan_grid(v.cu_count, nports)), dim3(TPB), 0, v.stream, ports, start_node, flag, srank, nports, w_edge, w_id, w_len, d_asym, ix);
	GCHK(hipGetLastError());
	unsigned int asym = 0;
	GCHK(hipMemcpyAsync(&asym, d_asym, 4, hipMemcpyDeviceToHost, v.stream));
	GCHK(hipStreamSynchronize(v.stream));
	if (asym) return fail(SDT_ESTATE, "sdt_gpu_build_edges: a chain does not lead back to the port it was entered from (build the edges sequentially)");
	rc = exclusive_scan<uint32_t>(v, w_edge, e_scan, nports + 1);
	if (rc == SDT_OK) rc = exclusive_scan<uint32_t>(v, w_id, id_scan, nports + 1);
	if (rc == SDT_OK) rc = exclusive_scan<uint64_t>(v, w_len, len_scan, nports + 1);
	if (rc != SDT_OK) return rc;
	uint32_t ne = 0, ids = 0;
	uint64_t nb = 0;
	GCHK(hipMemcpy(&ne, e_scan + nports, 4, hipMemcpyDeviceToHost));
	GCHK(hipMemcpy(&ids, id_scan + nports, 4, hipMemcpyDeviceToHost));
	GCHK(hipMemcpy(&nb, len_scan + nports, 8, hipMemcpyDeviceToHost));
	const int RW = 4 + 2 * v.nw;
	uint64_t *erec;
	unsigned char *seq;
	GCHK(S.alloc(&erec, ((uint64_t)ne + 1) * RW * 8)); GCHK(S.alloc(&seq, nb + 16));
	if (nports) LAUNCH_NW_IX(v, k_edge_stamp, IX, sdti::scan_grid(v.cu_count, nports), *v.d_idx, gx->d_slot_of, v.K, ports, start_node, nports, w_edge, e_scan, id_scan, len_scan, pw, seq, erec, v.d_stats, ix);
	GCHK(hipGetLastError());
	rc = sdti::sync_stats(c);
	if (rc != SDT_OK) return fail(SDT_ESTATE, "sdt_gpu_build_edges: %llu chains changed between the two walks", (unsigned long long)v.h_stats->probe_fail);
	gx->d_result = (uint64_t *)S.release(erec);
	gx->result_words = (uint64_t)ne * RW;
	gx->result_nodes = false;
	gx->d_seq = (unsigned char *)S.release(seq);
	gx->seq_bytes = nb;
	gx->d_pw = (uint64_t *)S.release(pw);
	gx->pw_n = n;
	*n_edges = ne;
	*num_ed = ids;
	*n_bases = nb;
	return SDT_OK;
}

// ---- numbering: the layout's order and the node index of every slot ----------------------------------------------------
// the visiting order from the settled tables of the layout replay: the occupied slots ranked over all sets (ranks of the form's width),
// order[rank] = rank of the key in the sorted key array
template <class IX>
int layout_order(const GraphView &v, const RpSet *d_sets, const unsigned long long *d_pre, int p, const unsigned long long *tab, const uint32_t *d_occ,
                 uint64_t slot_total, uint64_t *d_order)
{
	using T = typename IX::T;
	Scratch S;
	T *d_rank;
	GCHK(S.alloc(&d_rank, (slot_total + 1) * sizeof(T)));
	const int rc = exclusive_scan<T, uint32_t>(v, d_occ, d_rank, slot_total);
	if (rc != SDT_OK) return rc;
	hipLaunchKernelGGL(k_rp_order<T>, dim3(sdti::scan_grid(v.cu_count, slot_total ? slot_total : 1)), dim3(TPB), 0, v.stream, d_sets, d_pre, p, tab, d_occ, d_rank, d_order);
	GCHK(hipGetLastError());
	GCHK(hipStreamSynchronize(v.stream));
	return SDT_OK;
}

// idx[slot of the node at visiting position i] = base + i (order[i] = its rank in sval), slot_of[i] = that slot
template <class IX>
int layout_number(const GraphView &v, IX ix, const uint64_t *sval, const uint64_t *order, uint64_t n, uint64_t *d_idx, uint64_t *d_slot_of)
{
	hipLaunchKernelGGL(k_layout_apply<IX>, dim3(sdti::scan_grid(v.cu_count, n ? n : 1)), dim3(TPB), 0, v.stream, sval, order, n, d_idx, d_slot_of, v.d_stats, ix);
	GCHK(hipGetLastError());
	return SDT_OK;
}

// the same from the host's keys in visiting order (sdt_gpu_set_node_index)
template <class IX>
int set_index(const GraphView &v, IX ix, const uint64_t *d_keys, uint64_t n)
{
	LAUNCH_NW_IX(v, k_set_index, IX, sdti::scan_grid(v.cu_count, n ? n : 1), d_keys, n, *v.d_idx, v.d_stats, ix);
	GCHK(hipGetLastError());
	return SDT_OK;
}

// the host's look-up index (entries E = node position + 1) into d_index, zeroed by the caller
template <class IX, class E>
int host_index(const GraphView &v, IX ix, E *d_index, uint64_t index_mask)
{
	const int g = sdti::scan_grid(v.cu_count, v.slots);
	if (v.nw == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_build_host_index<1, IX, E>), dim3(g), dim3(TPB), 0, v.stream, sdti::table_of<1>(v), *v.d_idx, d_index, index_mask, ix);
	else if (v.nw == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_build_host_index<2, IX, E>), dim3(g), dim3(TPB), 0, v.stream, sdti::table_of<2>(v), *v.d_idx, d_index, index_mask, ix);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_build_host_index<4, IX, E>), dim3(g), dim3(TPB), 0, v.stream, sdti::table_of<4>(v), *v.d_idx, d_index, index_mask, ix);
	GCHK(hipGetLastError());
	return SDT_OK;
}

}  // namespace sdti

// the Ix64 instantiations live in sdt_gpu_graph64.hip (a translation unit of their own: the parallel build does not get longer)
#ifndef SDT_GRAPH_WIDE_UNIT
extern template int sdti::tip_walks_labelled<Ix64>(sdt_ctx *, Ix64, int, int, uint64_t *);
extern template int sdti::minor_out_labelled<Ix64>(sdt_ctx *, Ix64, double, uint64_t *, uint64_t *);
extern template int sdti::minor_out_commit_begin<Ix64>(sdt_ctx *, Ix64, double, uint64_t, uint64_t *, uint64_t *, uint64_t *);
extern template int sdti::build_edges<Ix64>(sdt_ctx *, Ix64, uint64_t *, uint64_t *, uint64_t *);
extern template int sdti::layout_order<Ix64>(const GraphView &, const RpSet *, const unsigned long long *, int, const unsigned long long *, const uint32_t *, uint64_t, uint64_t *);
extern template int sdti::layout_number<Ix64>(const GraphView &, Ix64, const uint64_t *, const uint64_t *, uint64_t, uint64_t *, uint64_t *);
extern template int sdti::set_index<Ix64>(const GraphView &, Ix64, const uint64_t *, uint64_t);
extern template int sdti::host_index<Ix64, unsigned int>(const GraphView &, Ix64, unsigned int *, uint64_t);
extern template int sdti::host_index<Ix64, unsigned long long>(const GraphView &, Ix64, unsigned long long *, uint64_t);
#endif
