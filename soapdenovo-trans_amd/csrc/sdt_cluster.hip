// sdt_cluster.hip -- reads clustered by connected component of the counted k-mer graph (the rule: include/sdt_gpu.h).  cluster_begin
// builds the clustering = k_cl_init, k_cl_unite, k_cl_flatten, a radix sort of the roots by key, k_cl_rank, k_cl_label
// (sdt_cluster_kernels.cuh); the forms over reads = k_cl_reads and, for the kept reads, k_cl_units.  Nothing here writes the table, the
// kept reads or a cache of the context: the count's high half is read from aux itself.  The labels are one 32-bit word per slot of the
// context's own, from cluster_begin to cluster_end, tied to the state of the table they were built on as the assembly tally is --
// search_cache_drop (sdt_ctx.hpp) marks them stale wherever counts or slots change, and stale labels are refused.  State rules and
// staging are those of the read stages (sdt_readstage.hpp); there is no strip of LDS and so no limit on the length of a read.
#include "sdt_readstage.hpp"
#include "sdt_cluster_kernels.cuh"
#include <rocprim/rocprim.hpp>
#include <cstddef>

static_assert(sizeof(sdt_read_cluster) == sizeof(ReadCluster) && offsetof(sdt_read_cluster, cluster) == 12 && offsetof(sdt_read_cluster, verdict) == 20,
              "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_cluster_comp) == sizeof(ClusterComp) && offsetof(sdt_cluster_comp, nodes) == 8, "include/sdt_gpu.h and the kernel agree");
static_assert(SDT_CLUSTER_NONE == CL_NONE, "include/sdt_gpu.h and the kernel agree");

// labels that the other calls may use: begun, and on the table as it was then
static int cluster_open(const sdt_ctx *c, const char *what)
{
	if (!c->cl.open)
		return fail(SDT_ESTATE, "%s: no clustering: call sdt_gpu_cluster_begin first", what);
	if (c->cl.stale || c->cl.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_cluster_begin", what);
	return SDT_OK;
}

static void cluster_free(sdt_ctx *c)
{
	if (c->cl.label) (void)hipFree(c->cl.label);
	c->cl = sdt_ctx::Clustering();
}

// the largest table that 32-bit labels serve: a slot's index and 0xFFFFFFFF for "none" (SDT_CLUSTER_MAX_SLOTS: test hook -- a smaller
// figure, so that the refusal is reached on a table a test can afford; read at every begin)
static uint64_t label_slots_max()
{
	const long long forced = sdt_test_env("SDT_CLUSTER_MAX_SLOTS") ? atoll(sdt_test_env("SDT_CLUSTER_MAX_SLOTS")) : 0;
	return forced > 0 ? (uint64_t)forced : 0xFFFFFFFEULL;
}

static int cluster_params_ok(const sdt_cluster_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_cluster_params is NULL");
	if (p->flags)
		return fail(SDT_EINVAL, "sdt_cluster_params.flags = 0x%x: no flag is defined", p->flags);
	if (p->min_link < 1 || p->min_link > 63)
		return fail(SDT_EINVAL, "sdt_cluster_params.min_link = %u: 1 to 63 (a link counter saturates at 63)", p->min_link);
	const uint32_t mc = p->min_count > 1 ? p->min_count : 1u;
	if (p->max_count && p->max_count < mc)
		return fail(SDT_EINVAL, "sdt_cluster_params.max_count = %u is below min_count = %u: 0 (no upper bound) or at least that", p->max_count, mc);
	return SDT_OK;
}

// the roots sorted by key: stable passes from the least significant word; *sorted: the buffer that holds them in the end
static int sort_roots(sdt_ctx *c, uint64_t n, DevBuf &r_a, DevBuf &r_b, DevBuf &k_a, DevBuf &k_b, uint32_t **sorted)
{
	size_t tb = 0;
	HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, (uint64_t *)k_a.p, (uint64_t *)k_b.p, (uint32_t *)r_a.p, (uint32_t *)r_b.p, (size_t)n, 0, 64, c->stream));
	DevBuf d_tmp;
	int rc = d_tmp.get(tb, "sdt_gpu_cluster_begin: sort");
	if (rc != SDT_OK) return rc;
	uint32_t *in = (uint32_t *)r_a.p, *out = (uint32_t *)r_b.p;
	const int g = scan_grid(c, n);
	hipError_t e = hipSuccess;
	for (int w = c->nw - 1; w >= 0 && e == hipSuccess; w--) {
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_cl_sortkey<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), (const uint32_t *)in, n, w, (uint64_t *)k_a.p);
		});
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

// checked arguments, the context entered; on failure the caller frees the labels
static int cluster_build(sdt_ctx *c, const ClusterRule &rule, uint64_t info[8])
{
	const uint64_t slots = c->slots;
	DevBuf d_work, d_ctr, d_ra, d_rb, d_ka, d_kb, d_keys, d_comp;
	int rc = d_work.get(slots * sizeof(uint32_t), "sdt_gpu_cluster_begin: 4 bytes per table slot of working memory");
	if (rc == SDT_OK) rc = d_ctr.get(CL_COUNTERS * sizeof(unsigned long long), "sdt_gpu_cluster_begin: counters");
	if (rc != SDT_OK) return rc;
	unsigned long long *ctr = (unsigned long long *)d_ctr.p, h[CL_COUNTERS] = {0, 0, 0, 0};
	uint32_t *label = c->cl.label, *work = (uint32_t *)d_work.p;
	const int g = scan_grid(c, slots);
	HIPCHK(hipMemsetAsync(ctr, 0, CL_COUNTERS * sizeof(unsigned long long), c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_cl_init<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), rule, label, ctr);
		hipLaunchKernelGGL(k_cl_unite<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, label, ctr);
	});
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = hipStreamSynchronize(c->stream);             // (the buffers go when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	const uint64_t n_live = h[CL_N_LIVE], n_ends = h[CL_N_ENDS], n_dead = h[CL_N_DEAD];
	rc = d_ra.get(n_live * sizeof(uint32_t), "sdt_gpu_cluster_begin: the roots");
	if (rc != SDT_OK) return rc;
	hipLaunchKernelGGL(k_cl_flatten, dim3(g), dim3(TPB), 0, c->stream, label, slots, work, (uint32_t *)d_ra.p, n_live, ctr);
	e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream);
	e2 = hipStreamSynchronize(c->stream);
	HIPCHK(e);
	HIPCHK(e2);
	const uint64_t n = h[CL_N_ROOTS];
	if (n > n_live)
		return fail(SDT_ESTATE, "sdt_gpu_cluster_begin: %llu roots among %llu live nodes", (unsigned long long)n, (unsigned long long)n_live);
	c->cl.keys.assign((size_t)n * c->nw, 0);
	c->cl.count_sum.assign((size_t)n, 0);
	c->cl.nodes.assign((size_t)n, 0);
	uint64_t largest = 0, largest_id = 0;
	if (n) {
		rc = d_rb.get(n * sizeof(uint32_t), "sdt_gpu_cluster_begin: the roots");
		if (rc == SDT_OK) rc = d_ka.get(n * sizeof(uint64_t), "sdt_gpu_cluster_begin: sort keys");
		if (rc == SDT_OK) rc = d_kb.get(n * sizeof(uint64_t), "sdt_gpu_cluster_begin: sort keys");
		if (rc == SDT_OK) rc = d_keys.get(n * c->nw * sizeof(uint64_t), "sdt_gpu_cluster_begin: the clusters' k-mers");
		if (rc == SDT_OK) rc = d_comp.get(n * sizeof(ClusterComp), "sdt_gpu_cluster_begin: the clusters");
		uint32_t *sorted = nullptr;
		if (rc == SDT_OK) rc = sort_roots(c, n, d_ra, d_rb, d_ka, d_kb, &sorted);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemsetAsync(d_comp.p, 0, n * sizeof(ClusterComp), c->stream));
		const int gr = scan_grid(c, n);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_cl_rank<NW>, dim3(gr), dim3(TPB), 0, c->stream, table_of<NW>(c), (const uint32_t *)sorted, n, label, (uint64_t *)d_keys.p);
			hipLaunchKernelGGL(k_cl_label<NW>, dim3(g), dim3(TPB), 0, c->stream, table_of<NW>(c), (const uint32_t *)work, label, (ClusterComp *)d_comp.p);
		});
		e = hipGetLastError();
		std::vector<ClusterComp> comp((size_t)n);
		if (e == hipSuccess) e = hipMemcpyAsync(c->cl.keys.data(), d_keys.p, n * c->nw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(comp.data(), d_comp.p, n * sizeof(ClusterComp), hipMemcpyDeviceToHost, c->stream);
		e2 = hipStreamSynchronize(c->stream);
		HIPCHK(e);
		HIPCHK(e2);
		for (uint64_t i = 0; i < n; i++) {
			c->cl.count_sum[i] = comp[i].count_sum;
			c->cl.nodes[i] = comp[i].nodes;
			if (comp[i].nodes > largest) { largest = comp[i].nodes; largest_id = i; }
		}
	}
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = slots;                                   // (slots walked, not k-mers)
	}
	if (info) {
		const uint64_t out[8] = {n_live, n_ends, n, largest, largest_id, n_dead, 0, 0};
		memcpy(info, out, sizeof out);
	}
	return SDT_OK;
}

static int reads_args_ok(uint64_t nreads, int paired)
{
	if (paired && (nreads & 1))
		return fail(SDT_EINVAL, "paired reads: reads 2t and 2t + 1 are mates, %llu reads is an odd number", (unsigned long long)nreads);
	return SDT_OK;
}

// enqueue k_cl_reads for one device-resident batch.  resolve: units of `mates` reads are decided in the kernel, keep (may be NULL) and
// *ctr with them; else every read is walked alone and its record goes to d_rec[out_base + i * out_stride]
static int launch_reads(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, int mates, bool resolve, uint32_t pick_lo,
                        uint32_t pick_hi, ReadCluster *d_rec, uint64_t out_base, uint64_t out_stride, uint8_t *d_keep, unsigned long long *ctr)
{
	const uint64_t nunits = nreads / (uint64_t)mates;
	const int g = wave_grid(c, nunits);
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		if (resolve)
			hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cl_reads<NW, true>), dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, nunits, mates, c->K, table_of<NW>(c),
			                   (const uint32_t *)c->cl.label, pick_lo, pick_hi, d_rec, out_base, out_stride, d_keep, ctr);
		else
			hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cl_reads<NW, false>), dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, nunits, mates, c->K, table_of<NW>(c),
			                   (const uint32_t *)c->cl.label, pick_lo, pick_hi, d_rec, out_base, out_stride, d_keep, ctr);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;                                  // (reads, not k-mers: their lengths are on the device only)
	}
	return SDT_OK;
}

// one dense device-resident batch, checked arguments.  n_kept NULL: enqueued only; else the call waits and adds the reads kept.
static int reads_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, int paired, uint32_t pick_lo, uint32_t pick_hi,
                        ReadCluster *d_rec, uint8_t *d_keep, uint64_t *n_kept)
{
	int rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	unsigned long long *ctr = c->d_cov_flags + 2;
	HIPCHK(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
	rc = launch_reads(c, d_words, d_offs, nreads, paired ? 2 : 1, true, pick_lo, pick_hi, d_rec, 0, 1, d_keep, ctr);
	if (rc != SDT_OK || !n_kept) return rc;
	unsigned long long kept = 0;
	HIPCHK(hipMemcpyAsync(&kept, ctr, sizeof kept, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*n_kept += kept;
	return SDT_OK;
}

extern "C" {

int sdt_gpu_cluster_begin(sdt_ctx *c, const sdt_cluster_params *params, uint64_t info[8])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	int rc = cluster_params_ok(params);
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_cluster_begin");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	if (c->slots > label_slots_max())
		return fail(SDT_EINVAL, "sdt_gpu_cluster_begin: a table of %llu slots: the labels are 32-bit, %llu slots at most", (unsigned long long)c->slots,
		            (unsigned long long)label_slots_max());
	HIPCHK(hipStreamSynchronize(c->stream));                 // (a cluster_reads_device of the clustering that goes may still be running)
	if (c->cl.label && c->cl.slots != c->slots) cluster_free(c);
	c->cl.open = false;
	if (!c->cl.label) {
		const hipError_t e = hipMalloc((void **)&c->cl.label, c->slots * sizeof(uint32_t));
		if (e != hipSuccess) {
			c->cl.label = nullptr;
			return fail(SDT_ENOMEM, "the cluster labels: %llu bytes, four per table slot: %s", (unsigned long long)c->slots * sizeof(uint32_t), hipGetErrorString(e));
		}
	}
	c->cl.slots = c->slots;
	const ClusterRule rule = {params->min_count > 1 ? params->min_count : 1u, params->max_count, params->min_link};
	rc = cluster_build(c, rule, info);
	if (rc != SDT_OK) {
		(void)hipStreamSynchronize(c->stream);
		cluster_free(c);
		return rc;
	}
	c->cl.stale = false;
	c->cl.open = true;
	return SDT_OK;
}

int sdt_gpu_cluster_components(sdt_ctx *c, uint64_t *keys, sdt_cluster_comp *out, uint64_t capacity, uint64_t *n)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n) *n = 0;
	const int rc = cluster_open(c, "sdt_gpu_cluster_components");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const uint64_t total = c->cl.nodes.size(), take = total < capacity ? total : capacity;
	if (n) *n = total;
	if (keys && take) memcpy(keys, c->cl.keys.data(), (size_t)take * c->nw * sizeof(uint64_t));
	if (out)
		for (uint64_t i = 0; i < take; i++) out[i] = sdt_cluster_comp{c->cl.count_sum[i], c->cl.nodes[i], 0};
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_cluster_components: %llu clusters, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	return SDT_OK;
}

int sdt_gpu_cluster_lookup(sdt_ctx *c, const uint64_t *keys, uint64_t n, uint32_t *cluster)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!keys || !cluster)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = cluster_open(c, "sdt_gpu_cluster_lookup");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_cluster_lookup");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const uint64_t piece = chunk_items(PROFILE_CHUNK_READS), most = n < piece ? n : piece;
	DevBuf d_k, d_o;
	rc = d_k.get(most * c->nw * sizeof(uint64_t), "cluster lookup staging");
	if (rc == SDT_OK) rc = d_o.get(most * sizeof(uint32_t), "cluster lookup staging");
	if (rc != SDT_OK) return rc;
	for (uint64_t i0 = 0; i0 < n; i0 += piece) {
		const uint64_t k = n - i0 < piece ? n - i0 : piece;
		HIPCHK(hipMemcpyAsync(d_k.p, keys + i0 * c->nw, k * c->nw * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		const int g = scan_grid(c, k);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_cl_lookup<NW>, dim3(g), dim3(TPB), 0, c->stream, (const uint64_t *)d_k.p, k, c->K, table_of<NW>(c),
			                   (const uint32_t *)c->cl.label, (uint32_t *)d_o.p);
		});
		const hipError_t e = hipGetLastError();
		const hipError_t e2 = e == hipSuccess ? hipMemcpyAsync(cluster + i0, d_o.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
		const hipError_t e3 = hipStreamSynchronize(c->stream);   // (the next piece is staged in the same buffers)
		HIPCHK(e);
		HIPCHK(e2);
		HIPCHK(e3);
	}
	return SDT_OK;
}

int sdt_gpu_cluster_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired, uint32_t pick_lo,
                                 uint32_t pick_hi, void *d_rec, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_rec)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = reads_args_ok(nreads, paired);
	if (rc == SDT_OK) rc = cluster_open(c, "sdt_gpu_cluster_reads");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_cluster_reads");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return reads_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, paired, pick_lo, pick_hi, (ReadCluster *)d_rec,
	                    (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_cluster_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired,
                          uint32_t pick_lo, uint32_t pick_hi, sdt_read_cluster *rec, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !rec)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = reads_args_ok(nreads, paired);
	if (rc == SDT_OK) rc = cluster_open(c, "sdt_gpu_cluster_reads");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_cluster_reads");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	if (in.longest >> 32)
		return fail(SDT_EINVAL, "a read of %llu bases: the fields of sdt_read_cluster are 32-bit", (unsigned long long)in.longest);
	SDT_ENTER(c);
	// (a piece of a paired batch holds whole pairs)
	return staged_records<ReadCluster>(c, packed_words, offsets, nreads, paired ? 2 : 1, "cluster staging", rec, keep, n_kept,
	                                   [&](const StagedPiece &p, ReadCluster *d_r, uint8_t *d_k, uint64_t *kept) {
		return reads_device(c, p.d_words, p.d_offs, p.nr, paired, pick_lo, pick_hi, d_r, d_k, kept);
	});
}

int sdt_gpu_cluster_kept_reads(sdt_ctx *c, const uint64_t *pair_ranges, uint64_t n_ranges, uint32_t pick_lo, uint32_t pick_hi, sdt_read_cluster *rec,
                               uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = cluster_open(c, "sdt_gpu_cluster_kept_reads");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_cluster_kept_reads");
	if (rc != SDT_OK) return rc;
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "rec", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!rec)
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->copy_stream));            // (sdt_gpu_keep_reads uploads on the copy stream)
	// records by ordinal on the device, preset to "no read": every kept batch fills in its own, then the units are decided
	KeptUnits ku(pair_ranges, n_ranges, nord);
	DevBuf d_rec;
	rc = d_rec.get(nord * sizeof(ReadCluster), "cluster records");
	if (rc == SDT_OK) rc = ku.d_segs.get(ku.bytes(), "cluster units");
	if (rc == SDT_OK) rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	unsigned long long *ctr = c->d_cov_flags + 2, kept = 0;
	HIPCHK(hipMemsetAsync(d_rec.p, 0xFF, nord * sizeof(ReadCluster), c->stream));
	HIPCHK(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
	rc = ku.upload(c);
	if (rc != SDT_OK) return rc;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = launch_reads(c, kb.d_words, kb.d_offs, kb.nreads, 1, false, pick_lo, pick_hi, (ReadCluster *)d_rec.p, kb.ord_base, kb.ord_stride, nullptr, ctr);
		if (rc != SDT_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
	}
	hipLaunchKernelGGL(k_cl_units, dim3(scan_grid(c, ku.units)), dim3(TPB), 0, c->stream, (ReadCluster *)d_rec.p, nord, (const UnitStretch *)ku.d_segs.p,
	                   (uint32_t)ku.segs.size(), ku.units, pick_lo, pick_hi, ctr);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(&kept, ctr, sizeof kept, hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (segs may go)
	HIPCHK(e);
	HIPCHK(e2);
	rc = fetch_present<ReadCluster>(rec, d_rec, nord, CL_ABSENT);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

int sdt_gpu_cluster_end(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));                 // (a cluster_reads of the device form may still be running)
	cluster_free(c);
	return SDT_OK;
}

} // extern "C"
