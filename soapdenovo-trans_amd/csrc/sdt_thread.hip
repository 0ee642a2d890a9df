// sdt_thread.hip -- reads threaded through the unitig list (the rule: include/sdt_gpu.h).  unitigs_index = a memset and k_th_label: 8 B
// per table slot that say in which unitig and where the slot's node lies; unitigs_lookup = k_th_lookup; the forms over reads =
// k_th_reads twice with an exclusive scan of the segment counts between (sdt_thread_kernels.cuh), as unitigs_links runs k_ug_links twice.
// Nothing here writes the table, the kept reads, or a cache or tally of the context.  The index belongs to the list it was built from:
// unitigs_free (sdt_unitig.hip) and sdt_gpu_destroy free it, and where the list is stale or gone so is the index.  State rules and
// staging are those of the read stages (sdt_readstage.hpp); there is no strip of LDS and so no limit on the length of a read.
#include "sdt_readstage.hpp"
#include "sdt_thread_kernels.cuh"
#include <rocprim/rocprim.hpp>
#include <cstddef>

static_assert(sizeof(sdt_read_path) == sizeof(ReadPath) && offsetof(sdt_read_path, segs) == 8 && offsetof(sdt_read_path, last) == 20, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_path_seg) == sizeof(PathSeg) && offsetof(sdt_path_seg, read_pos) == 8 && offsetof(sdt_path_seg, kmers) == 16, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_unitig_pos) == sizeof(UnitigPos) && offsetof(sdt_unitig_pos, info) == 8, "include/sdt_gpu.h and the kernel agree");
static_assert(SDT_UNITIG_NONE == TH_NONE, "include/sdt_gpu.h and the kernel agree");

// the list that the index was or will be built from: the messages of the unitig calls (sdt_unitig.hip: unitigs_open)
static int list_open(const sdt_ctx *c, const char *what)
{
	if (!c->ug.open)
		return fail(SDT_ESTATE, "%s: no unitig list: call sdt_gpu_unitigs_begin first", what);
	if (c->ug.stale || c->ug.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_unitigs_begin", what);
	return SDT_OK;
}

static int index_open(const sdt_ctx *c, const char *what)
{
	const int rc = list_open(c, what);
	if (rc != SDT_OK) return rc;
	if (!c->ug.lab)
		return fail(SDT_ESTATE, "%s: no sdt_gpu_unitigs_index of this unitig list", what);
	return SDT_OK;
}

static void index_free(sdt_ctx *c)
{
	if (c->ug.lab) (void)hipFree(c->ug.lab);
	c->ug.lab = nullptr;
}

static ClusterRule rule_of(const sdt_ctx *c) { return ClusterRule{c->ug.min_count, c->ug.max_count, c->ug.min_link}; }

// One dense device-resident batch, checked arguments: the records and the segment offsets (d_rec[nreads], d_seg_offs[nreads + 1]), and
// *total = the segments.  Waits.  d_counts: nreads + 1 words of scratch.
static int reads_count(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, ReadPath *d_rec, uint64_t *d_seg_offs, DevBuf &d_counts,
                       uint64_t *total)
{
	int rc = d_counts.reserve((nreads + 1) * sizeof(uint64_t), "sdt_gpu_unitigs_reads: segment counts");
	if (rc != SDT_OK) return rc;
	uint64_t *counts = (uint64_t *)d_counts.p;
	size_t tb = 0;
	HIPCHK(rocprim::exclusive_scan(nullptr, tb, counts, d_seg_offs, (uint64_t)0, (size_t)(nreads + 1), rocprim::plus<uint64_t>(), c->stream));
	DevBuf d_tmp;
	rc = d_tmp.get(tb, "sdt_gpu_unitigs_reads: scan");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(counts + nreads, 0, sizeof(uint64_t), c->stream));
	const int g = wave_grid(c, nreads);
	const uint32_t min_link = c->ug.min_link;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_th_reads<NW, false>), dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, nreads, c->K, min_link, table_of<NW>(c),
		                   (const uint2 *)c->ug.lab, d_rec, counts, (const uint64_t *)nullptr, (PathSeg *)nullptr);
	});
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && ev) {
		e = hipEventRecord(ev->b, c->stream);
		ev->kmers = nreads;                                  // (reads, not k-mers: their lengths are on the device only)
	}
	if (e == hipSuccess) e = rocprim::exclusive_scan(d_tmp.p, tb, counts, d_seg_offs, (uint64_t)0, (size_t)(nreads + 1), rocprim::plus<uint64_t>(), c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(total, d_seg_offs + nreads, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (the scan's scratch goes when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	return SDT_OK;
}

// the segment records of the same batch at d_segs[d_seg_offs[r] ..]; enqueued only
static int reads_write(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, const uint64_t *d_seg_offs, PathSeg *d_segs)
{
	const int g = wave_grid(c, nreads);
	const uint32_t min_link = c->ug.min_link;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(k_th_reads<NW, true>), dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, nreads, c->K, min_link, table_of<NW>(c),
		                   (const uint2 *)c->ug.lab, (ReadPath *)nullptr, (uint64_t *)nullptr, d_seg_offs, d_segs);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;
	}
	return SDT_OK;
}

extern "C" {

int sdt_gpu_unitigs_index(sdt_ctx *c, uint64_t info[4])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	int rc = list_open(c, "sdt_gpu_unitigs_index");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_index");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));                 // (a unitigs_reads_device on the index that goes may still be running)
	index_free(c);                                           // (a second index rebuilds)
	const uint64_t slots = c->slots, bytes = slots * sizeof(uint2), n = c->ug.n;
	DevBuf d_ctr;
	rc = d_ctr.get(TH_COUNTERS * sizeof(unsigned long long), "sdt_gpu_unitigs_index: counters");
	if (rc != SDT_OK) return rc;
	const hipError_t em = hipMalloc(&c->ug.lab, bytes);
	if (em != hipSuccess) {
		c->ug.lab = nullptr;
		return fail(SDT_ENOMEM, "the unitig index: %llu bytes, eight per table slot: %s", (unsigned long long)bytes, hipGetErrorString(em));
	}
	unsigned long long h[TH_COUNTERS] = {};
	hipError_t e = hipMemsetAsync(c->ug.lab, 0xFF, bytes, c->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_ctr.p, 0, sizeof h, c->stream);
	EventPair *ev = e == hipSuccess ? next_event(c) : nullptr;
	if (ev) e = hipEventRecord(ev->a, c->stream);
	if (e == hipSuccess && n) {
		const ClusterRule rule = rule_of(c);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_th_label<NW>, dim3(scan_grid(c, n)), dim3(TPB), 0, c->stream, table_of<NW>(c), c->K, rule, (const uint64_t *)c->ug.keys,
			                   (const Unitig *)c->ug.rec, n, (uint2 *)c->ug.lab, (unsigned long long *)d_ctr.p);
		});
		e = hipGetLastError();
	}
	if (e == hipSuccess && ev) {
		e = hipEventRecord(ev->b, c->stream);
		ev->kmers = slots;                                   // (slots labelled or cleared, not k-mers)
	}
	if (e == hipSuccess) e = hipMemcpyAsync(h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (the counters go when this returns)
	if (e != hipSuccess || e2 != hipSuccess) index_free(c);
	HIPCHK(e);
	HIPCHK(e2);
	if (h[TH_N_TOO_LONG]) {
		index_free(c);
		return fail(SDT_ELIMIT, "sdt_gpu_unitigs_index: %llu unitigs of 2^31 nodes or more: a position and its strand share 32 bits", h[TH_N_TOO_LONG]);
	}
	const unsigned long long n_live = c->ug.live;            // the labelled nodes are the live nodes of begin
	if (h[TH_N_BROKEN] || h[TH_N_NODES] != n_live) {
		index_free(c);
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_index: %llu unitigs do not walk as they did at sdt_gpu_unitigs_begin (%llu nodes labelled of %llu)", h[TH_N_BROKEN],
		            h[TH_N_NODES], n_live);
	}
	if (info) {
		const uint64_t out[4] = {h[TH_N_NODES], n, bytes, 0};
		memcpy(info, out, sizeof out);
	}
	return SDT_OK;
}

int sdt_gpu_unitigs_lookup(sdt_ctx *c, const uint64_t *keys, uint64_t n, sdt_unitig_pos *out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!keys || !out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = index_open(c, "sdt_gpu_unitigs_lookup");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_lookup");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const uint64_t piece = chunk_items(PROFILE_CHUNK_READS), most = n < piece ? n : piece;
	DevBuf d_k, d_o;
	rc = d_k.get(most * c->nw * sizeof(uint64_t), "unitig lookup staging");
	if (rc == SDT_OK) rc = d_o.get(most * sizeof(UnitigPos), "unitig lookup staging");
	if (rc != SDT_OK) return rc;
	for (uint64_t i0 = 0; i0 < n; i0 += piece) {
		const uint64_t k = n - i0 < piece ? n - i0 : piece;
		HIPCHK(hipMemcpyAsync(d_k.p, keys + i0 * c->nw, k * c->nw * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		const int g = scan_grid(c, k);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_th_lookup<NW>, dim3(g), dim3(TPB), 0, c->stream, (const uint64_t *)d_k.p, k, c->K, table_of<NW>(c), (const uint2 *)c->ug.lab,
			                   (UnitigPos *)d_o.p);
		});
		const hipError_t e = hipGetLastError();
		const hipError_t e2 = e == hipSuccess ? hipMemcpyAsync(out + i0, d_o.p, k * sizeof(UnitigPos), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
		const hipError_t e3 = hipStreamSynchronize(c->stream);   // (the next piece is staged in the same buffers)
		HIPCHK(e);
		HIPCHK(e2);
		HIPCHK(e3);
	}
	return SDT_OK;
}

int sdt_gpu_unitigs_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, void *d_rec, void *d_seg_offsets, void *d_segs,
                                 uint64_t capacity, uint64_t *n_segs)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_rec || !d_seg_offsets || !n_segs || (!d_segs && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = index_open(c, "sdt_gpu_unitigs_reads");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_reads");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf d_counts;
	uint64_t total = 0;
	rc = reads_count(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (ReadPath *)d_rec, (uint64_t *)d_seg_offsets, d_counts, &total);
	if (rc != SDT_OK) return rc;
	*n_segs = total;
	if (!d_segs && capacity == 0)
		return SDT_OK;                                       // (the records and the offsets only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_reads: %llu segments, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	if (total == 0)
		return SDT_OK;
	rc = reads_write(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (const uint64_t *)d_seg_offsets, (PathSeg *)d_segs);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

int sdt_gpu_unitigs_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, sdt_read_path *rec,
                          uint64_t *seg_offsets, sdt_path_seg *segs, uint64_t capacity, uint64_t *n_segs)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !rec || !seg_offsets || !n_segs || (!segs && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = index_open(c, "sdt_gpu_unitigs_reads");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_reads");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	if (in.longest >> 32)
		return fail(SDT_EINVAL, "a read of %llu bases: the fields of sdt_read_path and sdt_path_seg are 32-bit", (unsigned long long)in.longest);
	SDT_ENTER(c);
	// piece by piece: the records, the offsets moved on by the segments of the pieces before, and the segments while they fit
	DevBuf d_rec, d_so, d_counts, d_segs;
	uint64_t total = 0;
	const bool want = segs != nullptr;
	rc = for_each_piece(c, packed_words, offsets, nreads, 1, "unitig thread staging", [&](const StagedPiece &p) -> int {
		int rc = d_rec.reserve(p.nr * sizeof(ReadPath), "unitig thread staging");
		if (rc == SDT_OK) rc = d_so.reserve((p.nr + 1) * sizeof(uint64_t), "unitig thread staging");
		uint64_t here = 0;
		if (rc == SDT_OK) rc = reads_count(c, p.d_words, p.d_offs, p.nr, (ReadPath *)d_rec.p, (uint64_t *)d_so.p, d_counts, &here);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(rec + p.r0, d_rec.p, p.nr * sizeof(ReadPath), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(seg_offsets + p.r0, d_so.p, (p.nr + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i <= p.nr; i++) seg_offsets[p.r0 + i] += total;
		if (want && here && total + here <= capacity) {
			rc = d_segs.reserve(here * sizeof(PathSeg), "unitig thread staging");
			if (rc == SDT_OK) rc = reads_write(c, p.d_words, p.d_offs, p.nr, (const uint64_t *)d_so.p, (PathSeg *)d_segs.p);
			if (rc != SDT_OK) return rc;
			HIPCHK(hipMemcpyAsync(segs + total, d_segs.p, here * sizeof(PathSeg), hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));         // (the next piece is staged in the same buffers)
		}
		total += here;
		return SDT_OK;
	});
	if (rc != SDT_OK) return rc;
	*n_segs = total;
	if (want && total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_reads: %llu segments, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	return SDT_OK;
}

} // extern "C"
