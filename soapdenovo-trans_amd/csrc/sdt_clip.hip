// sdt_clip.hip -- sequencing adapters and poly-A/T tails clipped from reads before pass 1 (the rule: include/sdt_gpu.h) = k_clip_reads
// (sdt_clip_kernels.cuh).  Needs no counted table: the dense forms need the context for its stream only, the kept form for the reads
// kept in HBM.  Nothing here writes the table or the kept reads.  What is refused, and the adapters as the kernel takes them, are
// sdt_read_plan.h's; staging in pieces and the kept batches are sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as
// they are: start, len and verdict sit where sdt_read_trim has them.
#include "sdt_compact.hpp"
#include "sdt_clip_kernels.cuh"

static_assert(sizeof(sdt_read_clip) == sizeof(ReadClip) && sizeof(sdt_clip_params) == sizeof(ClipParams), "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_clip>(), "sdt_gpu_compact_trimmed takes sdt_read_clip records through a pointer cast");
static_assert(SDT_CLIP_MAX_ADAPTERS == CLIP_MAX_ADAPTERS && SDT_CLIP_MAX_ADAPTER_LEN == CLIP_MAX_ADAPTER_LEN, "include/sdt_gpu.h and sdt_read_plan.h agree");

// every refusal of the parameters and of the adapter set, before any launch
static int args_ok(const sdt_clip_params *p, const sdt_adapter_set *as)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_clip_params is NULL");
	const ClipParams q = {p->min_overlap, p->max_err_pct, p->min_len, p->min_tail, p->tail_err_pct, p->tail3_bases, p->tail5_bases, p->flags};
	switch (check_clip_params(q)) {
	case CLIP_FLAGS: return fail(SDT_EINVAL, "sdt_clip_params.flags = 0x%x: no flag is known", p->flags);
	case CLIP_MIN_OVERLAP: return fail(SDT_EINVAL, "sdt_clip_params.min_overlap = 0: an overlap of no bases always hits");
	case CLIP_MAX_ERR_PCT: return fail(SDT_EINVAL, "sdt_clip_params.max_err_pct = %u: a percentage, 100 at most", p->max_err_pct);
	case CLIP_TAIL_ERR_PCT: return fail(SDT_EINVAL, "sdt_clip_params.tail_err_pct = %u: a percentage, 100 at most", p->tail_err_pct);
	case CLIP_TAIL3_BASES: return fail(SDT_EINVAL, "sdt_clip_params.tail3_bases = 0x%x: a mask of the four bases, 15 at most", p->tail3_bases);
	case CLIP_TAIL5_BASES: return fail(SDT_EINVAL, "sdt_clip_params.tail5_bases = 0x%x: a mask of the four bases, 15 at most", p->tail5_bases);
	case CLIP_MIN_TAIL: return fail(SDT_EINVAL, "sdt_clip_params.min_tail = 0 with a tail mask set: every read would lose a tail");
	default: break;
	}
	if (!as || as->n == 0)
		return SDT_OK;
	if (as->n > SDT_CLIP_MAX_ADAPTERS)
		return fail(SDT_EINVAL, "sdt_adapter_set.n = %u: %d adapters at most", as->n, SDT_CLIP_MAX_ADAPTERS);
	if (!as->words || !as->offsets || !as->ends)
		return fail(SDT_EINVAL, "sdt_adapter_set: NULL words, offsets or ends with n = %u", as->n);
	uint64_t i;
	const ClipFault f = check_adapter_set(as->offsets, as->ends, as->n, p->min_overlap, &i);
	const unsigned long long a = i, m = f == CLIP_OK || f == CLIP_OFFSETS ? 0 : as->offsets[i + 1] - as->offsets[i];
	switch (f) {
	case CLIP_OFFSETS: return fail(SDT_EINVAL, "sdt_adapter_set.offsets not monotonic at adapter %llu", a);
	case CLIP_ADAPTER_EMPTY: return fail(SDT_EINVAL, "adapter %llu has 0 bases", a);
	case CLIP_ADAPTER_LONG: return fail(SDT_EINVAL, "adapter %llu has %llu bases: %d at most", a, m, SDT_CLIP_MAX_ADAPTER_LEN);
	case CLIP_ADAPTER_SHORT: return fail(SDT_EINVAL, "adapter %llu has %llu bases, fewer than min_overlap = %u: it could never hit", a, m, p->min_overlap);
	case CLIP_ADAPTER_END: return fail(SDT_EINVAL, "sdt_adapter_set.ends[%llu] = %u: 0 (3') or 1 (5')", a, (unsigned)as->ends[i]);
	default: return SDT_OK;
	}
}

// what a call holds on the device beside the reads: the adapters, 3' first, and the counter of the reads kept
struct ClipState {
	DevBuf ads, ctr;
	ClipSet set = {nullptr, 0, 0};
	ClipParams prm;
	int prepare(const sdt_clip_params *p, const sdt_adapter_set *as)
	{
		prm = ClipParams{p->min_overlap, p->max_err_pct, p->min_len, p->min_tail, p->tail_err_pct, p->tail3_bases, p->tail5_bases, p->flags};
		std::vector<ClipAdapter> host;
		const uint32_t n = as ? as->n : 0;
		for (uint32_t end = 0; end < 2; end++)
			for (uint32_t i = 0; i < n; i++)
				if (as->ends[i] == end) host.push_back(split_adapter(as->words, as->offsets, as->ends, i));
		for (uint32_t i = 0; i < n; i++) (as->ends[i] ? set.n5 : set.n3)++;
		int rc = ads.get(host.size() * sizeof(ClipAdapter), "adapters");
		if (rc == SDT_OK) rc = ctr.get(sizeof(unsigned long long), "clip counter");
		if (rc != SDT_OK) return rc;
		if (!host.empty()) HIPCHK(hipMemcpy(ads.p, host.data(), host.size() * sizeof(ClipAdapter), hipMemcpyHostToDevice));
		set.ad = (const ClipAdapter *)ads.p;
		return SDT_OK;
	}
};

// one dense device-resident batch, checked arguments: the kernel and the wait for its counter
static int clip_device(sdt_ctx *c, const ClipState &st, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, ReadClip *d_clip,
                       uint8_t *d_keep, uint64_t *n_kept)
{
	return launch_counted(c, st.ctr, nreads, nreads, n_kept, [&](int grid, unsigned long long *ctr) {
		hipLaunchKernelGGL(k_clip_reads, dim3(grid), dim3(TPB), 0, c->stream, d_words, d_offs, nreads, st.prm, st.set, d_clip, d_keep, ctr);
	});
}

extern "C" {

int sdt_gpu_clip_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const sdt_clip_params *params,
                              const sdt_adapter_set *adapters, void *d_clip, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_clip)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, adapters);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	ClipState st;
	rc = st.prepare(params, adapters);
	if (rc != SDT_OK) return rc;
	return clip_device(c, st, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (ReadClip *)d_clip, (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_clip_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                       const sdt_clip_params *params, const sdt_adapter_set *adapters, sdt_read_clip *clip, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !clip)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, adapters);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	ClipState st;
	rc = st.prepare(params, adapters);
	if (rc != SDT_OK) return rc;
	return staged_records<ReadClip>(c, packed_words, offsets, nreads, 1, "clip staging", clip, keep, n_kept,
	                                [&](const StagedPiece &p, ReadClip *d_r, uint8_t *d_k, uint64_t *kept) {
		return clip_device(c, st, p.d_words, p.d_offs, p.nr, d_r, d_k, kept);
	});
}

int sdt_gpu_clip_kept_reads(sdt_ctx *c, const sdt_clip_params *params, const sdt_adapter_set *adapters, sdt_read_clip *clip,
                            uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = args_ok(params, adapters);
	if (rc != SDT_OK) return rc;
	rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_clip_kept_reads", false);
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "clip", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!clip)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	ClipState st;
	rc = st.prepare(params, adapters);
	if (rc != SDT_OK) return rc;
	uint64_t kept = 0;
	rc = for_each_kept_batch<ReadClip>(c, clip, most, "clip records", [&](const sdt_ctx::KeptBatch &kb, ReadClip *d_r) {
		return clip_device(c, st, kb.d_words, kb.d_offs, kb.nreads, d_r, nullptr, &kept);
	});
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
