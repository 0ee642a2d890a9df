// sdt_complexity.hip -- low-complexity reads (homopolymers, short tandem repeats, runs of N that the stream shows as poly-G) flagged,
// dropped or trimmed before pass 1 (the rule: include/sdt_gpu.h) = k_complexity_reads (sdt_complexity_kernels.cuh).  Needs no counted
// table: the dense forms need the context for its stream only, the kept form for the reads kept in HBM.  Nothing here writes the table
// or the kept reads.  What is refused and the windows are sdt_read_plan.h's; staging in pieces and the kept batches are
// sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len and verdict sit where sdt_read_trim has them.
#include "sdt_compact.hpp"
#include "sdt_complexity_kernels.cuh"

static_assert(sizeof(sdt_read_complexity) == sizeof(ReadComplexity) && sizeof(sdt_complexity_params) == sizeof(ComplexityParams),
              "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_complexity>(), "sdt_gpu_compact_trimmed takes sdt_read_complexity records through a pointer cast");
static_assert(SDT_COMPLEXITY_TRIM == COMPLEXITY_TRIM, "include/sdt_gpu.h and sdt_read_plan.h agree");

// every refusal of the parameters, before any launch
static int args_ok(const sdt_complexity_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_complexity_params is NULL");
	switch (check_complexity_params(ComplexityParams{p->max_score_pct, p->max_low_pct, p->min_len, p->flags})) {
	case COMPLEXITY_FLAGS: return fail(SDT_EINVAL, "sdt_complexity_params.flags = 0x%x: SDT_COMPLEXITY_TRIM is the only flag", p->flags);
	case COMPLEXITY_MAX_SCORE_PCT:
		return fail(SDT_EINVAL, "sdt_complexity_params.max_score_pct = %u: a percentage from 1 to 100 (at 0 every window would be low)", p->max_score_pct);
	case COMPLEXITY_MAX_LOW_PCT: return fail(SDT_EINVAL, "sdt_complexity_params.max_low_pct = %u: a percentage, 100 at most", p->max_low_pct);
	case COMPLEXITY_TRIM_MAX_LOW_PCT:
		return fail(SDT_EINVAL, "sdt_complexity_params.max_low_pct = %u under SDT_COMPLEXITY_TRIM: it must be 0, the clean stretch is what is kept",
		            p->max_low_pct);
	default: return SDT_OK;
	}
}

// one dense device-resident batch, checked arguments: the kernel and the wait for its counter (ctr: one 64-bit word on the device)
static int complexity_device(sdt_ctx *c, const DevBuf &ctr, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads,
                             const sdt_complexity_params *p, ReadComplexity *d_cx, uint8_t *d_keep, uint64_t *n_kept)
{
	const ComplexityParams prm = {p->max_score_pct, p->max_low_pct, p->min_len, p->flags};
	const DenseReads reads = {d_words, d_offs, nullptr, nreads};
	return launch_counted(c, ctr, nreads, nreads, n_kept, [&](int grid, unsigned long long *d_ctr) {
		hipLaunchKernelGGL(k_complexity_reads<DenseReads>, dim3(grid), dim3(TPB), 0, c->stream, reads, prm, d_cx, d_keep, d_ctr);
	});
}

extern "C" {

int sdt_gpu_complexity_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const sdt_complexity_params *params,
                                    void *d_cx, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_cx)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "complexity counter");
	if (rc != SDT_OK) return rc;
	return complexity_device(c, ctr, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, params, (ReadComplexity *)d_cx,
	                         (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_complexity_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                             const sdt_complexity_params *params, sdt_read_complexity *cx, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !cx)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "complexity counter");
	if (rc != SDT_OK) return rc;
	return staged_records<ReadComplexity>(c, packed_words, offsets, nreads, 1, "complexity staging", cx, keep, n_kept,
	                                      [&](const StagedPiece &p, ReadComplexity *d_r, uint8_t *d_k, uint64_t *kept) {
		return complexity_device(c, ctr, p.d_words, p.d_offs, p.nr, params, d_r, d_k, kept);
	});
}

int sdt_gpu_complexity_kept_reads(sdt_ctx *c, const sdt_complexity_params *params, sdt_read_complexity *cx, uint64_t out_capacity, uint64_t *nreads,
                                  uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_complexity_kept_reads", true);       // (as search_ready: stricter than the other table-free forms)
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "cx", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!cx)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "complexity counter");
	if (rc != SDT_OK) return rc;
	uint64_t kept = 0;
	rc = for_each_kept_batch<ReadComplexity>(c, cx, most, "complexity records", [&](const sdt_ctx::KeptBatch &kb, ReadComplexity *d_r) {
		return complexity_device(c, ctr, kb.d_words, kb.d_offs, kb.nreads, params, d_r, nullptr, &kept);
	});
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
