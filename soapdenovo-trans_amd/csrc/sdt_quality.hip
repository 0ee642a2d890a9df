// sdt_quality.hip -- reads trimmed to their best segment by Mott's rule and filtered by low bases and expected errors, from their base
// qualities alone, before anything else of the chain runs (the rule: include/sdt_gpu.h) = k_quality_reads (sdt_quality_kernels.cuh).
// Needs no counted table and not the bases: both forms need the context for its stream only.  There is no kept form: the reads kept
// in HBM carry no qualities.  What is refused, the table of expected errors and the cut of a byte stream into pieces are
// sdt_read_plan.h's; staging the pieces is sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len
// and verdict sit where sdt_read_trim has them.
#include "sdt_compact.hpp"
#include "sdt_quality_kernels.cuh"

static_assert(sizeof(sdt_read_quality) == sizeof(ReadQuality) && sizeof(sdt_quality_params) == sizeof(QualityParams),
              "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_quality>(), "sdt_gpu_compact_trimmed takes sdt_read_quality records through a pointer cast");

static QualityParams kernel_params(const sdt_quality_params *p)
{
	return QualityParams{p->phred_offset, p->cut_q, p->low_q, p->max_low_pct, p->max_ee_ppm, p->min_len, p->flags, p->reserved};
}

// every refusal of the parameters, before any launch
static int args_ok(const sdt_quality_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_quality_params is NULL");
	switch (check_quality_params(kernel_params(p))) {
	case QUALITY_PHRED_OFFSET: return fail(SDT_EINVAL, "sdt_quality_params.phred_offset = %u: 33, 64 or 0 (the bytes are the qualities)", p->phred_offset);
	case QUALITY_CUT_Q: return fail(SDT_EINVAL, "sdt_quality_params.cut_q = %u: a quality, 93 at most (0: no trimming)", p->cut_q);
	case QUALITY_LOW_Q: return fail(SDT_EINVAL, "sdt_quality_params.low_q = %u: a quality, 93 at most (0: no base is low)", p->low_q);
	case QUALITY_MAX_LOW_PCT: return fail(SDT_EINVAL, "sdt_quality_params.max_low_pct = %u: a percentage, 100 at most", p->max_low_pct);
	case QUALITY_FLAGS: return fail(SDT_EINVAL, "sdt_quality_params.flags = 0x%x: no flag is defined", p->flags);
	case QUALITY_RESERVED: return fail(SDT_EINVAL, "sdt_quality_params.reserved = %u: it must be 0", p->reserved);
	default: return SDT_OK;
	}
}

// one device-resident batch, checked arguments: the kernel and the wait for its counter (ctr: one 64-bit word on the device)
static int quality_device(sdt_ctx *c, const DevBuf &ctr, const uint8_t *d_quals, const uint64_t *d_offs, uint64_t nreads, const sdt_quality_params *p,
                          ReadQuality *d_out, uint8_t *d_keep, uint64_t *n_kept)
{
	return launch_counted(c, ctr, nreads, nreads, n_kept, [&](int grid, unsigned long long *d_ctr) {
		hipLaunchKernelGGL(k_quality_reads, dim3(grid), dim3(TPB), 0, c->stream, d_quals, d_offs, nreads, kernel_params(p), d_out, d_keep, d_ctr);
	});
}

extern "C" {

int sdt_gpu_quality_reads_device(sdt_ctx *c, const void *d_quals, const void *d_offsets, uint64_t nreads, const sdt_quality_params *params, void *d_out,
                                 void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_quals || !d_offsets || !d_out)
		return fail(SDT_EINVAL, "NULL argument");
	if ((uintptr_t)d_quals & 3)
		return fail(SDT_EINVAL, "d_quals = %p: it must be 4-byte aligned", d_quals);
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "quality counter");
	if (rc != SDT_OK) return rc;
	return quality_device(c, ctr, (const uint8_t *)d_quals, (const uint64_t *)d_offsets, nreads, params, (ReadQuality *)d_out, (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_quality_reads(sdt_ctx *c, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets, uint64_t nreads, const sdt_quality_params *params,
                          sdt_read_quality *out, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!quals || !offsets || !out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = byte_stream_args_ok(offsets, nreads, nbytes, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr, d_r, d_k;
	rc = ctr.get(sizeof(unsigned long long), "quality counter");
	if (rc != SDT_OK) return rc;
	uint64_t kept = 0;
	rc = for_each_byte_piece(c, quals, offsets, nreads, "quality staging", [&](const StagedBytePiece &p) -> int {
		int rc = d_r.reserve(p.nr * sizeof(ReadQuality), "quality staging");
		if (rc == SDT_OK) rc = d_k.reserve(p.nr, "quality staging");
		if (rc == SDT_OK) rc = quality_device(c, ctr, p.d_bytes, p.d_offs, p.nr, params, (ReadQuality *)d_r.p, (uint8_t *)d_k.p, &kept);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(out + p.r0, d_r.p, p.nr * sizeof(ReadQuality), hipMemcpyDeviceToHost));
		if (keep) HIPCHK(hipMemcpy(keep + p.r0, d_k.p, p.nr, hipMemcpyDeviceToHost));
		return SDT_OK;
	});
	if (rc == SDT_OK && n_kept) *n_kept = kept;
	return rc;
}

} // extern "C"
