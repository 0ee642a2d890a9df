// sdt_qc.hip -- the per-cycle QC report of a read batch: base composition, qualities, lengths, GC and mean quality by histograms that
// the call ADDS to (the rule: include/sdt_gpu.h) = k_qc_reads (sdt_qc_kernels.cuh).  Needs no counted table: both forms need the
// context for its stream only.  There is no kept form: the reads kept in HBM carry no qualities.  What is refused, the layout of the
// report and the grid are sdt_read_plan.h's; staging the pieces is sdt_readstage.hpp's.  The ranges are the 24-byte records of any
// stage: only start and len, where sdt_read_trim has them, are read.
#include "sdt_readstage.hpp"
#include "sdt_qc_kernels.cuh"
#include <cstddef>

static_assert(sizeof(sdt_qc_params) == sizeof(QcParams), "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_read_trim) == sizeof(ReadTrim) && offsetof(sdt_read_trim, start) == offsetof(ReadTrim, start) &&
                  offsetof(sdt_read_trim, len) == offsetof(ReadTrim, len),
              "the ranges are read where sdt_read_trim has start and len");
static_assert(SDT_QC_MAX_CYCLES == QC_MAX_CYCLES && SDT_QC_FROM_END == QC_FROM_END, "include/sdt_gpu.h and sdt_read_plan.h agree");

static QcParams kernel_params(const sdt_qc_params *p) { return QcParams{p->cycles, p->phred_offset, p->flags, p->class_sel, p->reserved}; }

// every refusal of the parameters, before any launch
static int args_ok(const sdt_qc_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_qc_params is NULL");
	switch (check_qc_params(kernel_params(p))) {
	case QC_CYCLES: return fail(SDT_EINVAL, "sdt_qc_params.cycles = %u: 1 to %u", p->cycles, QC_MAX_CYCLES);
	case QC_PHRED_OFFSET: return fail(SDT_EINVAL, "sdt_qc_params.phred_offset = %u: 33, 64 or 0 (the bytes are the qualities)", p->phred_offset);
	case QC_FLAGS: return fail(SDT_EINVAL, "sdt_qc_params.flags = 0x%x: only SDT_QC_FROM_END (0x%x) is defined", p->flags, QC_FROM_END);
	case QC_CLASS_SEL: return fail(SDT_EINVAL, "sdt_qc_params.class_sel = %u: a class byte, 255 at most", p->class_sel);
	case QC_RESERVED: return fail(SDT_EINVAL, "sdt_qc_params.reserved = %u: it must be 0", p->reserved);
	default: return SDT_OK;
	}
}

// one device-resident batch, checked arguments: the kernel, which adds to d_report, and the wait for it
static int qc_device(sdt_ctx *c, const uint32_t *d_words, const uint8_t *d_quals, long long delta, const uint64_t *d_offs, uint64_t nreads,
                     const ReadTrim *d_ranges, const uint8_t *d_classes, const sdt_qc_params *p, unsigned long long *d_report)
{
	const QcArgs A = {d_words, d_quals, d_offs, nreads, d_ranges, d_classes, delta, kernel_params(p), d_report};
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	hipLaunchKernelGGL(k_qc_reads, dim3(qc_blocks(nreads, c->cu_count, wave_blocks_forced())), dim3(QC_TPB), 0, c->stream, A);
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;                                  // (reads, not k-mers: sdt_gpu_kernel_time reports them as they are)
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

extern "C" {

uint64_t sdt_gpu_qc_report_words(uint32_t cycles) { return qc_report_words(cycles); }

int sdt_gpu_qc_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_quals, const void *d_offsets, uint64_t nreads, const void *d_ranges,
                            const void *d_classes, const sdt_qc_params *params, void *d_report)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_report)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	if ((uintptr_t)d_quals & 3)
		return fail(SDT_EINVAL, "d_quals = %p: it must be 4-byte aligned", d_quals);
	if ((uintptr_t)d_report & 7)
		return fail(SDT_EINVAL, "d_report = %p: it must be 8-byte aligned", d_report);
	SDT_ENTER(c);
	return qc_device(c, (const uint32_t *)d_packed_words, (const uint8_t *)d_quals, 0, (const uint64_t *)d_offsets, nreads, (const ReadTrim *)d_ranges,
	                 (const uint8_t *)d_classes, params, (unsigned long long *)d_report);
}

int sdt_gpu_qc_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets,
                     uint64_t nreads, const sdt_read_trim *ranges, const uint8_t *classes, const sdt_qc_params *params, uint64_t *report,
                     uint64_t report_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !report)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params);
	if (rc != SDT_OK) return rc;
	const uint64_t words = qc_report_words(params->cycles);
	if (report_words < words)
		return fail(SDT_EINVAL, "report_words = %llu: cycles = %u takes %llu words", (unsigned long long)report_words, params->cycles,
		            (unsigned long long)words);
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	if (quals) {
		rc = byte_stream_args_ok(offsets, nreads, nbytes, &in);
		if (rc != SDT_OK) return rc;
	}
	if (ranges)
		for (uint64_t r = 0; r < nreads; r++)
			if ((uint64_t)ranges[r].start + ranges[r].len > offsets[r + 1] - offsets[r])
				return fail(SDT_EINVAL, "ranges[%llu]: start = %u, len = %u, the read has %llu bases", (unsigned long long)r, ranges[r].start,
				            ranges[r].len, (unsigned long long)(offsets[r + 1] - offsets[r]));
	SDT_ENTER(c);
	DevBuf d_rep, d_q, d_rg, d_cl;
	rc = d_rep.get(words * sizeof(uint64_t), "qc report");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_rep.p, 0, words * sizeof(uint64_t), c->stream));
	rc = for_each_piece(c, packed_words, offsets, nreads, 1, "qc staging", [&](const StagedPiece &p) -> int {
		// the piece's words start at base 16 w0 of the stream, its bytes at b0: the byte of a base lies at its index + 16 w0 - b0
		const uint64_t w0 = offsets[p.r0] >> 4, b0 = offsets[p.r0] & ~3ULL, qbytes = offsets[p.r0 + p.nr] - b0;
		int rc = SDT_OK;
		if (quals) rc = d_q.reserve((qbytes + 3) & ~(size_t)3, "qc staging");
		if (rc == SDT_OK && ranges) rc = d_rg.reserve(p.nr * sizeof(ReadTrim), "qc staging");
		if (rc == SDT_OK && classes) rc = d_cl.reserve(p.nr, "qc staging");
		if (rc != SDT_OK) return rc;
		if (quals && qbytes) HIPCHK(hipMemcpyAsync(d_q.p, quals + b0, qbytes, hipMemcpyHostToDevice, c->stream));
		if (ranges) HIPCHK(hipMemcpyAsync(d_rg.p, ranges + p.r0, p.nr * sizeof(ReadTrim), hipMemcpyHostToDevice, c->stream));
		if (classes) HIPCHK(hipMemcpyAsync(d_cl.p, classes + p.r0, p.nr, hipMemcpyHostToDevice, c->stream));
		return qc_device(c, p.d_words, quals ? (const uint8_t *)d_q.p : nullptr, (long long)((w0 << 4) - b0), p.d_offs, p.nr,
		                 ranges ? (const ReadTrim *)d_rg.p : nullptr, classes ? (const uint8_t *)d_cl.p : nullptr, params, (unsigned long long *)d_rep.p);
	});
	if (rc != SDT_OK) return rc;
	std::vector<uint64_t> got(words);
	HIPCHK(hipMemcpy(got.data(), d_rep.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < words; i++) report[i] += got[i];
	return SDT_OK;
}

} // extern "C"
