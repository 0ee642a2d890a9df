// sdt_trim.hip -- reads cut back to their longest solid stretch against the counted node table (the rule: include/sdt_gpu.h) =
// k_trim_reads, and the compaction of a 2-bit stream to the kept range of every read = k_trim_place + k_compact_words.  Nothing here
// writes the table or the kept reads.  State rules and the high halves of the counts are sdt_search.hip's; launch geometry,
// staging in pieces and the walk over the kept batches are sdt_readstage.hpp's.
#include "sdt_compact.hpp"
#include "sdt_trim_kernels.cuh"

static_assert(sizeof(sdt_read_trim) == sizeof(ReadTrim) && sizeof(sdt_trim_params) == sizeof(TrimParams), "include/sdt_gpu.h and the kernels agree");

// one dense device-resident batch, checked arguments: the kernel and the wait for its two counters (d_cov_flags[2]: the reads kept)
static int trim_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                       const sdt_trim_params *p, ReadTrim *d_trim, uint8_t *d_keep, uint64_t *n_kept)
{
	int rc = flags_begin(c);
	if (rc != SDT_OK) return rc;
	const TrimParams prm = {p->min_count, p->min_cov, p->min_len, p->flags};
	rc = launch_strip(c, nreads, max_read_len, [&](auto nw, const StripGeometry &geo, const HiView &hv) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_trim_reads<NW>, dim3(geo.blocks), dim3(TPB), geo.lds_bytes, c->stream, d_words, d_offs, nreads, c->K, table_of<NW>(c),
		                   hv, prm, (int)geo.mk, geo.waves, d_trim, d_keep, c->d_cov_flags, c->d_cov_flags + 2);
	});
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	rc = flags_end(c, "sdt_gpu_trim_reads", max_read_len, fl);
	if (n_kept) *n_kept += fl[2];
	return rc;
}

static int params_ok(const sdt_trim_params *p)
{
	if (!p)
		return fail(SDT_EINVAL, "NULL argument");
	if (p->flags & ~(uint32_t)SDT_TRIM_CORRECTED)
		return fail(SDT_EINVAL, "trim flags 0x%x: only SDT_TRIM_CORRECTED (0x%x) is known", p->flags, (unsigned)SDT_TRIM_CORRECTED);
	return SDT_OK;
}

// the compaction of one device-resident stream to the kept range of every read, checked arguments
static int compact_trimmed_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, const ReadTrim *d_trim,
                                  uint32_t *d_out_words, uint64_t out_words_cap, uint64_t *d_out_offs, uint64_t *n_out_reads,
                                  uint64_t *n_out_words)
{
	const auto place = [&](int grid, const uint64_t *new_off, const uint64_t *rank, uint64_t *src) {
		hipLaunchKernelGGL(k_trim_place, dim3(grid), dim3(TPB), 0, c->stream, d_trim, d_offs, nreads, new_off, rank, d_out_offs, src);
	};
	return compact_stream(c, "sdt_gpu_compact_trimmed", d_words, nreads, TrimmedLen{d_trim, d_offs, nreads}, TrimmedFlag{d_trim, d_offs, nreads},
	                      place, d_out_words, out_words_cap, d_out_offs, n_out_reads, n_out_words);
}

extern "C" {

int sdt_gpu_trim_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, uint64_t max_read_len,
                              const sdt_trim_params *params, void *d_trim, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_trim)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = params_ok(params);
	if (rc != SDT_OK) return rc;
	rc = search_ready(c, "sdt_gpu_trim_reads");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return trim_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, max_read_len, params, (ReadTrim *)d_trim,
	                   (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_trim_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                       const sdt_trim_params *params, sdt_read_trim *trim, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !trim)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = params_ok(params);
	if (rc != SDT_OK) return rc;
	rc = search_ready(c, "sdt_gpu_trim_reads");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	StripGeometry geo;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc == SDT_OK) rc = strip_plan(c, nreads, in.longest, &geo);      // (the whole call is refused before a piece's records are written)
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return staged_records<ReadTrim>(c, packed_words, offsets, nreads, 1, "trim staging", trim, keep, n_kept,
	                                [&](const StagedPiece &p, ReadTrim *d_r, uint8_t *d_k, uint64_t *kept) {
		return trim_device(c, p.d_words, p.d_offs, p.nr, p.maxlen, params, d_r, d_k, kept);
	});
}

int sdt_gpu_trim_kept_reads(sdt_ctx *c, const sdt_trim_params *params, sdt_read_trim *trim, uint64_t out_capacity, uint64_t *nreads,
                            uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = params_ok(params);
	if (rc != SDT_OK) return rc;
	rc = search_ready(c, "sdt_gpu_trim_kept_reads");
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "trim", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!trim)
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	uint64_t kept = 0;
	rc = for_each_kept_batch<ReadTrim>(c, trim, most, "trim records", [&](const sdt_ctx::KeptBatch &kb, ReadTrim *d_r) {
		return trim_device(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, params, d_r, nullptr, &kept);
	});
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

int sdt_gpu_compact_trimmed_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const void *d_trim,
                                   void *d_out_words, uint64_t out_words_cap, void *d_out_offsets, uint64_t *n_out_reads,
                                   uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!d_out_words || !d_out_offsets || (nreads && (!d_packed_words || !d_offsets || !d_trim)))
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	return compact_trimmed_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (const ReadTrim *)d_trim,
	                              (uint32_t *)d_out_words, out_words_cap, (uint64_t *)d_out_offsets, n_out_reads, n_out_words);
}

int sdt_gpu_compact_trimmed(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                            const sdt_read_trim *trim, uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets,
                            uint64_t *n_out_reads, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!out_words || !out_offsets || (nreads && (!packed_words || !offsets || !trim)))
		return fail(SDT_EINVAL, "NULL argument");
	// every range lies in its read
	const auto tally = [&](uint64_t i, uint64_t &bases, uint64_t &kept) -> int {
		if ((uint64_t)trim[i].start + trim[i].len > offsets[i + 1] - offsets[i])
			return fail(SDT_EINVAL, "read %llu has %llu bases, its record keeps [%u, %u + %u)", (unsigned long long)i,
			            (unsigned long long)(offsets[i + 1] - offsets[i]), trim[i].start, trim[i].start, trim[i].len);
		if (trim[i].len) { bases += trim[i].len; kept++; }
		return SDT_OK;
	};
	const auto device = [&](const uint32_t *d_w, const uint64_t *d_o, const void *d_trim, uint32_t *d_ow, uint64_t cap, uint64_t *d_oo, uint64_t *reads,
	                        uint64_t *words) { return compact_trimmed_device(c, d_w, d_o, nreads, (const ReadTrim *)d_trim, d_ow, cap, d_oo, reads, words); };
	return compact_host(c, "sdt_gpu_compact_trimmed", packed_words, nwords, offsets, nreads, tally, trim, nreads * sizeof(ReadTrim), device, out_words,
	                    out_words_cap, out_offsets, n_out_reads, n_out_words);
}

} // extern "C"
