// sdt_overlap.hip -- the overlap of the two mates of a pair, and read-through pairs clipped at the fragment's end without an adapter
// list, before pass 1 (the rule: include/sdt_gpu.h) = k_overlap_pairs (sdt_overlap_kernels.cuh).  Needs no counted table: the dense
// forms need the context for its stream only, the kept form for the reads kept in HBM.  Nothing here writes the table or the kept
// reads.  What is refused, the check of the pair ranges and the cut of the units into stretches are sdt_read_plan.h's; staging in
// pieces and the kept batches are sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len and verdict
// sit where sdt_read_trim has them.
#include "sdt_compact.hpp"
#include "sdt_overlap_kernels.cuh"

static_assert(sizeof(sdt_read_overlap) == sizeof(ReadOverlap) && sizeof(sdt_overlap_params) == sizeof(OverlapParams), "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_overlap>(), "sdt_gpu_compact_trimmed takes sdt_read_overlap records through a pointer cast");

// every refusal of the parameters, before any launch; dense_reads: 0 for the kept form
static int args_ok(const sdt_overlap_params *p, uint64_t dense_reads)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_overlap_params is NULL");
	switch (check_overlap_params(OverlapParams{p->min_overlap, p->max_err_pct, p->min_len, p->flags}, dense_reads)) {
	case OVERLAP_FLAGS: return fail(SDT_EINVAL, "sdt_overlap_params.flags = 0x%x: no flag is known", p->flags);
	case OVERLAP_MIN_OVERLAP: return fail(SDT_EINVAL, "sdt_overlap_params.min_overlap = 0: an overlap of no bases is always admissible");
	case OVERLAP_MAX_ERR_PCT: return fail(SDT_EINVAL, "sdt_overlap_params.max_err_pct = %u: a percentage, 100 at most", p->max_err_pct);
	case OVERLAP_ODD_READS:
		return fail(SDT_EINVAL, "nreads = %llu: reads 2t and 2t + 1 are mates, an odd number of reads holds no whole pairs", (unsigned long long)dense_reads);
	default: return SDT_OK;
	}
}

// the kernel over units whose reads are in place, and the wait for its counter (ctr: one 64-bit word on the device)
template <class Reads>
static int overlap_launch(sdt_ctx *c, const Reads &reads, const Units &U, uint64_t nreads, const sdt_overlap_params *p, ReadOverlap *d_ov,
                          uint8_t *d_keep, const DevBuf &ctr, uint64_t *n_kept)
{
	const OverlapParams prm = {p->min_overlap, p->max_err_pct, p->min_len, p->flags};
	return launch_counted(c, ctr, U.n, nreads, n_kept, [&](int grid, unsigned long long *d_ctr) {
		hipLaunchKernelGGL(k_overlap_pairs<Reads>, dim3(grid), dim3(TPB), 0, c->stream, reads, U, prm, d_ov, d_keep, d_ctr);
	});
}

// one dense device-resident batch of whole pairs, checked arguments
static int overlap_device(sdt_ctx *c, const DevBuf &ctr, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, const sdt_overlap_params *p,
                          ReadOverlap *d_ov, uint8_t *d_keep, uint64_t *n_kept)
{
	const DenseReads reads = {d_words, d_offs, nullptr, nreads};
	const Units U = {nullptr, 0, UnitStretch{0, 0, 2}, nreads / 2};
	return overlap_launch(c, reads, U, nreads, p, d_ov, d_keep, ctr, n_kept);
}

extern "C" {

int sdt_gpu_overlap_pairs_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const sdt_overlap_params *params,
                                 void *d_ov, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_ov)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, nreads);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "overlap counter");
	if (rc != SDT_OK) return rc;
	return overlap_device(c, ctr, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, params, (ReadOverlap *)d_ov, (uint8_t *)d_keep,
	                      n_kept);
}

int sdt_gpu_overlap_pairs(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                          const sdt_overlap_params *params, sdt_read_overlap *ov, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !ov)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, nreads);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "overlap counter");
	if (rc != SDT_OK) return rc;
	// step 2: the mates of a pair are never split between two pieces
	return staged_records<ReadOverlap>(c, packed_words, offsets, nreads, 2, "overlap staging", ov, keep, n_kept,
	                                   [&](const StagedPiece &p, ReadOverlap *d_r, uint8_t *d_k, uint64_t *kept) {
		return overlap_device(c, ctr, p.d_words, p.d_offs, p.nr, params, d_r, d_k, kept);
	});
}

int sdt_gpu_overlap_kept_pairs(sdt_ctx *c, const sdt_overlap_params *params, const uint64_t *pair_ranges, uint64_t n_ranges, sdt_read_overlap *ov,
                               uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = args_ok(params, 0);
	if (rc == SDT_OK) rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_overlap_kept_pairs", false);
	if (rc != SDT_OK) return rc;
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "ov", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!ov)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// the entries and the records of ALL ordinals on the device at once (sdt_readstage.hpp: KeptUnits); the fingerprint in an entry is not used
	KeptUnits ku(pair_ranges, n_ranges, nord);
	DevBuf d_ent, d_ov, ctr;
	rc = d_ent.get(nord * sizeof(DedupEnt), "overlap entries");
	if (rc == SDT_OK) rc = d_ov.get(nord * sizeof(ReadOverlap), "overlap records");
	if (rc == SDT_OK) rc = ku.d_segs.get(ku.bytes(), "overlap units");
	if (rc == SDT_OK) rc = ctr.get(sizeof(unsigned long long), "overlap counter");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_ov.p, 0xFF, nord * sizeof(ReadOverlap), c->stream));
	rc = ku.upload(c);
	if (rc == SDT_OK) rc = kept_entries(c, nord, d_ent);
	uint64_t kept = 0;
	const KeptReads reads = {(const DedupEnt *)d_ent.p, nord};
	if (rc == SDT_OK) rc = overlap_launch(c, reads, ku.on_device(), total, params, (ReadOverlap *)d_ov.p, nullptr, ctr, &kept);     // (waits)
	if (rc == SDT_OK) rc = fetch_present<ReadOverlap>(ov, d_ov, nord, OVERLAP_ABSENT);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
