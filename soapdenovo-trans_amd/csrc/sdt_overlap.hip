// sdt_overlap.hip -- the overlap of the two mates of a pair, and read-through pairs clipped at the fragment's end without an adapter
// list, before pass 1 (the rule: include/sdt_gpu.h) = k_overlap_pairs (sdt_overlap_kernels.cuh).  Needs no counted table: the dense
// forms need the context for its stream only, the kept form for the reads kept in HBM.  Nothing here writes the table or the kept
// reads.  What is refused, the check of the pair ranges and the cut of the units into stretches are sdt_read_plan.h's; staging in
// pieces and the kept batches are sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len and verdict
// sit where sdt_read_trim has them.
#include "sdt_readstage.hpp"
#include "sdt_overlap_kernels.cuh"
#include <cstddef>

static_assert(sizeof(sdt_read_overlap) == sizeof(ReadOverlap) && sizeof(sdt_overlap_params) == sizeof(OverlapParams), "include/sdt_gpu.h and the kernel agree");
static_assert(offsetof(sdt_read_overlap, start) == offsetof(sdt_read_trim, start) && offsetof(sdt_read_overlap, len) == offsetof(sdt_read_trim, len) &&
                  offsetof(sdt_read_overlap, verdict) == offsetof(sdt_read_trim, verdict) && sizeof(sdt_read_overlap) == sizeof(sdt_read_trim),
              "sdt_gpu_compact_trimmed takes sdt_read_overlap records through a pointer cast");

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

// the kernel over units whose reads are in place, and the wait for its counter (ctr: one zeroed-here 64-bit word on the device)
template <class Reads>
static int overlap_launch(sdt_ctx *c, const Reads &reads, const Units &U, uint64_t nreads, const sdt_overlap_params *p, ReadOverlap *d_ov,
                          uint8_t *d_keep, unsigned long long *ctr, uint64_t *n_kept)
{
	const OverlapParams prm = {p->min_overlap, p->max_err_pct, p->min_len, p->flags};
	unsigned long long kept = 0;
	HIPCHK(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	hipLaunchKernelGGL(k_overlap_pairs<Reads>, dim3(wave_grid(c, U.n)), dim3(TPB), 0, c->stream, reads, U, prm, d_ov, d_keep, ctr);
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;                                  // (reads, not k-mers: sdt_gpu_kernel_time reports them as they are)
	}
	HIPCHK(hipMemcpyAsync(&kept, ctr, sizeof kept, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_kept) *n_kept += kept;
	return SDT_OK;
}

// one dense device-resident batch of whole pairs, checked arguments
static int overlap_device(sdt_ctx *c, const DevBuf &ctr, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, const sdt_overlap_params *p,
                          ReadOverlap *d_ov, uint8_t *d_keep, uint64_t *n_kept)
{
	const DenseReads reads = {d_words, d_offs, nullptr, nreads};
	const Units U = {nullptr, 0, UnitStretch{0, 0, 2}, nreads / 2};
	return overlap_launch(c, reads, U, nreads, p, d_ov, d_keep, (unsigned long long *)ctr.p, n_kept);
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
	DevBuf ctr, d_r, d_k;
	rc = ctr.get(sizeof(unsigned long long), "overlap counter");
	if (rc != SDT_OK) return rc;
	uint64_t kept = 0;
	// step 2: the mates of a pair are never split between two pieces
	rc = for_each_piece(c, packed_words, offsets, nreads, 2, "overlap staging", [&](const StagedPiece &p) -> int {
		int rc = d_r.reserve(p.nr * sizeof(ReadOverlap), "overlap staging");
		if (rc == SDT_OK) rc = d_k.reserve(p.nr, "overlap staging");
		if (rc == SDT_OK) rc = overlap_device(c, ctr, p.d_words, p.d_offs, p.nr, params, (ReadOverlap *)d_r.p, (uint8_t *)d_k.p, &kept);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(ov + p.r0, d_r.p, p.nr * sizeof(ReadOverlap), hipMemcpyDeviceToHost));
		if (keep) HIPCHK(hipMemcpy(keep + p.r0, d_k.p, p.nr, hipMemcpyDeviceToHost));
		return SDT_OK;
	});
	if (rc == SDT_OK && n_kept) *n_kept = kept;
	return rc;
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
	if (rc != SDT_OK) return rc;
	if (n_ranges && !pair_ranges)
		return fail(SDT_EINVAL, "NULL argument");
	PairRangeFault fault;
	const uint64_t bad = check_pair_ranges(pair_ranges, n_ranges, &fault);
	if (fault == PAIR_RANGE_NOT_PAIRS)
		return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) does not hold whole pairs", (unsigned long long)bad,
		            (unsigned long long)pair_ranges[2 * bad], (unsigned long long)pair_ranges[2 * bad + 1]);
	if (fault == PAIR_RANGE_OVERLAPS)
		return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) starts before range %llu ends: ranges are ascending and disjoint",
		            (unsigned long long)bad, (unsigned long long)pair_ranges[2 * bad], (unsigned long long)pair_ranges[2 * bad + 1],
		            (unsigned long long)(bad - 1));
	rc = kept_ready(c);
	if (rc != SDT_OK) return rc;
	if (c->staged_head < c->staged.size())
		return fail(SDT_ESTATE, "sdt_gpu_overlap_kept_pairs: batches were pushed and not drained: call sdt_gpu_finish_count first");
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "ov", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!ov)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	std::vector<UnitStretch> segs(2 * n_ranges + 1);
	uint64_t units = 0;
	segs.resize(cut_unit_stretches(pair_ranges, n_ranges, nord, segs.data(), &units));
	// mates sit in different kept batches: the entries and the records of ALL ordinals are on the device at once, the records preset
	// to "no read".  The entries are k_read_fp's (sdt_dedup_kernels.cuh): where an ordinal's bases are; the fingerprint in them is not used.
	DevBuf d_ent, d_ov, d_segs, ctr;
	rc = d_ent.get(nord * sizeof(DedupEnt), "overlap entries");
	if (rc == SDT_OK) rc = d_ov.get(nord * sizeof(ReadOverlap), "overlap records");
	if (rc == SDT_OK) rc = d_segs.get(segs.size() * sizeof(UnitStretch), "overlap units");
	if (rc == SDT_OK) rc = ctr.get(sizeof(unsigned long long), "overlap counter");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_ent.p, 0, nord * sizeof(DedupEnt), c->stream));
	HIPCHK(hipMemsetAsync(d_ov.p, 0xFF, nord * sizeof(ReadOverlap), c->stream));
	HIPCHK(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(UnitStretch), hipMemcpyHostToDevice, c->stream));
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		hipLaunchKernelGGL(k_read_fp, dim3(wave_grid(c, kb.nreads)), dim3(TPB), 0, c->stream, kb.d_words, kb.d_offs, kb.nreads, (uint64_t *)nullptr,
		                   (DedupEnt *)d_ent.p, kb.ord_base, kb.ord_stride);
		HIPCHK(hipGetLastError());
	}
	uint64_t kept = 0;
	const KeptReads reads = {(const DedupEnt *)d_ent.p, nord};
	const Units U = {(const UnitStretch *)d_segs.p, (uint32_t)segs.size(), UnitStretch{0, 0, 1}, units};
	rc = overlap_launch(c, reads, U, total, params, (ReadOverlap *)d_ov.p, nullptr, (unsigned long long *)ctr.p, &kept);      // (waits: segs may go)
	if (rc != SDT_OK) return rc;
	// back in blocks; the records of ordinals that no kept read has stay as the caller had them
	const uint64_t block = 1ULL << 22;
	std::vector<ReadOverlap> tmp((size_t)(nord < block ? nord : block));
	for (uint64_t o0 = 0; o0 < nord; o0 += block) {
		const uint64_t k = nord - o0 < block ? nord - o0 : block;
		HIPCHK(hipMemcpy(tmp.data(), (const ReadOverlap *)d_ov.p + o0, k * sizeof(ReadOverlap), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < k; i++)
			if (tmp[i].verdict != OVERLAP_ABSENT) memcpy(ov + o0 + i, &tmp[i], sizeof(ReadOverlap));
	}
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
