// sdt_select.hip -- in-silico read normalisation against the counted node table (the rule: include/sdt_gpu.h) = k_pick_stats +
// k_pick_decide, and the compaction of a 2-bit stream to the reads that were kept = k_compact_place + k_compact_words.  Nothing here
// writes the table or the kept reads.  State rules and the high halves of the counts are sdt_search.hip's; launch geometry,
// staging in pieces and the checks of the kept batches are sdt_readstage.hpp's.
#include "sdt_compact.hpp"

// enqueue k_pick_stats for one device-resident batch: read i's record goes to d_pick[out_base + i * out_stride]
static int launch_pick_stats(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                             uint32_t max_cv_pct, ReadPick *d_pick, uint64_t out_base, uint64_t out_stride)
{
	return launch_strip(c, nreads, max_read_len, [&](auto nw, const StripGeometry &geo, const HiView &hv) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_pick_stats<NW>, dim3(geo.blocks), dim3(TPB), geo.lds_bytes, c->stream, d_words, d_offs, nreads, c->K, table_of<NW>(c),
		                   hv, max_cv_pct, (int)geo.mk, geo.waves, d_pick, out_base, out_stride, c->d_cov_flags);
	});
}

// enqueue k_pick_decide; d_cov_flags[2] counts the kept reads
static int launch_pick_decide(sdt_ctx *c, ReadPick *d_pick, uint64_t npick, const UnitSeg *d_segs, uint32_t nsegs, UnitSeg dense, uint64_t nunits,
                              uint64_t id_base, const sdt_norm_params *p, uint8_t *d_keep)
{
	if (!nunits) return SDT_OK;
	const int g = scan_grid(c, nunits);
	hipLaunchKernelGGL(k_pick_decide, dim3(g), dim3(TPB), 0, c->stream, d_pick, npick, d_segs, nsegs, dense, nunits, id_base, p->target, p->seed,
	                   d_keep, c->d_cov_flags + 2);
	HIPCHK(hipGetLastError());
	return SDT_OK;
}

// one dense device-resident batch, checked arguments: both kernels and the wait for their two counters.  id_base: the index of the
// batch's first read in the caller's numbering (a piece of a host batch).
static int select_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len, int paired,
                         const sdt_norm_params *p, ReadPick *d_pick, uint8_t *d_keep, uint64_t id_base, uint64_t *n_kept)
{
	int rc = flags_begin(c);
	if (rc != SDT_OK) return rc;
	rc = launch_pick_stats(c, d_words, d_offs, nreads, max_read_len, p->max_cv_pct, d_pick, 0, 1);
	if (rc != SDT_OK) return rc;
	const UnitSeg dense = {0, 0, paired ? 2ULL : 1ULL};
	rc = launch_pick_decide(c, d_pick, nreads, nullptr, 0, dense, paired ? nreads / 2 : nreads, id_base, p, d_keep);
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	rc = flags_end(c, "sdt_gpu_select_reads", max_read_len, fl);
	if (n_kept) *n_kept += fl[2];
	return rc;
}

static int params_ok(const sdt_norm_params *p, uint64_t nreads, int paired)
{
	if (!p)
		return fail(SDT_EINVAL, "NULL argument");
	if (p->target == 0)
		return fail(SDT_EINVAL, "target coverage 0: every read with a k-mer would be dropped");
	if (paired && (nreads & 1))
		return fail(SDT_EINVAL, "paired reads: reads 2t and 2t + 1 are mates, %llu reads is an odd number", (unsigned long long)nreads);
	return SDT_OK;
}

// the compaction of one device-resident stream to its kept reads, checked arguments
static int compact_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, const uint8_t *d_keep,
                          uint32_t *d_out_words, uint64_t out_words_cap, uint64_t *d_out_offs, uint64_t *n_out_reads, uint64_t *n_out_words)
{
	const auto place = [&](int grid, const uint64_t *new_off, const uint64_t *rank, uint64_t *src) {
		hipLaunchKernelGGL(k_compact_place, dim3(grid), dim3(TPB), 0, c->stream, d_keep, d_offs, nreads, new_off, rank, d_out_offs, src);
	};
	return compact_stream(c, "sdt_gpu_compact_reads", d_words, nreads, KeptLen{d_keep, d_offs, nreads}, KeptFlag{d_keep, nreads}, place,
	                      d_out_words, out_words_cap, d_out_offs, n_out_reads, n_out_words);
}

extern "C" {

int sdt_gpu_select_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, uint64_t max_read_len,
                                int paired, const sdt_norm_params *params, void *d_pick, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_pick)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = params_ok(params, nreads, paired);
	if (rc != SDT_OK) return rc;
	rc = search_ready(c, "sdt_gpu_select_reads");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return select_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, max_read_len, paired, params,
	                     (ReadPick *)d_pick, (uint8_t *)d_keep, 0, n_kept);
}

int sdt_gpu_select_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired,
                         const sdt_norm_params *params, sdt_read_pick *pick, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !pick)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = params_ok(params, nreads, paired);
	if (rc != SDT_OK) return rc;
	rc = search_ready(c, "sdt_gpu_select_reads");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	StripGeometry geo;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc == SDT_OK) rc = strip_plan(c, nreads, in.longest, &geo);      // (the whole call is refused before a piece's records are written)
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	// a piece of a paired batch holds whole pairs, and a unit's id in the draw is the index of its first read in the whole batch
	return staged_records<ReadPick>(c, packed_words, offsets, nreads, paired ? 2 : 1, "selection staging", pick, keep, n_kept,
	                                [&](const StagedPiece &p, ReadPick *d_r, uint8_t *d_k, uint64_t *kept) {
		return select_device(c, p.d_words, p.d_offs, p.nr, p.maxlen, paired, params, d_r, d_k, p.r0, kept);
	});
}

int sdt_gpu_select_kept_reads(sdt_ctx *c, const sdt_norm_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                              sdt_read_pick *pick, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = params_ok(params, 0, 0);
	if (rc == SDT_OK) rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_select_kept_reads");
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "pick", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!pick)
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// the unit list, as stretches: single reads up to a range, the pairs of the range, and so on up to the last ordinal a read has
	// (sdt_readstage.hpp: KeptUnits); records by ordinal on the device, preset to "no read": every kept batch fills in its own, then
	// the units are decided
	KeptUnits ku(pair_ranges, n_ranges, npick);
	DevBuf d_pick;
	rc = d_pick.get(npick * sizeof(ReadPick), "selection records");
	if (rc == SDT_OK) rc = ku.d_segs.get(ku.bytes(), "selection units");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_pick.p, 0xFF, npick * sizeof(ReadPick), c->stream));
	rc = flags_begin(c);
	if (rc == SDT_OK) rc = ku.upload(c);
	if (rc != SDT_OK) return rc;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = launch_pick_stats(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, params->max_cv_pct, (ReadPick *)d_pick.p, kb.ord_base, kb.ord_stride);
		if (rc != SDT_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
	}
	rc = launch_pick_decide(c, (ReadPick *)d_pick.p, npick, (const UnitSeg *)ku.d_segs.p, (uint32_t)ku.segs.size(), UnitSeg{0, 0, 1}, ku.units, 0, params,
	                        nullptr);
	unsigned long long fl[3] = {0, 0, 0};
	if (rc == SDT_OK) HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));             // (segs may go)
	if (rc != SDT_OK) return rc;
	if (fl[0])
		return fail(SDT_EINVAL, "sdt_gpu_select_kept_reads: %llu kept reads are longer than their batch says", fl[0]);
	rc = fetch_present<ReadPick>(pick, d_pick, npick, PICK_ABSENT);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = fl[2];
	return SDT_OK;
}

int sdt_gpu_compact_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const void *d_keep,
                                 void *d_out_words, uint64_t out_words_cap, void *d_out_offsets, uint64_t *n_out_reads, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!d_out_words || !d_out_offsets || (nreads && (!d_packed_words || !d_offsets || !d_keep)))
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	return compact_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (const uint8_t *)d_keep,
	                      (uint32_t *)d_out_words, out_words_cap, (uint64_t *)d_out_offsets, n_out_reads, n_out_words);
}

int sdt_gpu_compact_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                          const uint8_t *keep, uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets, uint64_t *n_out_reads,
                          uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!out_words || !out_offsets || (nreads && (!packed_words || !offsets || !keep)))
		return fail(SDT_EINVAL, "NULL argument");
	const auto tally = [&](uint64_t i, uint64_t &bases, uint64_t &kept) -> int {
		if (keep[i]) { bases += offsets[i + 1] - offsets[i]; kept++; }
		return SDT_OK;
	};
	const auto device = [&](const uint32_t *d_w, const uint64_t *d_o, const void *d_keep, uint32_t *d_ow, uint64_t cap, uint64_t *d_oo, uint64_t *reads,
	                        uint64_t *words) { return compact_device(c, d_w, d_o, nreads, (const uint8_t *)d_keep, d_ow, cap, d_oo, reads, words); };
	return compact_host(c, "sdt_gpu_compact_reads", packed_words, nwords, offsets, nreads, tally, keep, nreads, device, out_words, out_words_cap,
	                    out_offsets, n_out_reads, n_out_words);
}

} // extern "C"
