// sdt_select.hip -- in-silico read normalisation against the counted node table (the rule: include/sdt_gpu.h) = k_pick_stats +
// k_pick_decide, and the compaction of a 2-bit stream to the reads that were kept = k_compact_place + k_compact_words.  Nothing here
// writes the table or the kept reads.  State rules, staging in pieces and the high halves of the counts are sdt_search.hip's.
#include "sdt_compact.hpp"

// enqueue k_pick_stats for one device-resident batch; d_cov_flags[0] counts the reads longer than max_read_len
static int launch_pick_stats(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                             uint32_t max_cv_pct, ReadPick *d_pick, uint64_t out_base, uint64_t out_stride)
{
	HiView hv;
	int rc = hi_prepare(c, &hv);
	if (rc != SDT_OK) return rc;
	if (max_read_len < (uint64_t)c->K) max_read_len = (uint64_t)c->K;
	const uint64_t mk = max_read_len - c->K + 1;
	const size_t per_wave = (size_t)mk * sizeof(uint32_t);
	if (per_wave > 64 * 1024)
		return fail(SDT_EINVAL, "reads of %llu bases do not fit the per-wavefront LDS strip (%llu k-mers, 16384 at most)",
		            (unsigned long long)max_read_len, (unsigned long long)mk);
	int waves = 4;
	while (waves > 1 && per_wave * waves > 64 * 1024) waves >>= 1;
	uint64_t blocks = (nreads + waves - 1) / waves;
	const uint64_t cap = (uint64_t)c->cu_count * 32;
	if (blocks > cap) blocks = cap;
	if (blocks == 0) blocks = 1;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
#define PICK_LAUNCH(NWV) hipLaunchKernelGGL(k_pick_stats<NWV>, dim3((unsigned)blocks), dim3(TPB), per_wave * waves, c->stream, d_words, d_offs, nreads, \
	c->K, table_of<NWV>(c), hv, max_cv_pct, (int)mk, waves, d_pick, out_base, out_stride, c->d_cov_flags)
	if (c->nw == 1) PICK_LAUNCH(1);
	else if (c->nw == 2) PICK_LAUNCH(2);
	else PICK_LAUNCH(4);
#undef PICK_LAUNCH
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads * mk;                         // (an upper bound, as for the count kernels)
	}
	return SDT_OK;
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
	int rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags + 2, 0, sizeof(unsigned long long), c->stream));
	rc = launch_pick_stats(c, d_words, d_offs, nreads, max_read_len, p->max_cv_pct, d_pick, 0, 1);
	if (rc != SDT_OK) return rc;
	const UnitSeg dense = {0, 0, paired ? 2ULL : 1ULL};
	rc = launch_pick_decide(c, d_pick, nreads, nullptr, 0, dense, paired ? nreads / 2 : nreads, id_base, p, d_keep);
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_kept) *n_kept += fl[2];
	if (fl[0])
		return fail(SDT_EINVAL, "sdt_gpu_select_reads: %llu reads are longer than max_read_len = %llu; their records have kmers = 0xFFFFFFFF",
		            fl[0], (unsigned long long)max_read_len);
	return SDT_OK;
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
	HIPCHK(hipSetDevice(c->device));
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
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	if (((offsets[nreads] + 15) >> 4) + TAIL_PAD > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)(((offsets[nreads] + 15) >> 4) + TAIL_PAD), TAIL_PAD);
	HIPCHK(hipSetDevice(c->device));
	// in pieces, as sdt_gpu_profile_reads stages them; a piece of a paired batch holds whole pairs, and a unit's id in the draw is the
	// index of its first read in the whole batch
	const uint64_t step = paired ? 2 : 1;
	uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	if (paired) piece_reads = piece_reads < 2 ? 2 : piece_reads & ~1ULL;
	std::vector<uint64_t> rel;
	DevBuf d_w, d_o, d_r, d_k;
	uint64_t cap_w = 0, cap_r = 0, kept = 0;
	for (uint64_t r0 = 0; r0 < nreads;) {
		uint64_t r1 = r0, maxlen = 0;
		while (r1 < nreads && (r1 == r0 || (r1 - r0 < piece_reads && offsets[r1 + step] - offsets[r0] <= PROFILE_CHUNK_BASES))) {
			for (uint64_t i = r1; i < r1 + step; i++)
				if (offsets[i + 1] - offsets[i] > maxlen) maxlen = offsets[i + 1] - offsets[i];
			r1 += step;
		}
		const uint64_t w0 = offsets[r0] >> 4, w1 = ((offsets[r1] + 15) >> 4) + TAIL_PAD, nw = w1 - w0, nr = r1 - r0;
		rel.resize(nr + 1);
		for (uint64_t i = 0; i <= nr; i++) rel[i] = offsets[r0 + i] - (w0 << 4);
		if (cap_w < nw || cap_r < nr) {
			HIPCHK(hipStreamSynchronize(c->stream));
			cap_w = nw; cap_r = nr;
			rc = d_w.get(cap_w * sizeof(uint32_t), "selection staging");
			if (rc == SDT_OK) rc = d_o.get((cap_r + 1) * sizeof(uint64_t), "selection staging");
			if (rc == SDT_OK) rc = d_r.get(cap_r * sizeof(ReadPick), "selection staging");
			if (rc == SDT_OK) rc = d_k.get(cap_r, "selection staging");
			if (rc != SDT_OK) return rc;
		}
		HIPCHK(hipMemcpyAsync(d_w.p, packed_words + w0, nw * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, rel.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		rc = select_device(c, (const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nr, maxlen, paired, params, (ReadPick *)d_r.p, (uint8_t *)d_k.p,
		                   r0, &kept);                                   // (waits for the kernels: rel may be refilled)
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(pick + r0, d_r.p, nr * sizeof(ReadPick), hipMemcpyDeviceToHost));
		if (keep) HIPCHK(hipMemcpy(keep + r0, d_k.p, nr, hipMemcpyDeviceToHost));
		r0 = r1;
	}
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

int sdt_gpu_select_kept_reads(sdt_ctx *c, const sdt_norm_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                              sdt_read_pick *pick, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = params_ok(params, 0, 0);
	if (rc != SDT_OK) return rc;
	if (n_ranges && !pair_ranges)
		return fail(SDT_EINVAL, "NULL argument");
	for (uint64_t i = 0; i < n_ranges; i++) {
		const uint64_t first = pair_ranges[2 * i], end = pair_ranges[2 * i + 1];
		if (end < first || ((end - first) & 1))
			return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) does not hold whole pairs", (unsigned long long)i, (unsigned long long)first,
			            (unsigned long long)end);
		if (i && first < pair_ranges[2 * i - 1])
			return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) starts before range %llu ends: ranges are ascending and disjoint",
			            (unsigned long long)i, (unsigned long long)first, (unsigned long long)end, (unsigned long long)(i - 1));
	}
	rc = search_ready(c, "sdt_gpu_select_kept_reads");
	if (rc != SDT_OK) return rc;
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	uint64_t total = 0, npick = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (last >= out_capacity)
			return fail(SDT_EFULL, "a kept read has ordinal %llu, pick[] holds %llu records", (unsigned long long)last, (unsigned long long)out_capacity);
		total += kb.nreads;
		if (last + 1 > npick) npick = last + 1;
	}
	if (total == 0)
		return SDT_OK;
	if (!pick)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipSetDevice(c->device));
	rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// the unit list, as stretches: single reads up to a range, the pairs of the range, and so on up to the last ordinal a read has
	std::vector<UnitSeg> segs;
	uint64_t units = 0, at = 0;
	for (uint64_t i = 0; i < n_ranges && at < npick; i++) {
		const uint64_t first = pair_ranges[2 * i], end = pair_ranges[2 * i + 1] < npick ? pair_ranges[2 * i + 1] : npick;
		if (first >= npick || end == first) continue;
		if (first > at) {
			segs.push_back({units, at, 1});
			units += first - at;
		}
		segs.push_back({units, first, 2});
		units += (end - first + 1) >> 1;                 // (npick may cut a pair: its first mate is a unit, the kernel finds no second)
		at = pair_ranges[2 * i + 1];
	}
	if (at < npick) {
		segs.push_back({units, at, 1});
		units += npick - at;
	}
	// records by ordinal on the device, preset to "no read": every kept batch fills in its own, then the units are decided
	DevBuf d_pick, d_segs;
	rc = d_pick.get(npick * sizeof(ReadPick), "selection records");
	if (rc == SDT_OK) rc = d_segs.get(segs.size() * sizeof(UnitSeg), "selection units");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_pick.p, 0xFF, npick * sizeof(ReadPick), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags + 2, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(UnitSeg), hipMemcpyHostToDevice, c->stream));
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = launch_pick_stats(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, params->max_cv_pct, (ReadPick *)d_pick.p, kb.ord_base, kb.ord_stride);
		if (rc != SDT_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
	}
	rc = launch_pick_decide(c, (ReadPick *)d_pick.p, npick, (const UnitSeg *)d_segs.p, (uint32_t)segs.size(), UnitSeg{0, 0, 1}, units, 0, params, nullptr);
	unsigned long long fl[3] = {0, 0, 0};
	if (rc == SDT_OK) HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));             // (segs may go)
	if (rc != SDT_OK) return rc;
	if (fl[0])
		return fail(SDT_EINVAL, "sdt_gpu_select_kept_reads: %llu kept reads are longer than their batch says", fl[0]);
	// back in blocks; the records of ordinals that no kept read has stay as the caller had them
	const uint64_t block = 1ULL << 22;
	std::vector<ReadPick> tmp((size_t)(npick < block ? npick : block));
	for (uint64_t o0 = 0; o0 < npick; o0 += block) {
		const uint64_t k = npick - o0 < block ? npick - o0 : block;
		HIPCHK(hipMemcpy(tmp.data(), (const ReadPick *)d_pick.p + o0, k * sizeof(ReadPick), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < k; i++)
			if (tmp[i].verdict != PICK_ABSENT) memcpy(pick + o0 + i, &tmp[i], sizeof(ReadPick));
	}
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
	HIPCHK(hipSetDevice(c->device));
	return compact_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (const uint8_t *)d_keep,
	                      (uint32_t *)d_out_words, out_words_cap, (uint64_t *)d_out_offsets, n_out_reads, n_out_words);
}

int sdt_gpu_compact_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                          const uint8_t *keep, uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets, uint64_t *n_out_reads,
                          uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!out_words || !out_offsets || (nreads && (!packed_words || !offsets || !keep)))
		return fail(SDT_EINVAL, "NULL argument");
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	const uint64_t in_words = nreads ? ((offsets[nreads] + 15) >> 4) + TAIL_PAD : 0;
	if (in_words > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)in_words, TAIL_PAD);
	// what the output takes is known here already: nothing is staged for an output that does not fit
	uint64_t bases = 0, kept = 0;
	for (uint64_t i = 0; i < nreads; i++)
		if (keep[i]) { bases += offsets[i + 1] - offsets[i]; kept++; }
	const uint64_t need = (bases + 15) >> 4;
	if (out_words_cap < need + TAIL_PAD) {
		if (n_out_reads) *n_out_reads = kept;
		if (n_out_words) *n_out_words = need;
		return fail(SDT_EFULL, "sdt_gpu_compact_reads: the kept reads take %llu words and %d pad words, out_words holds %llu",
		            (unsigned long long)need, TAIL_PAD, (unsigned long long)out_words_cap);
	}
	HIPCHK(hipSetDevice(c->device));
	// the whole stream at once: the output of pieces would meet in the middle of words
	DevBuf d_w, d_o, d_k, d_ow, d_oo;
	int rc = d_w.get(in_words * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc == SDT_OK) rc = d_k.get(nreads, "compaction staging");
	if (rc == SDT_OK) rc = d_ow.get((need + TAIL_PAD) * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_oo.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc != SDT_OK) return rc;
	const uint64_t zero = 0;
	if (nreads) {
		HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_k.p, keep, nreads, hipMemcpyHostToDevice, c->stream));
	} else {
		HIPCHK(hipMemcpyAsync(d_o.p, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
	}
	uint64_t got_reads = 0, got_words = 0;
	rc = compact_device(c, (const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nreads, (const uint8_t *)d_k.p, (uint32_t *)d_ow.p, need + TAIL_PAD,
	                    (uint64_t *)d_oo.p, &got_reads, &got_words);
	if (rc != SDT_OK) return rc;
	if (got_reads != kept || got_words != need)
		return fail(SDT_EHIP, "sdt_gpu_compact_reads: the device kept %llu reads in %llu words, the host counted %llu in %llu",
		            (unsigned long long)got_reads, (unsigned long long)got_words, (unsigned long long)kept, (unsigned long long)need);
	HIPCHK(hipMemcpy(out_words, d_ow.p, (need + TAIL_PAD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_offsets, d_oo.p, (kept + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (n_out_reads) *n_out_reads = kept;
	if (n_out_words) *n_out_words = need;
	return SDT_OK;
}

} // extern "C"
