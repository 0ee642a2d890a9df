// sdt_trim.hip -- reads cut back to their longest solid stretch against the counted node table (the rule: include/sdt_gpu.h) =
// k_trim_reads, and the compaction of a 2-bit stream to the kept range of every read = k_trim_place + k_compact_words.  Nothing here
// writes the table or the kept reads.  State rules, staging in pieces and the high halves of the counts are sdt_search.hip's.
#include "sdt_compact.hpp"
#include "sdt_trim_kernels.cuh"

static_assert(sizeof(sdt_read_trim) == sizeof(ReadTrim) && sizeof(sdt_trim_params) == sizeof(TrimParams), "include/sdt_gpu.h and the kernels agree");

// enqueue k_trim_reads for one device-resident batch; d_cov_flags[0] counts the reads longer than max_read_len, [2] the reads kept
static int launch_trim(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                       const sdt_trim_params *p, ReadTrim *d_trim, uint8_t *d_keep)
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
	const TrimParams prm = {p->min_count, p->min_cov, p->min_len, p->flags};
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
#define TRIM_LAUNCH(NWV) hipLaunchKernelGGL(k_trim_reads<NWV>, dim3((unsigned)blocks), dim3(TPB), per_wave * waves, c->stream, d_words, d_offs, nreads, \
	c->K, table_of<NWV>(c), hv, prm, (int)mk, waves, d_trim, d_keep, c->d_cov_flags, c->d_cov_flags + 2)
	if (c->nw == 1) TRIM_LAUNCH(1);
	else if (c->nw == 2) TRIM_LAUNCH(2);
	else TRIM_LAUNCH(4);
#undef TRIM_LAUNCH
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads * mk;                         // (an upper bound, as for the count kernels)
	}
	return SDT_OK;
}

// one dense device-resident batch, checked arguments: the kernel and the wait for its two counters
static int trim_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                       const sdt_trim_params *p, ReadTrim *d_trim, uint8_t *d_keep, uint64_t *n_kept)
{
	int rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags + 2, 0, sizeof(unsigned long long), c->stream));
	rc = launch_trim(c, d_words, d_offs, nreads, max_read_len, p, d_trim, d_keep);
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_kept) *n_kept += fl[2];
	if (fl[0])
		return fail(SDT_EINVAL, "sdt_gpu_trim_reads: %llu reads are longer than max_read_len = %llu; their records have kmers = 0xFFFFFFFF",
		            fl[0], (unsigned long long)max_read_len);
	return SDT_OK;
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
	HIPCHK(hipSetDevice(c->device));
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
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	if (((offsets[nreads] + 15) >> 4) + TAIL_PAD > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)(((offsets[nreads] + 15) >> 4) + TAIL_PAD), TAIL_PAD);
	HIPCHK(hipSetDevice(c->device));
	// in pieces, as sdt_gpu_profile_reads stages them
	const uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	std::vector<uint64_t> rel;
	DevBuf d_w, d_o, d_r, d_k;
	uint64_t cap_w = 0, cap_r = 0, kept = 0;
	for (uint64_t r0 = 0; r0 < nreads;) {
		uint64_t r1 = r0 + 1, maxlen = offsets[r1] - offsets[r0];
		while (r1 < nreads && r1 - r0 < piece_reads && offsets[r1 + 1] - offsets[r0] <= PROFILE_CHUNK_BASES) {
			if (offsets[r1 + 1] - offsets[r1] > maxlen) maxlen = offsets[r1 + 1] - offsets[r1];
			r1++;
		}
		const uint64_t w0 = offsets[r0] >> 4, w1 = ((offsets[r1] + 15) >> 4) + TAIL_PAD, nw = w1 - w0, nr = r1 - r0;
		rel.resize(nr + 1);
		for (uint64_t i = 0; i <= nr; i++) rel[i] = offsets[r0 + i] - (w0 << 4);
		if (cap_w < nw || cap_r < nr) {
			HIPCHK(hipStreamSynchronize(c->stream));
			cap_w = nw; cap_r = nr;
			rc = d_w.get(cap_w * sizeof(uint32_t), "trim staging");
			if (rc == SDT_OK) rc = d_o.get((cap_r + 1) * sizeof(uint64_t), "trim staging");
			if (rc == SDT_OK) rc = d_r.get(cap_r * sizeof(ReadTrim), "trim staging");
			if (rc == SDT_OK) rc = d_k.get(cap_r, "trim staging");
			if (rc != SDT_OK) return rc;
		}
		HIPCHK(hipMemcpyAsync(d_w.p, packed_words + w0, nw * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, rel.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		rc = trim_device(c, (const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nr, maxlen, params, (ReadTrim *)d_r.p, (uint8_t *)d_k.p,
		                 &kept);                                         // (waits for the kernel: rel may be refilled)
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(trim + r0, d_r.p, nr * sizeof(ReadTrim), hipMemcpyDeviceToHost));
		if (keep) HIPCHK(hipMemcpy(keep + r0, d_k.p, nr, hipMemcpyDeviceToHost));
		r0 = r1;
	}
	if (n_kept) *n_kept = kept;
	return SDT_OK;
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
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	uint64_t total = 0, most = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (last >= out_capacity)
			return fail(SDT_EFULL, "a kept read has ordinal %llu, trim[] holds %llu records", (unsigned long long)last, (unsigned long long)out_capacity);
		total += kb.nreads;
		if (kb.nreads > most) most = kb.nreads;
	}
	if (total == 0)
		return SDT_OK;
	if (!trim)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// batch by batch: dense records on the device, scattered to their ordinals on the host (nothing else of trim[] is touched)
	DevBuf d_r;
	rc = d_r.get(most * sizeof(ReadTrim), "trim records");
	if (rc != SDT_OK) return rc;
	std::vector<ReadTrim> tmp(most);
	uint64_t kept = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = trim_device(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, params, (ReadTrim *)d_r.p, nullptr, &kept);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(tmp.data(), d_r.p, kb.nreads * sizeof(ReadTrim), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < kb.nreads; i++)
			memcpy(trim + (kb.ord_base + i * kb.ord_stride), &tmp[i], sizeof(ReadTrim));
	}
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
	HIPCHK(hipSetDevice(c->device));
	return compact_trimmed_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, (const ReadTrim *)d_trim,
	                              (uint32_t *)d_out_words, out_words_cap, (uint64_t *)d_out_offsets, n_out_reads, n_out_words);
}

int sdt_gpu_compact_trimmed(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                            const sdt_read_trim *trim, uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets,
                            uint64_t *n_out_reads, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_reads) *n_out_reads = 0;
	if (n_out_words) *n_out_words = 0;
	if (!out_words || !out_offsets || (nreads && (!packed_words || !offsets || !trim)))
		return fail(SDT_EINVAL, "NULL argument");
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	const uint64_t in_words = nreads ? ((offsets[nreads] + 15) >> 4) + TAIL_PAD : 0;
	if (in_words > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)in_words, TAIL_PAD);
	// every range lies in its read, and what the output takes is known here already: nothing is staged for an output that does not fit
	uint64_t bases = 0, kept = 0;
	for (uint64_t i = 0; i < nreads; i++) {
		if ((uint64_t)trim[i].start + trim[i].len > offsets[i + 1] - offsets[i])
			return fail(SDT_EINVAL, "read %llu has %llu bases, its record keeps [%u, %u + %u)", (unsigned long long)i,
			            (unsigned long long)(offsets[i + 1] - offsets[i]), trim[i].start, trim[i].start, trim[i].len);
		if (trim[i].len) { bases += trim[i].len; kept++; }
	}
	const uint64_t need = (bases + 15) >> 4;
	if (out_words_cap < need + TAIL_PAD) {
		if (n_out_reads) *n_out_reads = kept;
		if (n_out_words) *n_out_words = need;
		return fail(SDT_EFULL, "sdt_gpu_compact_trimmed: the kept reads take %llu words and %d pad words, out_words holds %llu",
		            (unsigned long long)need, TAIL_PAD, (unsigned long long)out_words_cap);
	}
	HIPCHK(hipSetDevice(c->device));
	// the whole stream at once: the output of pieces would meet in the middle of words
	DevBuf d_w, d_o, d_t, d_ow, d_oo;
	int rc = d_w.get(in_words * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc == SDT_OK) rc = d_t.get(nreads * sizeof(ReadTrim), "compaction staging");
	if (rc == SDT_OK) rc = d_ow.get((need + TAIL_PAD) * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_oo.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc != SDT_OK) return rc;
	const uint64_t zero = 0;
	if (nreads) {
		HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_t.p, trim, nreads * sizeof(ReadTrim), hipMemcpyHostToDevice, c->stream));
	} else {
		HIPCHK(hipMemcpyAsync(d_o.p, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
	}
	uint64_t got_reads = 0, got_words = 0;
	rc = compact_trimmed_device(c, (const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nreads, (const ReadTrim *)d_t.p, (uint32_t *)d_ow.p,
	                            need + TAIL_PAD, (uint64_t *)d_oo.p, &got_reads, &got_words);
	if (rc != SDT_OK) return rc;
	if (got_reads != kept || got_words != need)
		return fail(SDT_EHIP, "sdt_gpu_compact_trimmed: the device kept %llu reads in %llu words, the host counted %llu in %llu",
		            (unsigned long long)got_reads, (unsigned long long)got_words, (unsigned long long)kept, (unsigned long long)need);
	HIPCHK(hipMemcpy(out_words, d_ow.p, (need + TAIL_PAD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_offsets, d_oo.p, (kept + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (n_out_reads) *n_out_reads = kept;
	if (n_out_words) *n_out_words = need;
	return SDT_OK;
}

} // extern "C"
