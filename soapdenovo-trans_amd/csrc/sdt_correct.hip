// sdt_correct.hip -- k-mer-spectrum correction of substitution errors in reads against the counted node table = k_correct_reads
// (the rule: include/sdt_gpu.h), and the way back to the host for the reads kept in HBM.  Nothing here writes the table or the
// kept reads.  State rules, staging in pieces and the high halves of the counts are sdt_search.hip's.
#include "sdt_ctx.hpp"
#include "sdt_correct_kernels.cuh"
#include <algorithm>

// enqueue k_correct_reads for one device-resident batch; d_cov_flags[0] counts the reads longer than max_read_len, [2] the edits
static int launch_correct(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                          uint32_t min_count, ReadFix *d_fix, uint32_t *d_out, unsigned long long *d_edits, uint64_t max_edits,
                          uint64_t edit_base, uint64_t edit_stride)
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
#define CORRECT_LAUNCH(NWV) hipLaunchKernelGGL(k_correct_reads<NWV>, dim3((unsigned)blocks), dim3(TPB), per_wave * waves, c->stream, d_words, d_offs, nreads, \
	c->K, table_of<NWV>(c), hv, min_count, (int)mk, waves, d_fix, d_out, d_edits, (unsigned long long)max_edits, c->d_cov_flags + 2,          \
	edit_base, edit_stride, c->d_cov_flags)
	if (c->nw == 1) CORRECT_LAUNCH(1);
	else if (c->nw == 2) CORRECT_LAUNCH(2);
	else CORRECT_LAUNCH(4);
#undef CORRECT_LAUNCH
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads * mk;                         // (an upper bound, as for the count kernels)
	}
	return SDT_OK;
}

// one device-resident batch, checked arguments: the copy of the stream, the kernel, and the wait for its two counters
static int correct_device(sdt_ctx *c, const uint32_t *d_words, uint64_t nwords, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                          uint32_t min_count, ReadFix *d_fix, uint32_t *d_out, unsigned long long *d_edits, uint64_t max_edits,
                          uint64_t edit_base, uint64_t edit_stride, uint64_t *n_edits)
{
	int rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags + 2, 0, sizeof(unsigned long long), c->stream));
	if (d_out) HIPCHK(hipMemcpyAsync(d_out, d_words, nwords * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
	rc = launch_correct(c, d_words, d_offs, nreads, max_read_len, min_count, d_fix, d_out, d_edits, d_edits ? max_edits : 0, edit_base, edit_stride);
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_edits) *n_edits = fl[2];
	if (fl[0])
		return fail(SDT_EINVAL, "sdt_gpu_correct_reads: %llu reads are longer than max_read_len = %llu; their records have kmers = 0xFFFFFFFF",
		            fl[0], (unsigned long long)max_read_len);
	if (d_edits && fl[2] > max_edits)
		return fail(SDT_EFULL, "sdt_gpu_correct_reads: %llu edits, edits[] holds %llu", fl[2], (unsigned long long)max_edits);
	return SDT_OK;
}

// a batch whose number of edits nobody knows: the list grows to what the kernel asked for and the batch runs once more
struct EditBuf {
	unsigned long long *d = nullptr;
	uint64_t cap = 0;
	~EditBuf() { if (d) (void)hipFree(d); }
};
static int correct_device_grow(sdt_ctx *c, const uint32_t *d_words, uint64_t nwords, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                               uint32_t min_count, ReadFix *d_fix, EditBuf *eb, uint64_t edit_base, uint64_t edit_stride,
                               std::vector<uint64_t> *all)
{
	for (int attempt = 0; attempt < 2; attempt++) {
		if (eb->cap == 0) {
			eb->cap = nreads / 4 + 1024;
			HIPCHK(hipMalloc((void **)&eb->d, eb->cap * sizeof(unsigned long long)));
		}
		uint64_t got = 0;
		const int rc = correct_device(c, d_words, nwords, d_offs, nreads, max_read_len, min_count, d_fix, nullptr, eb->d, eb->cap, edit_base,
		                              edit_stride, &got);
		if (rc == SDT_EFULL && got > eb->cap && attempt == 0) {
			HIPCHK(hipFree(eb->d));
			eb->d = nullptr;
			eb->cap = 0;
			HIPCHK(hipMalloc((void **)&eb->d, got * sizeof(unsigned long long)));
			eb->cap = got;
			continue;
		}
		if (rc != SDT_OK) return rc;
		const size_t at = all->size();
		all->resize(at + got);
		if (got) HIPCHK(hipMemcpy(all->data() + at, eb->d, got * sizeof(uint64_t), hipMemcpyDeviceToHost));
		return SDT_OK;
	}
	return fail(SDT_EHIP, "sdt_gpu_correct_reads: the number of edits changed between two runs of one batch");
}

// the sorted edits to the caller: all of them counted, as many as fit stored
static int hand_over_edits(std::vector<uint64_t> &all, uint64_t *edits, uint64_t max_edits, uint64_t *n_edits, const char *what)
{
	std::sort(all.begin(), all.end());
	if (n_edits) *n_edits = all.size();
	if (!edits) return SDT_OK;
	const uint64_t k = all.size() < max_edits ? all.size() : max_edits;
	if (k) memcpy(edits, all.data(), k * sizeof(uint64_t));
	if (all.size() > max_edits)
		return fail(SDT_EFULL, "%s: %llu edits, edits[] holds %llu", what, (unsigned long long)all.size(), (unsigned long long)max_edits);
	return SDT_OK;
}

extern "C" {

int sdt_gpu_correct_reads_device(sdt_ctx *c, const void *d_packed_words, uint64_t nwords, const void *d_offsets, uint64_t nreads,
                                 uint64_t max_read_len, uint32_t min_count, void *d_fix, void *d_out_words, void *d_edits, uint64_t max_edits,
                                 uint64_t *n_edits)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_edits) *n_edits = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_fix)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_correct_reads");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipSetDevice(c->device));
	return correct_device(c, (const uint32_t *)d_packed_words, nwords, (const uint64_t *)d_offsets, nreads, max_read_len, min_count,
	                      (ReadFix *)d_fix, (uint32_t *)d_out_words, (unsigned long long *)d_edits, max_edits, 0, 1, n_edits);
}

int sdt_gpu_correct_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                          uint32_t min_count, sdt_read_fix *fix, uint32_t *out_words, uint64_t *edits, uint64_t max_edits, uint64_t *n_edits)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_edits) *n_edits = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !fix)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_correct_reads");
	if (rc != SDT_OK) return rc;
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	if (((offsets[nreads] + 15) >> 4) + TAIL_PAD > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)(((offsets[nreads] + 15) >> 4) + TAIL_PAD), TAIL_PAD);
	HIPCHK(hipSetDevice(c->device));
	// in pieces, as sdt_gpu_profile_reads stages them: a run of reads, the words that hold them (offsets rebased to the piece's first
	// word) and their records; the edits of a piece name its reads from 0
	const uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	std::vector<uint64_t> rel, all;
	uint32_t *d_w = nullptr;
	uint64_t *d_o = nullptr;
	ReadFix *d_r = nullptr;
	EditBuf eb;
	uint64_t cap_w = 0, cap_r = 0;
	for (uint64_t r0 = 0; r0 < nreads && rc == SDT_OK;) {
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
			if (d_w) (void)hipFree(d_w);
			if (d_o) (void)hipFree(d_o);
			if (d_r) (void)hipFree(d_r);
			d_w = nullptr; d_o = nullptr; d_r = nullptr;
			cap_w = nw; cap_r = nr;
			hipError_t e = hipMalloc((void **)&d_w, cap_w * sizeof(uint32_t));
			if (e == hipSuccess) e = hipMalloc((void **)&d_o, (cap_r + 1) * sizeof(uint64_t));
			if (e == hipSuccess) e = hipMalloc((void **)&d_r, cap_r * sizeof(ReadFix));
			if (e != hipSuccess) { rc = fail(SDT_ENOMEM, "correction staging: %s", hipGetErrorString(e)); break; }
		}
		hipError_t e = hipMemcpyAsync(d_w, packed_words + w0, nw * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(d_o, rel.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "correction staging: %s", hipGetErrorString(e)); break; }
		rc = correct_device_grow(c, d_w, nw, d_o, nr, maxlen, min_count, d_r, &eb, r0, 1, &all);      // (waits for the kernel: rel may be refilled)
		if (rc != SDT_OK) break;
		e = hipMemcpy(fix + r0, d_r, nr * sizeof(ReadFix), hipMemcpyDeviceToHost);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "correction records: %s", hipGetErrorString(e)); break; }
		r0 = r1;
	}
	if (d_w) (void)hipFree(d_w);
	if (d_o) (void)hipFree(d_o);
	if (d_r) (void)hipFree(d_r);
	if (rc != SDT_OK) return rc;
	// the corrected stream on the host: a piece may start in a word that also holds the previous read's last bases, so the words
	// of the pieces are not put together -- the edits are applied to a copy of the input
	if (out_words) {
		memcpy(out_words, packed_words, nwords * sizeof(uint32_t));
		for (const uint64_t e : all) {
			const uint64_t g = offsets[e >> 18] + ((e >> 2) & 0xFFFFu);
			const int sh = 30 - 2 * (int)(g & 15);
			out_words[g >> 4] = (out_words[g >> 4] & ~(3u << sh)) | ((uint32_t)(e & 3u) << sh);
		}
	}
	return hand_over_edits(all, edits, max_edits, n_edits, "sdt_gpu_correct_reads");
}

int sdt_gpu_correct_kept_reads(sdt_ctx *c, uint32_t min_count, sdt_read_fix *fix, uint64_t out_capacity, uint64_t *nreads,
                               uint64_t *edits, uint64_t max_edits, uint64_t *n_edits)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	if (n_edits) *n_edits = 0;
	int rc = search_ready(c, "sdt_gpu_correct_kept_reads");
	if (rc != SDT_OK) return rc;
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	uint64_t total = 0, most = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (last >= out_capacity)
			return fail(SDT_EFULL, "a kept read has ordinal %llu, fix[] holds %llu records", (unsigned long long)last, (unsigned long long)out_capacity);
		if (last >> 46)
			return fail(SDT_ELIMIT, "a kept read has ordinal %llu: an edit holds 46 bits of it", (unsigned long long)last);
		total += kb.nreads;
		if (kb.nreads > most) most = kb.nreads;
	}
	if (total == 0)
		return SDT_OK;
	if (!fix)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// batch by batch: dense records on the device, scattered to their ordinals on the host (nothing else of fix[] is touched)
	ReadFix *d_r = nullptr;
	HIPCHK(hipMalloc((void **)&d_r, most * sizeof(ReadFix)));
	std::vector<ReadFix> tmp(most);
	std::vector<uint64_t> all;
	EditBuf eb;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = correct_device_grow(c, kb.d_words, kb.nwords, kb.d_offs, kb.nreads, kb.maxlen, min_count, d_r, &eb, kb.ord_base, kb.ord_stride, &all);
		if (rc != SDT_OK) break;
		const hipError_t e = hipMemcpy(tmp.data(), d_r, kb.nreads * sizeof(ReadFix), hipMemcpyDeviceToHost);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "correction records: %s", hipGetErrorString(e)); break; }
		for (uint64_t i = 0; i < kb.nreads; i++)
			memcpy(fix + (kb.ord_base + i * kb.ord_stride), &tmp[i], sizeof(ReadFix));
	}
	(void)hipFree(d_r);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	return hand_over_edits(all, edits, max_edits, n_edits, "sdt_gpu_correct_kept_reads");
}

int sdt_gpu_kept_batches(const sdt_ctx *c, uint64_t *n)
{
	if (!c || !n)
		return fail(SDT_EINVAL, "NULL argument");
	*n = c->kept.size();
	return SDT_OK;
}

int sdt_gpu_fetch_kept_batch(sdt_ctx *c, uint64_t i, uint64_t info[4], uint32_t *words, uint64_t words_cap, uint64_t *offsets,
                             uint64_t offsets_cap)
{
	if (!c || !info)
		return fail(SDT_EINVAL, "NULL argument");
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	if (i >= c->kept.size())
		return fail(SDT_EINVAL, "kept batch %llu of %zu", (unsigned long long)i, c->kept.size());
	if (c->staged_head < c->staged.size())
		return fail(SDT_ESTATE, "sdt_gpu_fetch_kept_batch: batches were pushed and not drained: call sdt_gpu_finish_count first");
	const sdt_ctx::KeptBatch &kb = c->kept[i];
	info[0] = kb.nwords;
	info[1] = kb.nreads;
	info[2] = kb.ord_base;
	info[3] = kb.ord_stride;
	if (!words && !offsets)
		return SDT_OK;
	if ((words && words_cap < kb.nwords) || (offsets && offsets_cap < kb.nreads + 1))
		return fail(SDT_EFULL, "kept batch %llu has %llu words and %llu offsets", (unsigned long long)i, (unsigned long long)kb.nwords,
		            (unsigned long long)(kb.nreads + 1));
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (the uploads) and the offsets of a fixed-length batch, made on the device
	HIPCHK(hipStreamSynchronize(c->stream));
	if (words) HIPCHK(hipMemcpy(words, kb.d_words, kb.nwords * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (offsets) HIPCHK(hipMemcpy(offsets, kb.d_offs, (kb.nreads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return SDT_OK;
}

} // extern "C"
