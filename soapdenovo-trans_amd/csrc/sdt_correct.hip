// sdt_correct.hip -- k-mer-spectrum correction of substitution errors in reads against the counted node table = k_correct_reads
// (the rule: include/sdt_gpu.h), and the way back to the host for the reads kept in HBM.  Nothing here writes the table or the
// kept reads.  State rules and the high halves of the counts are sdt_search.hip's; launch geometry, staging in pieces and the walk over
// the kept batches are sdt_readstage.hpp's.
#include "sdt_readstage.hpp"
#include "sdt_correct_kernels.cuh"
#include <algorithm>

// one device-resident batch, checked arguments: the copy of the stream, the kernel, and the wait for its two counters
// (d_cov_flags[2]: the edits)
static int correct_device(sdt_ctx *c, const uint32_t *d_words, uint64_t nwords, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                          uint32_t min_count, ReadFix *d_fix, uint32_t *d_out, unsigned long long *d_edits, uint64_t max_edits,
                          uint64_t edit_base, uint64_t edit_stride, uint64_t *n_edits)
{
	int rc = flags_begin(c);
	if (rc != SDT_OK) return rc;
	if (d_out) HIPCHK(hipMemcpyAsync(d_out, d_words, nwords * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
	const unsigned long long room = d_edits ? max_edits : 0;
	rc = launch_strip(c, nreads, max_read_len, [&](auto nw, const StripGeometry &geo, const HiView &hv) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_correct_reads<NW>, dim3(geo.blocks), dim3(TPB), geo.lds_bytes, c->stream, d_words, d_offs, nreads, c->K, table_of<NW>(c),
		                   hv, min_count, (int)geo.mk, geo.waves, d_fix, d_out, d_edits, room, c->d_cov_flags + 2, edit_base, edit_stride,
		                   c->d_cov_flags);
	});
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	rc = flags_end(c, "sdt_gpu_correct_reads", max_read_len, fl);
	if (n_edits) *n_edits = fl[2];
	if (rc != SDT_OK) return rc;
	if (d_edits && fl[2] > max_edits)
		return fail(SDT_EFULL, "sdt_gpu_correct_reads: %llu edits, edits[] holds %llu", fl[2], (unsigned long long)max_edits);
	return SDT_OK;
}

// a batch whose number of edits nobody knows: the list grows to what the kernel asked for and the batch runs once more
static int correct_device_grow(sdt_ctx *c, const uint32_t *d_words, uint64_t nwords, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                               uint32_t min_count, ReadFix *d_fix, DevBuf *eb, uint64_t edit_base, uint64_t edit_stride,
                               std::vector<uint64_t> *all)
{
	for (int attempt = 0; attempt < 2; attempt++) {
		int rc = eb->p ? SDT_OK : eb->get((nreads / 4 + 1024) * sizeof(unsigned long long), "edit list");
		if (rc != SDT_OK) return rc;
		const uint64_t room = eb->cap / sizeof(unsigned long long);
		uint64_t got = 0;
		rc = correct_device(c, d_words, nwords, d_offs, nreads, max_read_len, min_count, d_fix, nullptr, (unsigned long long *)eb->p, room, edit_base,
		                    edit_stride, &got);
		if (rc == SDT_EFULL && got > room && attempt == 0) {
			rc = eb->get(got * sizeof(unsigned long long), "edit list");
			if (rc != SDT_OK) return rc;
			continue;
		}
		if (rc != SDT_OK) return rc;
		const size_t at = all->size();
		all->resize(at + got);
		if (got) HIPCHK(hipMemcpy(all->data() + at, eb->p, got * sizeof(uint64_t), hipMemcpyDeviceToHost));
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
	SDT_ENTER(c);
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
	StreamCheck in;
	StripGeometry geo;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc == SDT_OK) rc = strip_plan(c, nreads, in.longest, &geo);      // (the whole call is refused before a piece's records are written)
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	// the edits of a piece name its reads from its first read's index in the batch
	std::vector<uint64_t> all;
	DevBuf d_r, eb;
	rc = for_each_piece(c, packed_words, offsets, nreads, 1, "correction staging", [&](const StagedPiece &p) -> int {
		int rc = d_r.reserve(p.nr * sizeof(ReadFix), "correction staging");
		if (rc == SDT_OK) rc = correct_device_grow(c, p.d_words, p.nwords, p.d_offs, p.nr, p.maxlen, min_count, (ReadFix *)d_r.p, &eb, p.r0, 1, &all);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(fix + p.r0, d_r.p, p.nr * sizeof(ReadFix), hipMemcpyDeviceToHost));
		return SDT_OK;
	});
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
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_edits) *n_edits = 0;
	int rc = search_ready(c, "sdt_gpu_correct_kept_reads");
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "fix", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	for (const auto &kb : c->kept) {
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (kb.nreads && last >> 46)
			return fail(SDT_ELIMIT, "a kept read has ordinal %llu: an edit holds 46 bits of it", (unsigned long long)last);
	}
	if (total == 0)
		return SDT_OK;
	if (!fix)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	DevBuf eb;
	std::vector<uint64_t> all;
	rc = for_each_kept_batch<ReadFix>(c, fix, most, "correction records", [&](const sdt_ctx::KeptBatch &kb, ReadFix *d_r) {
		return correct_device_grow(c, kb.d_words, kb.nwords, kb.d_offs, kb.nreads, kb.maxlen, min_count, d_r, &eb, kb.ord_base, kb.ord_stride, &all);
	});
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
	SDT_ENTER(c);
	int rc = kept_ready(c);
	if (rc != SDT_OK) return rc;
	if (i >= c->kept.size())
		return fail(SDT_EINVAL, "kept batch %llu of %zu", (unsigned long long)i, c->kept.size());
	rc = kept_drained(c, "sdt_gpu_fetch_kept_batch", false);
	if (rc != SDT_OK) return rc;
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
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (the uploads) and the offsets of a fixed-length batch, made on the device
	HIPCHK(hipStreamSynchronize(c->stream));
	if (words) HIPCHK(hipMemcpy(words, kb.d_words, kb.nwords * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (offsets) HIPCHK(hipMemcpy(offsets, kb.d_offs, (kb.nreads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return SDT_OK;
}

} // extern "C"
