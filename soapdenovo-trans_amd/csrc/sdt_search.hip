// sdt_search.hip -- read-only questions to the counted node table: search_kmerset (newhash.c:239-283) for a batch of k-mers =
// k_search_kmers, and the k-mer coverage of reads (chopKmer4read's k-mers, prlHashReads.c:164-310, looked up instead of inserted) =
// k_profile_reads.  Nothing here writes the table.
#include "sdt_ctx.hpp"
#include "sdt_search_kernels.cuh"

// nodes with a count past 65 535 that the small hash takes (4 words per node: 8 MiB at most); more than that and aux itself is read
static const uint64_t HI_HASH_MAX = 1ULL << 18;
// queries / reads of a host batch that are on the device at a time
static const uint64_t SEARCH_CHUNK = 1ULL << 22;
// (PROFILE_CHUNK_READS / PROFILE_CHUNK_BASES: sdt_ctx.hpp -- sdt_correct.hip stages its reads the same way)
// (SDT_SEARCH_CHUNK: test hook -- pieces of that many queries / reads, so that small batches cross piece boundaries)
uint64_t chunk_items(uint64_t dflt)
{
	const char *v = sdt_test_env("SDT_SEARCH_CHUNK");
	return v && atoll(v) > 0 ? (uint64_t)atoll(v) : dflt;
}

// the state rules of include/sdt_gpu.h, one message each
int search_ready(sdt_ctx *c, const char *what)
{
	if (c->flags & SDT_FLAG_CONTIG_INDEX)
		return fail(SDT_ESTATE, "%s: a SDT_FLAG_CONTIG_INDEX context holds contig positions, not counts", what);
	if (c->comm.kind != 0)
		return fail(SDT_ESTATE, "%s: this context holds one shard of %d: it cannot tell an absent k-mer from another rank's", what, c->comm.nranks);
	if (c->paths_loaded)
		return fail(SDT_ESTATE, "%s: the counters were overwritten by path words (sdt_gpu_load_paths / sdt_gpu_import_paths)", what);
	if (!c->d_ent || !c->d_aux || c->slots == 0)
		return fail(SDT_ESTATE, "%s: the node table was released (sdt_gpu_release_table)", what);
	if (c->staged_head < c->staged.size() || c->sk.pending_kmers || c->kmers_since_sync || c->hard_since_sync)
		return fail(SDT_ESTATE, "%s: batches were pushed and not drained: call sdt_gpu_finish_count first", what);
	return SDT_OK;
}

int flags_reserve(sdt_ctx *c)
{
	if (!c->d_cov_flags) HIPCHK(hipMalloc((void **)&c->d_cov_flags, 3 * sizeof(unsigned long long)));
	return SDT_OK;
}

// where k_profile_reads finds the high half of a count: collected on the first profile after the table last changed
int hi_prepare(sdt_ctx *c, HiView *hv)
{
	if (c->hi_mode < 0) {
		HIPCHK(hipMemsetAsync(c->d_cov_flags + 1, 0, sizeof(unsigned long long), c->stream));
		const int g = scan_grid(c, c->slots);
		hipLaunchKernelGGL(k_hi_count, dim3(g), dim3(TPB), 0, c->stream, (const uint32_t *)c->d_aux, c->slots, c->d_cov_flags + 1);
		HIPCHK(hipGetLastError());
		unsigned long long n_hi = 0;
		HIPCHK(hipMemcpyAsync(&n_hi, c->d_cov_flags + 1, sizeof n_hi, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		// (SDT_PROFILE_AUX: test hook -- `aux` reads aux[slot] per look-up, `hash` builds the hash even when it would be empty)
		const char *force = sdt_test_env("SDT_PROFILE_AUX");
		const bool force_aux = force && !strcmp(force, "aux"), force_hash = force && !strcmp(force, "hash");
		if (force_aux || n_hi > HI_HASH_MAX) {
			c->hi_mode = HI_AUX;
		} else if (n_hi == 0 && !force_hash) {
			c->hi_mode = HI_NONE;
		} else {
			uint64_t hs = 1024;
			while (hs < 4 * n_hi) hs <<= 1;
			if (c->hi_slots < hs) {
				if (c->d_hi) HIPCHK(hipFree(c->d_hi));
				c->d_hi = nullptr;
				c->hi_slots = 0;
				HIPCHK(hipMalloc((void **)&c->d_hi, hs * sizeof(uint64_t)));
			}
			c->hi_slots = hs;
			HIPCHK(hipMemsetAsync(c->d_hi, 0, hs * sizeof(uint64_t), c->stream));
			hipLaunchKernelGGL(k_hi_fill, dim3(g), dim3(TPB), 0, c->stream, (const uint32_t *)c->d_aux, c->slots, c->d_hi, hs - 1);
			HIPCHK(hipGetLastError());
			c->hi_mode = HI_HASH;
		}
	}
	hv->mode = c->hi_mode;
	hv->tab = c->hi_mode == HI_HASH ? c->d_hi : nullptr;
	hv->mask = c->hi_mode == HI_HASH ? c->hi_slots - 1 : 0;
	return SDT_OK;
}

static int launch_search(sdt_ctx *c, const uint64_t *d_keys, uint64_t n, uint32_t *d_count, uint32_t *d_l, uint32_t *d_r, uint8_t *d_status)
{
	const int g = scan_grid(c, n);
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	if (c->nw == 1) hipLaunchKernelGGL(k_search_kmers<1>, dim3(g), dim3(TPB), 0, c->stream, d_keys, n, c->K, table_of<1>(c), d_count, d_l, d_r, d_status);
	else if (c->nw == 2) hipLaunchKernelGGL(k_search_kmers<2>, dim3(g), dim3(TPB), 0, c->stream, d_keys, n, c->K, table_of<2>(c), d_count, d_l, d_r, d_status);
	else hipLaunchKernelGGL(k_search_kmers<4>, dim3(g), dim3(TPB), 0, c->stream, d_keys, n, c->K, table_of<4>(c), d_count, d_l, d_r, d_status);
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = n;
	}
	return SDT_OK;
}

// enqueue k_profile_reads for one device-resident batch; d_cov_flags[0] counts the reads longer than max_read_len
static int launch_profile(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len,
                          uint32_t min_count, ReadCov *d_out, uint64_t out_base, uint64_t out_stride)
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
#define PROFILE_LAUNCH(NWV) hipLaunchKernelGGL(k_profile_reads<NWV>, dim3((unsigned)blocks), dim3(TPB), per_wave * waves, c->stream, d_words, d_offs, nreads, \
	c->K, table_of<NWV>(c), hv, min_count, (int)mk, waves, d_out, out_base, out_stride, c->d_cov_flags)
	if (c->nw == 1) PROFILE_LAUNCH(1);
	else if (c->nw == 2) PROFILE_LAUNCH(2);
	else PROFILE_LAUNCH(4);
#undef PROFILE_LAUNCH
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads * mk;                         // (an upper bound, as for the count kernels)
	}
	return SDT_OK;
}

extern "C" {

int sdt_gpu_search_kmers_device(sdt_ctx *c, const void *d_keys, uint64_t n, void *d_count, void *d_l_links, void *d_r_flags, void *d_status)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!d_keys)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_search_kmers");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipSetDevice(c->device));
	return launch_search(c, (const uint64_t *)d_keys, n, (uint32_t *)d_count, (uint32_t *)d_l_links, (uint32_t *)d_r_flags, (uint8_t *)d_status);
}

int sdt_gpu_search_kmers(sdt_ctx *c, const uint64_t *keys, uint64_t n, uint32_t *count, uint32_t *l_links, uint32_t *r_flags, uint8_t *status)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!keys)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_search_kmers");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipSetDevice(c->device));
	// in pieces through the arena: keys + 13 bytes of answers per query
	const uint64_t piece = chunk_items(SEARCH_CHUNK), m = n < piece ? n : piece;
	uint64_t *d_k = nullptr;
	uint32_t *d_c = nullptr, *d_l = nullptr, *d_r = nullptr;
	uint8_t *d_s = nullptr;
	int ret = SDT_OK;
#define SRCH_CHK(expr)                                                                                 \
	do {                                                                                               \
		hipError_t e5_ = (expr);                                                                       \
		if (e5_ != hipSuccess) {                                                                       \
			ret = fail(e5_ == hipErrorOutOfMemory ? SDT_ENOMEM : SDT_EHIP, "%s: %s", #expr, hipGetErrorString(e5_)); \
			goto done;                                                                                 \
		}                                                                                              \
	} while (0)
	SRCH_CHK(hipMalloc((void **)&d_k, m * c->nw * sizeof(uint64_t)));
	if (count) SRCH_CHK(hipMalloc((void **)&d_c, m * sizeof(uint32_t)));
	if (l_links) SRCH_CHK(hipMalloc((void **)&d_l, m * sizeof(uint32_t)));
	if (r_flags) SRCH_CHK(hipMalloc((void **)&d_r, m * sizeof(uint32_t)));
	if (status) SRCH_CHK(hipMalloc((void **)&d_s, m));
	for (uint64_t i0 = 0; i0 < n; i0 += m) {
		const uint64_t k = n - i0 < m ? n - i0 : m;
		SRCH_CHK(hipMemcpyAsync(d_k, keys + i0 * c->nw, k * c->nw * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		ret = launch_search(c, d_k, k, d_c, d_l, d_r, d_s);
		if (ret != SDT_OK) goto done;
		if (count) SRCH_CHK(hipMemcpyAsync(count + i0, d_c, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (l_links) SRCH_CHK(hipMemcpyAsync(l_links + i0, d_l, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (r_flags) SRCH_CHK(hipMemcpyAsync(r_flags + i0, d_r, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (status) SRCH_CHK(hipMemcpyAsync(status + i0, d_s, k, hipMemcpyDeviceToHost, c->stream));
		SRCH_CHK(hipStreamSynchronize(c->stream));
	}
done:
	if (d_k) (void)hipFree(d_k);
	if (d_c) (void)hipFree(d_c);
	if (d_l) (void)hipFree(d_l);
	if (d_r) (void)hipFree(d_r);
	if (d_s) (void)hipFree(d_s);
	return ret;
}

int sdt_gpu_profile_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, uint64_t max_read_len,
                                 uint32_t min_count, void *d_out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_profile_reads");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipSetDevice(c->device));
	rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	rc = launch_profile(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, max_read_len, min_count, (ReadCov *)d_out, 0, 1);
	if (rc != SDT_OK) return rc;
	unsigned long long too_long = 0;
	HIPCHK(hipMemcpyAsync(&too_long, c->d_cov_flags, sizeof too_long, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (too_long)
		return fail(SDT_EINVAL, "sdt_gpu_profile_reads: %llu reads are longer than max_read_len = %llu; their records have kmers = 0xFFFFFFFF",
		            too_long, (unsigned long long)max_read_len);
	return SDT_OK;
}

int sdt_gpu_profile_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                          uint32_t min_count, sdt_read_cov *out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = search_ready(c, "sdt_gpu_profile_reads");
	if (rc != SDT_OK) return rc;
	for (uint64_t i = 0; i < nreads; i++)
		if (offsets[i + 1] < offsets[i])
			return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)i);
	if (((offsets[nreads] + 15) >> 4) + TAIL_PAD > nwords)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)(((offsets[nreads] + 15) >> 4) + TAIL_PAD), TAIL_PAD);
	HIPCHK(hipSetDevice(c->device));
	// in pieces through the arena: a run of reads, the words that hold them (offsets rebased to the piece's first word) and their records
	const uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	std::vector<uint64_t> rel;
	uint32_t *d_w = nullptr;
	uint64_t *d_o = nullptr;
	ReadCov *d_r = nullptr;
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
			if (e == hipSuccess) e = hipMalloc((void **)&d_r, cap_r * sizeof(ReadCov));
			if (e != hipSuccess) { rc = fail(SDT_ENOMEM, "profile staging: %s", hipGetErrorString(e)); break; }
		}
		hipError_t e = hipMemcpyAsync(d_w, packed_words + w0, nw * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(d_o, rel.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "profile staging: %s", hipGetErrorString(e)); break; }
		rc = sdt_gpu_profile_reads_device(c, d_w, d_o, nr, maxlen, min_count, d_r);          // (waits for the kernel: rel may be refilled)
		if (rc != SDT_OK) break;
		e = hipMemcpy(out + r0, d_r, nr * sizeof(ReadCov), hipMemcpyDeviceToHost);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "profile records: %s", hipGetErrorString(e)); break; }
		r0 = r1;
	}
	if (d_w) (void)hipFree(d_w);
	if (d_o) (void)hipFree(d_o);
	if (d_r) (void)hipFree(d_r);
	return rc;
}

int sdt_gpu_profile_kept_reads(sdt_ctx *c, uint32_t min_count, sdt_read_cov *out, uint64_t out_capacity, uint64_t *nreads)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	int rc = search_ready(c, "sdt_gpu_profile_kept_reads");
	if (rc != SDT_OK) return rc;
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	uint64_t total = 0, most = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (last >= out_capacity)
			return fail(SDT_EFULL, "a kept read has ordinal %llu, out[] holds %llu records", (unsigned long long)last, (unsigned long long)out_capacity);
		total += kb.nreads;
		if (kb.nreads > most) most = kb.nreads;
	}
	if (total == 0)
		return SDT_OK;
	if (!out)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipSetDevice(c->device));
	rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// batch by batch: dense records on the device, scattered to their ordinals on the host (nothing else of out[] is touched)
	ReadCov *d_r = nullptr;
	HIPCHK(hipMalloc((void **)&d_r, most * sizeof(ReadCov)));
	std::vector<ReadCov> tmp(most);
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = sdt_gpu_profile_reads_device(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, min_count, d_r);
		if (rc != SDT_OK) break;
		const hipError_t e = hipMemcpy(tmp.data(), d_r, kb.nreads * sizeof(ReadCov), hipMemcpyDeviceToHost);
		if (e != hipSuccess) { rc = fail(SDT_EHIP, "profile records: %s", hipGetErrorString(e)); break; }
		for (uint64_t i = 0; i < kb.nreads; i++)
			memcpy(out + (kb.ord_base + i * kb.ord_stride), &tmp[i], sizeof(ReadCov));
	}
	(void)hipFree(d_r);
	if (rc == SDT_OK && nreads) *nreads = total;
	return rc;
}

} // extern "C"
