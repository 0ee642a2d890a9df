// sdt_search.hip -- read-only questions to the counted node table: search_kmerset (newhash.c:239-283) for a batch of k-mers =
// k_search_kmers, and the k-mer coverage of reads (chopKmer4read's k-mers, prlHashReads.c:164-310, looked up instead of inserted) =
// k_profile_reads.  Nothing here writes the table.
#include "sdt_readstage.hpp"

// nodes with a count past 65 535 that the small hash takes (4 words per node: 8 MiB at most); more than that and aux itself is read
static const uint64_t HI_HASH_MAX = 1ULL << 18;
// queries / reads of a host batch that are on the device at a time
static const uint64_t SEARCH_CHUNK = 1ULL << 22;
// (PROFILE_CHUNK_READS / PROFILE_CHUNK_BASES: sdt_readstage.hpp -- every read stage cuts its host batches the same way)
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
	return kept_drained(c, what, true);
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
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_search_kmers<NW>, dim3(g), dim3(TPB), 0, c->stream, d_keys, n, c->K, table_of<NW>(c), d_count, d_l, d_r, d_status);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = n;
	}
	return SDT_OK;
}

// one device-resident batch, checked arguments: k_profile_reads and the wait for its counter
static int profile_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t max_read_len, uint32_t min_count,
                          ReadCov *d_out)
{
	int rc = flags_begin(c);
	if (rc != SDT_OK) return rc;
	rc = launch_strip(c, nreads, max_read_len, [&](auto nw, const StripGeometry &geo, const HiView &hv) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_profile_reads<NW>, dim3(geo.blocks), dim3(TPB), geo.lds_bytes, c->stream, d_words, d_offs, nreads, c->K, table_of<NW>(c),
		                   hv, min_count, (int)geo.mk, geo.waves, d_out, (uint64_t)0, (uint64_t)1, c->d_cov_flags);
	});
	if (rc != SDT_OK) return rc;
	unsigned long long fl[3] = {0, 0, 0};
	return flags_end(c, "sdt_gpu_profile_reads", max_read_len, fl);
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
	SDT_ENTER(c);
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
	SDT_ENTER(c);
	// in pieces through the arena: keys + 13 bytes of answers per query
	const uint64_t piece = chunk_items(SEARCH_CHUNK), m = n < piece ? n : piece;
	DevBuf d_k, d_c, d_l, d_r, d_s;
	rc = d_k.get(m * c->nw * sizeof(uint64_t), "search staging");
	if (rc == SDT_OK && count) rc = d_c.get(m * sizeof(uint32_t), "search staging");
	if (rc == SDT_OK && l_links) rc = d_l.get(m * sizeof(uint32_t), "search staging");
	if (rc == SDT_OK && r_flags) rc = d_r.get(m * sizeof(uint32_t), "search staging");
	if (rc == SDT_OK && status) rc = d_s.get(m, "search staging");
	if (rc != SDT_OK) return rc;
	for (uint64_t i0 = 0; i0 < n; i0 += m) {
		const uint64_t k = n - i0 < m ? n - i0 : m;
		HIPCHK(hipMemcpyAsync(d_k.p, keys + i0 * c->nw, k * c->nw * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		rc = launch_search(c, (const uint64_t *)d_k.p, k, (uint32_t *)d_c.p, (uint32_t *)d_l.p, (uint32_t *)d_r.p, (uint8_t *)d_s.p);
		if (rc != SDT_OK) return rc;
		if (count) HIPCHK(hipMemcpyAsync(count + i0, d_c.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (l_links) HIPCHK(hipMemcpyAsync(l_links + i0, d_l.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (r_flags) HIPCHK(hipMemcpyAsync(r_flags + i0, d_r.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (status) HIPCHK(hipMemcpyAsync(status + i0, d_s.p, k, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	return SDT_OK;
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
	SDT_ENTER(c);
	return profile_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, max_read_len, min_count, (ReadCov *)d_out);
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
	StreamCheck in;
	StripGeometry geo;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc == SDT_OK) rc = strip_plan(c, nreads, in.longest, &geo);      // (the whole call is refused before a piece's records are written)
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf d_r;
	return for_each_piece(c, packed_words, offsets, nreads, 1, "profile staging", [&](const StagedPiece &p) -> int {
		int rc = d_r.reserve(p.nr * sizeof(ReadCov), "profile staging");
		if (rc == SDT_OK) rc = profile_device(c, p.d_words, p.d_offs, p.nr, p.maxlen, min_count, (ReadCov *)d_r.p);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy(out + p.r0, d_r.p, p.nr * sizeof(ReadCov), hipMemcpyDeviceToHost));
		return SDT_OK;
	});
}

int sdt_gpu_profile_kept_reads(sdt_ctx *c, uint32_t min_count, sdt_read_cov *out, uint64_t out_capacity, uint64_t *nreads)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads) *nreads = 0;
	int rc = search_ready(c, "sdt_gpu_profile_kept_reads");
	if (rc != SDT_OK) return rc;
	uint64_t total, most, npick;
	rc = kept_span(c, out_capacity, "out", &total, &most, &npick);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!out)
		return fail(SDT_EINVAL, "NULL argument");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	rc = for_each_kept_batch<ReadCov>(c, out, most, "profile records", [&](const sdt_ctx::KeptBatch &kb, ReadCov *d_r) {
		return profile_device(c, kb.d_words, kb.d_offs, kb.nreads, kb.maxlen, min_count, d_r);
	});
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	return SDT_OK;
}

} // extern "C"
