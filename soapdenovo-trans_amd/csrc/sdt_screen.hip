// sdt_screen.hip -- reads screened against reference sequences (rRNA, PhiX, a mitochondrial genome, vectors) before pass 1 (the rule:
// include/sdt_gpu.h) = k_screen_build, k_screen_lookup and k_screen_reads (sdt_screen_kernels.cuh).  Needs no counted table: the set
// is a hash table of its own that the context keeps from screen_load to screen_unload; the dense forms need the context for its stream
// and the set only, the kept form also for the reads kept in HBM.  Nothing here writes the node table or the kept reads.  What is
// refused, the size of the table and the unit verdicts of the kept form are sdt_read_plan.h's; staging in pieces and the kept batches
// are sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len and verdict sit where sdt_read_trim has
// them.
#include "sdt_compact.hpp"
#include "sdt_screen_kernels.cuh"

static_assert(sizeof(sdt_read_screen) == sizeof(ReadScreen) && sizeof(sdt_screen_params) == sizeof(ScreenParams), "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_screen>(), "sdt_gpu_compact_trimmed takes sdt_read_screen records through a pointer cast");
static_assert(SDT_SCREEN_KEEP_MATCHED == SCREEN_KEEP_MATCHED && SDT_SCREEN_NO_REF == SCREEN_NO_REF, "include/sdt_gpu.h and sdt_read_plan.h agree");

// every refusal of the parameters, before any launch
static int args_ok(const sdt_screen_params *p, uint64_t nreads, int paired)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_screen_params is NULL");
	switch (check_screen_params(ScreenParams{p->min_hits, p->min_hit_pct, p->flags, p->reserved})) {
	case SCREEN_MIN_HIT_PCT: return fail(SDT_EINVAL, "sdt_screen_params.min_hit_pct = %u: a percentage, 100 at most", p->min_hit_pct);
	case SCREEN_FLAGS: return fail(SDT_EINVAL, "sdt_screen_params.flags = 0x%x: SDT_SCREEN_KEEP_MATCHED is the only flag", p->flags);
	case SCREEN_RESERVED: return fail(SDT_EINVAL, "sdt_screen_params.reserved = %u: it must be 0", p->reserved);
	default: break;
	}
	if (paired && (nreads & 1))
		return fail(SDT_EINVAL, "paired reads: reads 2t and 2t + 1 are mates, %llu reads is an odd number", (unsigned long long)nreads);
	return SDT_OK;
}

static int set_ready(const sdt_ctx *c, const char *what)
{
	if (!c->screen.tab)
		return fail(SDT_ESTATE, "%s: no reference set is loaded: call sdt_gpu_screen_load first", what);
	return SDT_OK;
}

static ScreenTable table_of_set(const sdt_ctx *c) { return ScreenTable{(ScreenSlot *)c->screen.tab, c->screen.slots - 1, c->screen.k}; }

// one dense device-resident batch, checked arguments: the kernel and the wait for its counter (ctr: one 64-bit word on the device)
static int screen_device(sdt_ctx *c, const DevBuf &ctr, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, int paired,
                         const ScreenParams &prm, ReadScreen *d_out, uint8_t *d_keep, uint64_t *n_kept)
{
	const DenseReads reads = {d_words, d_offs, nullptr, nreads};
	const uint32_t stride = paired ? 2u : 1u;
	const uint64_t units = nreads / stride;
	return launch_counted(c, ctr, units, nreads, n_kept, [&](int grid, unsigned long long *d_ctr) {
		hipLaunchKernelGGL(k_screen_reads, dim3(grid), dim3(TPB), 0, c->stream, reads, units, stride, table_of_set(c), prm, d_out, d_keep, d_ctr);
	});
}

static ScreenParams params_of(const sdt_screen_params *p) { return ScreenParams{p->min_hits, p->min_hit_pct, p->flags, p->reserved}; }

extern "C" {

int sdt_gpu_screen_load(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nseqs,
                        const uint32_t *ref_of_seq, uint32_t n_refs, uint32_t k, uint64_t *n_kmers)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (k < SCREEN_MIN_K || k > SCREEN_MAX_K)
		return fail(SDT_EINVAL, "sdt_gpu_screen_load: k = %u: the screen takes k-mers of %u to %u bases", k, SCREEN_MIN_K, SCREEN_MAX_K);
	if (n_refs == 0)
		return fail(SDT_EINVAL, "sdt_gpu_screen_load: n_refs = 0: a set has a reference at least");
	if (nseqs && (!packed_words || !offsets || !ref_of_seq))
		return fail(SDT_EINVAL, "NULL argument");
	for (uint64_t i = 0; i < nseqs; i++)
		if (ref_of_seq[i] >= n_refs)
			return fail(SDT_EINVAL, "sdt_gpu_screen_load: ref_of_seq[%llu] = %u: there are %u references", (unsigned long long)i, ref_of_seq[i], n_refs);
	StreamCheck in;
	int rc = stream_args_ok(offsets, nseqs, nwords, &in);
	if (rc != SDT_OK) return rc;
	const uint64_t positions = screen_positions(offsets, nseqs, k);
	if (positions == 0)
		return fail(SDT_EINVAL, "sdt_gpu_screen_load: no sequence has k = %u bases: the set would hold no k-mer", k);
	uint64_t slots = screen_table_slots(positions);
	if (const char *v = sdt_test_env("SDT_SCREEN_SLOTS")) {
		const uint64_t forced = strtoull(v, nullptr, 10);
		if (!screen_forced_slots_ok(forced, positions))
			return fail(SDT_EINVAL, "SDT_SCREEN_SLOTS = %s: a power of two above the %llu k-mer positions of the set", v, (unsigned long long)positions);
		slots = forced;
	}
	SDT_ENTER(c);
	// the staged sequences go when this returns; the table stays, and replaces the previous one only once it is complete
	DevBuf d_w, d_o, d_r, d_n, tab;
	rc = d_w.get(in.need_words * sizeof(uint32_t), "screen staging");
	if (rc == SDT_OK) rc = d_o.get((nseqs + 1) * sizeof(uint64_t), "screen staging");
	if (rc == SDT_OK) rc = d_r.get(nseqs * sizeof(uint32_t), "screen staging");
	if (rc == SDT_OK) rc = d_n.get(sizeof(unsigned long long), "screen counter");
	if (rc == SDT_OK) rc = tab.get(slots * sizeof(ScreenSlot), "screen table");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in.need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nseqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_r.p, ref_of_seq, nseqs * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(tab.p, 0xFF, slots * sizeof(ScreenSlot), c->stream));
	const ScreenTable T = {(ScreenSlot *)tab.p, slots - 1, k};
	hipLaunchKernelGGL(k_screen_build, dim3(scan_grid(c, offsets[nseqs] - offsets[0])), dim3(TPB), 0, c->stream, (const uint32_t *)d_w.p,
	                   (const uint64_t *)d_o.p, nseqs, (const uint32_t *)d_r.p, T, (unsigned long long *)d_n.p);
	HIPCHK(hipGetLastError());
	unsigned long long distinct = 0;
	HIPCHK(hipMemcpyAsync(&distinct, d_n.p, sizeof distinct, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (c->screen.tab) (void)hipFree(c->screen.tab);
	c->screen.tab = tab.p;
	tab.p = nullptr;                                         // (the context's from here on)
	c->screen.slots = slots;
	c->screen.n_kmers = distinct;
	c->screen.k = k;
	c->screen.n_refs = n_refs;
	if (n_kmers) *n_kmers = distinct;
	return SDT_OK;
}

int sdt_gpu_screen_unload(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (!c->screen.tab)
		return SDT_OK;
	HIPCHK(hipStreamSynchronize(c->stream));
	(void)hipFree(c->screen.tab);
	c->screen = sdt_ctx::ScreenSet();
	return SDT_OK;
}

int sdt_gpu_screen_info(const sdt_ctx *c, uint64_t info[4])
{
	if (!c || !info)
		return fail(SDT_EINVAL, "NULL argument");
	info[0] = c->screen.k;
	info[1] = c->screen.n_refs;
	info[2] = c->screen.n_kmers;
	info[3] = c->screen.slots;
	return SDT_OK;
}

int sdt_gpu_screen_lookup(sdt_ctx *c, const uint64_t *keys, uint64_t n, uint32_t *refs)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!keys || !refs)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = set_ready(c, "sdt_gpu_screen_lookup");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const uint64_t piece = chunk_items(PROFILE_CHUNK_READS);
	DevBuf d_k, d_r;
	rc = d_k.get((n < piece ? n : piece) * sizeof(uint64_t), "screen keys");
	if (rc == SDT_OK) rc = d_r.get((n < piece ? n : piece) * sizeof(uint32_t), "screen keys");
	if (rc != SDT_OK) return rc;
	for (uint64_t i0 = 0; i0 < n; i0 += piece) {
		const uint64_t m = n - i0 < piece ? n - i0 : piece;
		HIPCHK(hipMemcpyAsync(d_k.p, keys + i0, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_screen_lookup, dim3(scan_grid(c, m)), dim3(TPB), 0, c->stream, (const uint64_t *)d_k.p, m, table_of_set(c), (uint32_t *)d_r.p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(refs + i0, d_r.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	return SDT_OK;
}

int sdt_gpu_screen_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired,
                                const sdt_screen_params *params, void *d_out, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, nreads, paired);
	if (rc == SDT_OK) rc = set_ready(c, "sdt_gpu_screen_reads_device");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "screen counter");
	if (rc != SDT_OK) return rc;
	return screen_device(c, ctr, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, paired, params_of(params), (ReadScreen *)d_out,
	                     (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_screen_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired,
                         const sdt_screen_params *params, sdt_read_screen *out, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, nreads, paired);
	if (rc == SDT_OK) rc = set_ready(c, "sdt_gpu_screen_reads");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "screen counter");
	if (rc != SDT_OK) return rc;
	// (the mates of a pair stay in one piece)
	return staged_records<ReadScreen>(c, packed_words, offsets, nreads, paired ? 2 : 1, "screen staging", out, keep, n_kept,
	                                  [&](const StagedPiece &p, ReadScreen *d_r, uint8_t *d_k, uint64_t *kept) {
		return screen_device(c, ctr, p.d_words, p.d_offs, p.nr, paired, params_of(params), d_r, d_k, kept);
	});
}

int sdt_gpu_screen_kept_reads(sdt_ctx *c, const sdt_screen_params *params, const uint64_t *pair_ranges, uint64_t n_ranges, sdt_read_screen *out,
                              uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = args_ok(params, 0, 0);
	if (rc == SDT_OK) rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = set_ready(c, "sdt_gpu_screen_kept_reads");
	if (rc == SDT_OK) rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_screen_kept_reads", false);
	if (rc != SDT_OK) return rc;
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "out", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!out)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// batch by batch: what every read has on its own, dense on the device, scattered to the ordinals of a copy on the host; mates sit
	// in different batches, so the unit verdicts are taken there (sdt_read_plan.h) before anything of out[] is written
	DevBuf ctr;
	rc = ctr.get(sizeof(unsigned long long), "screen counter");
	if (rc != SDT_OK) return rc;
	ScreenParams per_read = params_of(params);
	per_read.flags |= SCREEN_PER_READ;
	std::vector<ReadScreen> rec(nord);
	std::vector<uint8_t> present(nord, 0);
	rc = for_each_kept_batch<ReadScreen>(c, rec.data(), most, "screen records", [&](const sdt_ctx::KeptBatch &kb, ReadScreen *d_r) {
		for (uint64_t i = 0; i < kb.nreads; i++) present[kb.ord_base + i * kb.ord_stride] = 1;
		return screen_device(c, ctr, kb.d_words, kb.d_offs, kb.nreads, 0, per_read, d_r, nullptr, nullptr);
	});
	if (rc != SDT_OK) return rc;
	const uint64_t kept = screen_unit_verdicts(rec.data(), present.data(), nord, pair_ranges, n_ranges, params_of(params));
	for (uint64_t o = 0; o < nord; o++)
		if (present[o]) memcpy(out + o, &rec[o], sizeof(ReadScreen));
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
