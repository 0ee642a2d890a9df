// sdt_dedup.hip -- exact copies of a read or of a read pair dropped before pass 1 (the rule: include/sdt_gpu.h) = k_read_fp and rounds
// of k_dedup_insert + k_dedup_resolve + k_dedup_finish (sdt_dedup_kernels.cuh).  Needs no counted table: the dense forms need the
// context for its stream only, the kept form for the reads kept in HBM.  Nothing here writes the table or the kept reads.  The table
// size, the round cap, the check of the pair ranges and the cut of the units into stretches are sdt_read_plan.h's; staging checks and
// the kept batches are sdt_readstage.hpp's.
#include "sdt_readstage.hpp"
#include "sdt_dedup_kernels.cuh"

// (SDT_DEDUP_FP_BITS = 1 .. 64: test hook -- only the low bits of every unit fingerprint are kept, so that small inputs collide and
// go through later rounds)
static uint64_t fp_mask(void)
{
	const int b = sdt_knob_int(sdt_test_env("SDT_DEDUP_FP_BITS"), 64);
	return b >= 1 && b < 64 ? (1ULL << b) - 1 : ~0ULL;
}

static int launch_read_fp(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, uint64_t *d_fp, DedupEnt *d_ent,
                          uint64_t ord_base, uint64_t ord_stride)
{
	hipLaunchKernelGGL(k_read_fp, dim3(wave_grid(c, nreads)), dim3(TPB), 0, c->stream, d_words, d_offs, nreads, d_fp, d_ent, ord_base, ord_stride);
	HIPCHK(hipGetLastError());
	return SDT_OK;
}

// what the rounds hold on the device beside the reads: the table and two counters
struct DedupState {
	DevBuf tab, ctr;               // ctr[0]: units a round left unresolved, ctr[1]: reads kept
	uint64_t slots = 0;
	int reserve(uint64_t units)
	{
		slots = dedup_table_slots(units);
		const int rc = tab.get(slots * sizeof(DedupSlot), "duplicate table");
		return rc == SDT_OK ? ctr.get(2 * sizeof(unsigned long long), "duplicate counters") : rc;
	}
};

// The rounds over units whose fingerprints per read are in place, and the wait for them.  Records go to d_dup, indexed like the reads.
// SDT_ELIMIT past the round cap: d_dup and d_keep then hold records of resolved units only.
template <class Reads>
static int dedup_rounds(sdt_ctx *c, const char *what, DedupState &st, const Reads &reads, const Units &U, uint32_t flags, ReadDup *d_dup,
                        uint8_t *d_keep, uint64_t *n_kept)
{
	unsigned long long *ctr = (unsigned long long *)st.ctr.p;
	DedupRound R = {(DedupSlot *)st.tab.p, st.slots - 1, 0, fp_mask(), flags, 1};
	HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), c->stream));
	unsigned long long left[2] = {U.n, 0};
	const int lanes = scan_grid(c, U.n), waves = wave_grid(c, U.n);
	for (int round = 0; round < DEDUP_MAX_ROUNDS && left[0]; round++) {
		R.salt = mix64(0x9E3779B97F4A7C15ULL * (uint64_t)(round + 1));
		R.first = round == 0;
		HIPCHK(hipMemsetAsync(st.tab.p, 0, st.slots * sizeof(DedupSlot), c->stream));
		if (round) HIPCHK(hipMemsetAsync(ctr, 0, sizeof(unsigned long long), c->stream));
		hipLaunchKernelGGL(k_dedup_insert<Reads>, dim3(lanes), dim3(TPB), 0, c->stream, reads, U, R, d_dup);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_dedup_resolve<Reads>, dim3(waves), dim3(TPB), 0, c->stream, reads, U, R, d_dup, ctr);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_dedup_finish<Reads>, dim3(lanes), dim3(TPB), 0, c->stream, reads, U, R, d_dup, d_keep, ctr + 1);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(left, ctr, sizeof left, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	if (left[0])
		return fail(SDT_ELIMIT, "%s: %llu units are unresolved after %d rounds of fingerprint collisions", what, left[0], DEDUP_MAX_ROUNDS);
	if (n_kept) *n_kept = left[1];
	return SDT_OK;
}

// one dense device-resident batch, checked arguments
static int dedup_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, int paired, uint32_t flags,
                        ReadDup *d_dup, uint8_t *d_keep, uint64_t *n_kept)
{
	const uint64_t units = paired ? nreads / 2 : nreads;
	DedupState st;
	DevBuf d_fp;
	int rc = d_fp.get(nreads * sizeof(uint64_t), "read fingerprints");
	if (rc == SDT_OK) rc = st.reserve(units);
	if (rc != SDT_OK) return rc;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	rc = launch_read_fp(c, d_words, d_offs, nreads, (uint64_t *)d_fp.p, nullptr, 0, 0);
	if (rc == SDT_OK) {
		const DenseReads reads = {d_words, d_offs, (const uint64_t *)d_fp.p, nreads};
		const Units U = {nullptr, 0, UnitStretch{0, 0, paired ? 2ULL : 1ULL}, units};
		rc = dedup_rounds(c, "sdt_gpu_dedup_reads", st, reads, U, flags, d_dup, d_keep, n_kept);
	}
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;                                  // (reads, not k-mers: sdt_gpu_kernel_time reports them as they are)
	}
	(void)hipStreamSynchronize(c->stream);                   // (the scratch arrays go when this returns)
	return rc;
}

static int params_ok(const sdt_dedup_params *p, uint64_t nreads, int paired)
{
	if (!p)
		return fail(SDT_EINVAL, "NULL argument");
	if (p->flags & ~(uint32_t)SDT_DEDUP_MATE_SWAP)
		return fail(SDT_EINVAL, "sdt_dedup_params.flags = 0x%x: unknown bits", p->flags);
	if (paired && (nreads & 1))
		return fail(SDT_EINVAL, "paired reads: reads 2t and 2t + 1 are mates, %llu reads is an odd number", (unsigned long long)nreads);
	return SDT_OK;
}

extern "C" {

int sdt_gpu_dedup_reads_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired,
                               const sdt_dedup_params *params, void *d_dup, void *d_keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets || !d_dup)
		return fail(SDT_EINVAL, "NULL argument");
	const int rc = params_ok(params, nreads, paired);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return dedup_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, paired, params->flags, (ReadDup *)d_dup,
	                    (uint8_t *)d_keep, n_kept);
}

int sdt_gpu_dedup_reads(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired,
                        const sdt_dedup_params *params, sdt_read_dup *dup, uint8_t *keep, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_kept) *n_kept = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets || !dup)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = params_ok(params, nreads, paired);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	// copies of a read sit anywhere in the batch: the whole stream is staged at once
	DevBuf d_w, d_o, d_r, d_k;
	rc = d_w.get(in.need_words * sizeof(uint32_t), "duplicate staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "duplicate staging");
	if (rc == SDT_OK) rc = d_r.get(nreads * sizeof(ReadDup), "duplicate staging");
	if (rc == SDT_OK) rc = d_k.get(nreads, "duplicate staging");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in.need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	uint64_t kept = 0;
	rc = dedup_device(c, (const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nreads, paired, params->flags, (ReadDup *)d_r.p, (uint8_t *)d_k.p, &kept);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpy(dup, d_r.p, nreads * sizeof(ReadDup), hipMemcpyDeviceToHost));
	if (keep) HIPCHK(hipMemcpy(keep, d_k.p, nreads, hipMemcpyDeviceToHost));
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

int sdt_gpu_dedup_kept_reads(sdt_ctx *c, const sdt_dedup_params *params, const uint64_t *pair_ranges, uint64_t n_ranges, sdt_read_dup *dup,
                             uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_kept) *n_kept = 0;
	int rc = params_ok(params, 0, 0);
	if (rc == SDT_OK) rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_dedup_kept_reads", false);
	if (rc != SDT_OK) return rc;
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "dup", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0)
		return SDT_OK;
	if (!dup)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// mates and copies sit in different kept batches: the entries and the records of ALL ordinals on the device at once
	// (sdt_readstage.hpp: KeptUnits)
	KeptUnits ku(pair_ranges, n_ranges, nord);
	DedupState st;
	DevBuf d_ent, d_dup;
	rc = d_ent.get(nord * sizeof(DedupEnt), "duplicate entries");
	if (rc == SDT_OK) rc = d_dup.get(nord * sizeof(ReadDup), "duplicate records");
	if (rc == SDT_OK) rc = ku.d_segs.get(ku.bytes(), "duplicate units");
	if (rc == SDT_OK) rc = st.reserve(ku.units);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_dup.p, 0xFF, nord * sizeof(ReadDup), c->stream));
	rc = ku.upload(c);
	if (rc != SDT_OK) return rc;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	rc = kept_entries(c, nord, d_ent);                       // (its memset of the entries is timed with the kernels)
	uint64_t kept = 0;
	if (rc == SDT_OK) {
		const KeptReads reads = {(const DedupEnt *)d_ent.p, nord};
		rc = dedup_rounds(c, "sdt_gpu_dedup_kept_reads", st, reads, ku.on_device(), params->flags, (ReadDup *)d_dup.p, nullptr, &kept);
	}
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = total;
	}
	HIPCHK(hipStreamSynchronize(c->stream));             // (segs may go)
	if (rc != SDT_OK) return rc;
	rc = fetch_present<ReadDup>(dup, d_dup, nord, DUP_ABSENT);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	if (n_kept) *n_kept = kept;
	return SDT_OK;
}

} // extern "C"
