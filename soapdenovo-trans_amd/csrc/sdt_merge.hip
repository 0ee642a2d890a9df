// sdt_merge.hip -- the two mates of an overlapping pair merged into one fragment read, by the overlap records that
// sdt_gpu_overlap_pairs wrote (the rule: include/sdt_gpu.h) = k_merge_decide, three scans, k_merge_pairs into a scratch stream and
// k_compact_words out of it; and the quality bytes of a stream through one compaction = one scan and k_compact_quals
// (sdt_merge_kernels.cuh).  Needs no counted table: the dense forms need the context for its stream only, the kept form for the reads
// kept in HBM.  Nothing here writes the table or the kept reads.  What is refused and whether a pair merges are sdt_read_plan.h's;
// the kept batches are sdt_readstage.hpp's.  The records go to sdt_gpu_compact_trimmed as they are: start, len and verdict sit where
// sdt_read_trim has them, and what comes out is the stream of the pairs that did not merge.
#include "sdt_compact.hpp"
#include "sdt_merge_kernels.cuh"

static_assert(sizeof(sdt_read_merge) == sizeof(ReadMerge) && sizeof(sdt_merge_params) == sizeof(MergeParams), "include/sdt_gpu.h and the kernel agree");
static_assert(trim_layout_compatible<sdt_read_merge>(), "sdt_gpu_compact_trimmed takes sdt_read_merge records through a pointer cast");
static_assert(SDT_MERGE_MERGED == MERGE_MERGED, "include/sdt_gpu.h and the kernel agree");

// every refusal of the parameters, before any launch; dense_reads: 0 for the kept form
static int args_ok(const sdt_merge_params *p, bool with_quals, uint64_t dense_reads)
{
	if (!p)
		return fail(SDT_EINVAL, "sdt_merge_params is NULL");
	switch (check_merge_params(MergeParams{p->min_len, p->max_len, p->phred_offset, p->flags}, with_quals, dense_reads)) {
	case MERGE_FLAGS: return fail(SDT_EINVAL, "sdt_merge_params.flags = 0x%x: no flag is known", p->flags);
	case MERGE_MAX_LEN:
		return fail(SDT_EINVAL, "sdt_merge_params.max_len = %u: below max(min_len, 1) = %u no pair could merge (0: no limit)", p->max_len,
		            p->min_len > 1 ? p->min_len : 1u);
	case MERGE_PHRED_OFFSET: return fail(SDT_EINVAL, "sdt_merge_params.phred_offset = %u: 33, 64 or 0 (the bytes are the qualities)", p->phred_offset);
	case MERGE_ODD_READS:
		return fail(SDT_EINVAL, "nreads = %llu: reads 2t and 2t + 1 are mates, an odd number of reads holds no whole pairs", (unsigned long long)dense_reads);
	default: return SDT_OK;
	}
}

// an exclusive scan over m entries of a transform of the unit index, on the context's stream
template <class Fn>
static int scan_units(sdt_ctx *c, Fn fn, uint64_t *d_out, size_t m, DevBuf &tmp)
{
	const auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), fn);
	size_t tb = 0;
	HIPCHK(rocprim::exclusive_scan(nullptr, tb, it, d_out, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	const int rc = tmp.reserve(tb, "merge scan");
	if (rc != SDT_OK) return rc;
	HIPCHK(rocprim::exclusive_scan(tmp.p, tb, it, d_out, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	return SDT_OK;
}

// what is decided about the units before anything is written: which merge, and where every merged read goes
struct MergePlan {
	DevBuf flen, new_off, rank, chunk0, bad, tmp;
	uint64_t bases = 0, merged = 0, chunks = 0, words = 0;
	unsigned long long first_bad = MERGE_NO_UNIT;        // the smallest id of a unit with inconsistent records
};

template <class Reads>
static int merge_plan(sdt_ctx *c, const Reads &reads, const Units &U, const ReadOverlap *d_ov, const sdt_merge_params *p, MergePlan &pl)
{
	const size_t m = (size_t)U.n + 1;
	int rc = pl.flen.get(m * sizeof(uint32_t), "merge lengths");
	if (rc == SDT_OK) rc = pl.new_off.get(m * sizeof(uint64_t), "merge offsets");
	if (rc == SDT_OK) rc = pl.rank.get(m * sizeof(uint64_t), "merge ranks");
	if (rc == SDT_OK) rc = pl.chunk0.get(m * sizeof(uint64_t), "merge scratch starts");
	if (rc == SDT_OK) rc = pl.bad.get(sizeof(unsigned long long), "merge check");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(pl.bad.p, 0xFF, sizeof(unsigned long long), c->stream));
	hipLaunchKernelGGL(k_merge_decide<Reads>, dim3(scan_grid(c, m)), dim3(TPB), 0, c->stream, reads, U, d_ov,
	                   MergeParams{p->min_len, p->max_len, p->phred_offset, p->flags}, (uint32_t *)pl.flen.p, (unsigned long long *)pl.bad.p);
	HIPCHK(hipGetLastError());
	const uint32_t *flen = (const uint32_t *)pl.flen.p;
	rc = scan_units(c, MergedLen{flen}, (uint64_t *)pl.new_off.p, m, pl.tmp);
	if (rc == SDT_OK) rc = scan_units(c, MergedFlag{flen}, (uint64_t *)pl.rank.p, m, pl.tmp);
	if (rc == SDT_OK) rc = scan_units(c, MergedChunks{flen}, (uint64_t *)pl.chunk0.p, m, pl.tmp);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(&pl.bases, (uint64_t *)pl.new_off.p + U.n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&pl.merged, (uint64_t *)pl.rank.p + U.n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&pl.chunks, (uint64_t *)pl.chunk0.p + U.n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&pl.first_bad, pl.bad.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	pl.words = (pl.bases + 15) >> 4;
	return SDT_OK;
}

static int merge_full(const char *what, const MergePlan &pl, uint64_t out_words_cap)
{
	return fail(SDT_EFULL, "%s: the merged reads take %llu words and %d pad words, out_words holds %llu", what, (unsigned long long)pl.words, TAIL_PAD,
	            (unsigned long long)out_words_cap);
}

// the planned units merged: the records, the dense stream of pl.words + TAIL_PAD words and its pl.merged + 1 offsets.  Waits.
template <class Reads>
static int merge_run(sdt_ctx *c, const Reads &reads, const Units &U, const ReadOverlap *d_ov, const uint8_t *d_quals, const sdt_merge_params *p,
                     const MergePlan &pl, ReadMerge *d_mg, uint32_t *d_out_words, uint64_t *d_out_offs)
{
	DevBuf scratch, src;
	// (stream_word_at reads one word past the one that holds a base: two words behind the last value)
	int rc = scratch.get((2 * pl.chunks + 2) * sizeof(uint32_t), "merge scratch");
	if (rc == SDT_OK) rc = src.get((pl.merged + 1) * sizeof(uint64_t), "merge sources");
	if (rc != SDT_OK) return rc;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	hipLaunchKernelGGL(k_merge_pairs<Reads>, dim3(wave_grid(c, U.n)), dim3(TPB), 0, c->stream, reads, U, d_ov, d_quals, p->phred_offset,
	                   (const uint32_t *)pl.flen.p, (const uint64_t *)pl.new_off.p, (const uint64_t *)pl.rank.p, (const uint64_t *)pl.chunk0.p, pl.bases,
	                   pl.merged, d_mg, (uint2 *)scratch.p, d_out_offs, (uint64_t *)src.p);
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = 2 * U.n;                                 // (reads, not k-mers: sdt_gpu_kernel_time reports them as they are)
	}
	hipLaunchKernelGGL(k_compact_words, dim3(scan_grid(c, pl.words + TAIL_PAD)), dim3(TPB), 0, c->stream, (const uint32_t *)scratch.p,
	                   (const uint64_t *)d_out_offs, (const uint64_t *)src.p, pl.merged, pl.words, d_out_words);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->stream));             // (the scratch goes when this returns)
	return SDT_OK;
}

// the kept bytes of every read of one device-resident byte stream, checked arguments
static int compact_quals_device(sdt_ctx *c, const uint8_t *d_quals, const uint64_t *d_offs, uint64_t nreads, const ReadTrim *d_recs, uint32_t *d_out,
                                uint64_t out_cap, uint64_t *n_out_bytes)
{
	DevBuf new_off, tmp;
	const size_t m = (size_t)nreads + 1;
	int rc = new_off.get(m * sizeof(uint64_t), "quality compaction offsets");
	if (rc == SDT_OK) rc = scan_units(c, TrimmedLen{d_recs, d_offs, nreads}, (uint64_t *)new_off.p, m, tmp);
	if (rc != SDT_OK) return rc;
	uint64_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, (uint64_t *)new_off.p + nreads, sizeof total, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_out_bytes) *n_out_bytes = total;
	const uint64_t padded = (total + 3) & ~3ULL;
	if (out_cap < padded)
		return fail(SDT_EFULL, "sdt_gpu_compact_quals_trimmed: the kept bytes take %llu bytes with their pad, out_quals holds %llu",
		            (unsigned long long)padded, (unsigned long long)out_cap);
	if (!total) return SDT_OK;
	hipLaunchKernelGGL(k_compact_quals, dim3(scan_grid(c, padded >> 2)), dim3(TPB), 0, c->stream, d_quals, d_offs, nreads, d_recs,
	                   (const uint64_t *)new_off.p, total, d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->stream));             // (the scan goes when this returns)
	return SDT_OK;
}

extern "C" {

int sdt_gpu_merge_pairs_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, const void *d_ov, const void *d_quals,
                               const sdt_merge_params *params, void *d_mg, void *d_out_words, uint64_t out_words_cap, void *d_out_offsets,
                               uint64_t *n_merged, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_merged) *n_merged = 0;
	if (n_out_words) *n_out_words = 0;
	if (nreads == 0) {
		if (!d_out_offsets) return SDT_OK;
		SDT_ENTER(c);
		HIPCHK(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		return SDT_OK;
	}
	if (!d_packed_words || !d_offsets || !d_ov || !d_mg || !d_out_words || !d_out_offsets)
		return fail(SDT_EINVAL, "NULL argument");
	if ((uintptr_t)d_quals & 3)
		return fail(SDT_EINVAL, "d_quals = %p: it must be 4-byte aligned", d_quals);
	int rc = args_ok(params, d_quals != nullptr, nreads);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const DenseReads reads = {(const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nullptr, nreads};
	const Units U = {nullptr, 0, UnitStretch{0, 0, 2}, nreads / 2};
	MergePlan pl;
	rc = merge_plan(c, reads, U, (const ReadOverlap *)d_ov, params, pl);     // (a pair of inconsistent records is not merged: pl.first_bad is not looked at)
	if (rc != SDT_OK) return rc;
	if (n_merged) *n_merged = pl.merged;
	if (n_out_words) *n_out_words = pl.words;
	if (out_words_cap < pl.words + TAIL_PAD)
		return merge_full("sdt_gpu_merge_pairs_device", pl, out_words_cap);
	return merge_run(c, reads, U, (const ReadOverlap *)d_ov, (const uint8_t *)d_quals, params, pl, (ReadMerge *)d_mg, (uint32_t *)d_out_words,
	                 (uint64_t *)d_out_offsets);
}

int sdt_gpu_merge_pairs(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, const sdt_read_overlap *ov,
                        const uint8_t *quals, const sdt_merge_params *params, sdt_read_merge *mg, uint32_t *out_words, uint64_t out_words_cap,
                        uint64_t *out_offsets, uint64_t *n_merged, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_merged) *n_merged = 0;
	if (n_out_words) *n_out_words = 0;
	if (nreads == 0) {
		if (out_offsets) out_offsets[0] = 0;
		return SDT_OK;
	}
	if (!packed_words || !offsets || !ov || !mg || !out_words || !out_offsets)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = args_ok(params, quals != nullptr, nreads);
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	// every pair is decided here as the device decides it: what the output takes is known, and a pair of inconsistent records
	// refuses the call, before anything is staged
	uint64_t bases = 0, merged = 0;
	for (uint64_t t = 0; t < nreads / 2; t++) {
		const uint64_t La = offsets[2 * t + 1] - offsets[2 * t], Lb = offsets[2 * t + 2] - offsets[2 * t + 1];
		const int64_t F = merge_decide(La, Lb, ov[2 * t].insert, ov[2 * t + 1].insert, params->min_len, params->max_len);
		if (F == MERGE_INCONSISTENT)
			return fail(SDT_EINVAL, "pair %llu (reads %llu and %llu of %llu and %llu bases): the overlap records say inserts %u and %u: not one overlap of these mates",
			            (unsigned long long)t, (unsigned long long)(2 * t), (unsigned long long)(2 * t + 1), (unsigned long long)La, (unsigned long long)Lb,
			            ov[2 * t].insert, ov[2 * t + 1].insert);
		if (F) { bases += (uint64_t)F; merged++; }
	}
	const uint64_t need = (bases + 15) >> 4;
	if (out_words_cap < need + TAIL_PAD) {
		if (n_merged) *n_merged = merged;
		if (n_out_words) *n_out_words = need;
		return fail(SDT_EFULL, "sdt_gpu_merge_pairs: the merged reads take %llu words and %d pad words, out_words holds %llu", (unsigned long long)need,
		            TAIL_PAD, (unsigned long long)out_words_cap);
	}
	SDT_ENTER(c);
	// the whole stream at once: the output of pieces would meet in the middle of words
	const uint64_t qbytes = quals ? (offsets[nreads] + 3) & ~3ULL : 0;
	DevBuf d_w, d_o, d_v, d_q, d_m, d_ow, d_oo;
	rc = d_w.get(in.need_words * sizeof(uint32_t), "merge staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "merge staging");
	if (rc == SDT_OK) rc = d_v.get(nreads * sizeof(ReadOverlap), "merge staging");
	if (rc == SDT_OK && quals) rc = d_q.get(qbytes, "merge staging");
	if (rc == SDT_OK) rc = d_m.get(nreads * sizeof(ReadMerge), "merge staging");
	if (rc == SDT_OK) rc = d_ow.get((need + TAIL_PAD) * sizeof(uint32_t), "merge staging");
	if (rc == SDT_OK) rc = d_oo.get((merged + 1) * sizeof(uint64_t), "merge staging");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in.need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_v.p, ov, nreads * sizeof(ReadOverlap), hipMemcpyHostToDevice, c->stream));
	if (quals && offsets[nreads]) HIPCHK(hipMemcpyAsync(d_q.p, quals, offsets[nreads], hipMemcpyHostToDevice, c->stream));
	const DenseReads reads = {(const uint32_t *)d_w.p, (const uint64_t *)d_o.p, nullptr, nreads};
	const Units U = {nullptr, 0, UnitStretch{0, 0, 2}, nreads / 2};
	MergePlan pl;
	rc = merge_plan(c, reads, U, (const ReadOverlap *)d_v.p, params, pl);
	if (rc != SDT_OK) return rc;
	if (pl.merged != merged || pl.words != need)
		return fail(SDT_EHIP, "sdt_gpu_merge_pairs: the device merged %llu pairs into %llu words, the host counted %llu into %llu",
		            (unsigned long long)pl.merged, (unsigned long long)pl.words, (unsigned long long)merged, (unsigned long long)need);
	rc = merge_run(c, reads, U, (const ReadOverlap *)d_v.p, quals ? (const uint8_t *)d_q.p : nullptr, params, pl, (ReadMerge *)d_m.p, (uint32_t *)d_ow.p,
	               (uint64_t *)d_oo.p);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpy(mg, d_m.p, nreads * sizeof(ReadMerge), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_words, d_ow.p, (need + TAIL_PAD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_offsets, d_oo.p, (merged + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (n_merged) *n_merged = merged;
	if (n_out_words) *n_out_words = need;
	return SDT_OK;
}

int sdt_gpu_merge_kept_pairs(sdt_ctx *c, const sdt_merge_params *params, const uint64_t *pair_ranges, uint64_t n_ranges, const sdt_read_overlap *ov,
                             sdt_read_merge *mg, uint64_t out_capacity, uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets,
                             uint64_t out_reads_cap, uint64_t *nreads, uint64_t *n_merged, uint64_t *n_out_words)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	if (nreads) *nreads = 0;
	if (n_merged) *n_merged = 0;
	if (n_out_words) *n_out_words = 0;
	int rc = args_ok(params, false, 0);
	if (rc == SDT_OK) rc = pair_ranges_ok(pair_ranges, n_ranges);
	if (rc == SDT_OK) rc = kept_ready(c);
	if (rc == SDT_OK) rc = kept_drained(c, "sdt_gpu_merge_kept_pairs", false);
	if (rc != SDT_OK) return rc;
	uint64_t total, most, nord;
	rc = kept_span(c, out_capacity, "mg", &total, &most, &nord);
	if (rc != SDT_OK) return rc;
	if (total == 0) {
		if (out_offsets) out_offsets[0] = 0;
		return SDT_OK;
	}
	if (!ov || !mg || !out_words || !out_offsets)
		return fail(SDT_EINVAL, "NULL argument");
	HIPCHK(hipStreamSynchronize(c->copy_stream));        // (sdt_gpu_keep_reads uploads on the copy stream)
	// as sdt_gpu_overlap_kept_pairs: the entries and the records of ALL ordinals on the device at once (sdt_readstage.hpp: KeptUnits);
	// the overlap records of ordinals that no kept read has are uploaded and never looked at
	KeptUnits ku(pair_ranges, n_ranges, nord);
	DevBuf d_ent, d_ov, d_mg, d_ow, d_oo;
	rc = d_ent.get(nord * sizeof(DedupEnt), "merge entries");
	if (rc == SDT_OK) rc = d_ov.get(nord * sizeof(ReadOverlap), "merge overlap records");
	if (rc == SDT_OK) rc = d_mg.get(nord * sizeof(ReadMerge), "merge records");
	if (rc == SDT_OK) rc = ku.d_segs.get(ku.bytes(), "merge units");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(d_mg.p, 0xFF, nord * sizeof(ReadMerge), c->stream));
	HIPCHK(hipMemcpyAsync(d_ov.p, ov, nord * sizeof(ReadOverlap), hipMemcpyHostToDevice, c->stream));
	rc = ku.upload(c);
	if (rc == SDT_OK) rc = kept_entries(c, nord, d_ent);
	const KeptReads reads = {(const DedupEnt *)d_ent.p, nord};
	const Units U = ku.on_device();
	MergePlan pl;
	if (rc == SDT_OK) rc = merge_plan(c, reads, U, (const ReadOverlap *)d_ov.p, params, pl);   // (waits)
	if (rc != SDT_OK) return rc;
	if (pl.first_bad != MERGE_NO_UNIT)
		return fail(SDT_EINVAL, "the pair at ordinals %llu and %llu: the overlap records say inserts %u and %u: not one overlap of these mates",
		            pl.first_bad, pl.first_bad + 1, ov[pl.first_bad].insert, ov[pl.first_bad + 1].insert);
	if (n_merged) *n_merged = pl.merged;
	if (n_out_words) *n_out_words = pl.words;
	if (out_words_cap < pl.words + TAIL_PAD)
		return merge_full("sdt_gpu_merge_kept_pairs", pl, out_words_cap);
	if (out_reads_cap < pl.merged)
		return fail(SDT_EFULL, "sdt_gpu_merge_kept_pairs: %llu pairs merge, out_offsets holds the offsets of %llu reads", (unsigned long long)pl.merged,
		            (unsigned long long)out_reads_cap);
	rc = d_ow.get((pl.words + TAIL_PAD) * sizeof(uint32_t), "merge output");
	if (rc == SDT_OK) rc = d_oo.get((pl.merged + 1) * sizeof(uint64_t), "merge output");
	if (rc == SDT_OK)
		rc = merge_run(c, reads, U, (const ReadOverlap *)d_ov.p, nullptr, params, pl, (ReadMerge *)d_mg.p, (uint32_t *)d_ow.p, (uint64_t *)d_oo.p);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpy(out_words, d_ow.p, (pl.words + TAIL_PAD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_offsets, d_oo.p, (pl.merged + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	rc = fetch_present<ReadMerge>(mg, d_mg, nord, MERGE_ABSENT);
	if (rc != SDT_OK) return rc;
	if (nreads) *nreads = total;
	return SDT_OK;
}

int sdt_gpu_compact_quals_trimmed_device(sdt_ctx *c, const void *d_quals, const void *d_offsets, uint64_t nreads, const void *d_recs, void *d_out_quals,
                                         uint64_t out_cap, uint64_t *n_out_bytes)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_bytes) *n_out_bytes = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!d_quals || !d_offsets || !d_recs || !d_out_quals)
		return fail(SDT_EINVAL, "NULL argument");
	if ((uintptr_t)d_out_quals & 3)
		return fail(SDT_EINVAL, "d_out_quals = %p: it must be 4-byte aligned", d_out_quals);
	SDT_ENTER(c);
	return compact_quals_device(c, (const uint8_t *)d_quals, (const uint64_t *)d_offsets, nreads, (const ReadTrim *)d_recs, (uint32_t *)d_out_quals, out_cap,
	                            n_out_bytes);
}

int sdt_gpu_compact_quals_trimmed(sdt_ctx *c, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets, uint64_t nreads, const sdt_read_trim *recs,
                                  uint8_t *out_quals, uint64_t out_cap, uint64_t *n_out_bytes)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n_out_bytes) *n_out_bytes = 0;
	if (nreads == 0)
		return SDT_OK;
	if (!quals || !offsets || !recs || !out_quals)
		return fail(SDT_EINVAL, "NULL argument");
	StreamCheck in;
	int rc = byte_stream_args_ok(offsets, nreads, nbytes, &in);
	if (rc != SDT_OK) return rc;
	uint64_t total = 0;
	for (uint64_t i = 0; i < nreads; i++) {                              // every range lies in its read
		if ((uint64_t)recs[i].start + recs[i].len > offsets[i + 1] - offsets[i])
			return fail(SDT_EINVAL, "read %llu has %llu bases, its record keeps [%u, %u + %u)", (unsigned long long)i,
			            (unsigned long long)(offsets[i + 1] - offsets[i]), recs[i].start, recs[i].start, recs[i].len);
		total += recs[i].len;
	}
	const uint64_t padded = (total + 3) & ~3ULL;
	if (n_out_bytes) *n_out_bytes = total;
	if (out_cap < padded)
		return fail(SDT_EFULL, "sdt_gpu_compact_quals_trimmed: the kept bytes take %llu bytes with their pad, out_quals holds %llu",
		            (unsigned long long)padded, (unsigned long long)out_cap);
	SDT_ENTER(c);
	DevBuf d_q, d_o, d_r, d_out;
	rc = d_q.get(offsets[nreads], "quality compaction staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "quality compaction staging");
	if (rc == SDT_OK) rc = d_r.get(nreads * sizeof(ReadTrim), "quality compaction staging");
	if (rc == SDT_OK) rc = d_out.get(padded, "quality compaction staging");
	if (rc != SDT_OK) return rc;
	if (offsets[nreads]) HIPCHK(hipMemcpyAsync(d_q.p, quals, offsets[nreads], hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_r.p, recs, nreads * sizeof(ReadTrim), hipMemcpyHostToDevice, c->stream));
	uint64_t got = 0;
	rc = compact_quals_device(c, (const uint8_t *)d_q.p, (const uint64_t *)d_o.p, nreads, (const ReadTrim *)d_r.p, (uint32_t *)d_out.p, padded, &got);
	if (rc != SDT_OK) return rc;
	if (got != total)
		return fail(SDT_EHIP, "sdt_gpu_compact_quals_trimmed: the device kept %llu bytes, the host counted %llu", (unsigned long long)got,
		            (unsigned long long)total);
	if (padded) HIPCHK(hipMemcpy(out_quals, d_out.p, padded, hipMemcpyDeviceToHost));
	return SDT_OK;
}

} // extern "C"
