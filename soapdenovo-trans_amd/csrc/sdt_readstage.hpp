// sdt_readstage.hpp -- the host layer of the read stages on the counted table, over the context: what sdt_search.hip (profile),
// sdt_correct.hip, sdt_select.hip (normalise) and sdt_trim.hip do the same way.  A stage is a strip kernel (one wavefront per read,
// its k-mers' counts in a strip of LDS) with up to three forms: a device-resident batch, a host batch staged in pieces, and the
// reads kept in HBM with records by read ordinal.  The decisions themselves are pure functions in sdt_read_plan.h; here they meet
// the context, the stream and the messages.  Each stage keeps its kernel's own arguments and nothing else of this.  The stages that
// need no counted table (clip, overlap, complexity, quality, screen, dedup, merge) have the same three forms around a kernel that
// counts what it keeps: their launch, their staged host form, and the kept form over pairs, are the last section.
#pragma once
#include "sdt_ctx.hpp"
#include "sdt_read_plan.h"
#include "sdt_search_kernels.cuh"
#include "sdt_dedup_kernels.cuh"
#include <type_traits>

// ---- sdt_search.hip ----
constexpr uint64_t PROFILE_CHUNK_READS = 1ULL << 22, PROFILE_CHUNK_BASES = 1ULL << 29;     // reads / bases of a host batch that are on the device at a time
uint64_t chunk_items(uint64_t dflt);               // (SDT_SEARCH_CHUNK: test hook -- pieces of that many queries / reads)
int search_ready(sdt_ctx *c, const char *what);    // the state rules of include/sdt_gpu.h, one message each
int flags_reserve(sdt_ctx *c);
int hi_prepare(sdt_ctx *c, HiView *hv);            // where a strip kernel finds the high half of a count past 65 535

struct DevBuf {                                          // freed on every way out
	void *p = nullptr;
	size_t cap = 0;
	~DevBuf() { if (p) (void)hipFree(p); }
	int get(size_t bytes, const char *what)
	{
		if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
		const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
		if (e != hipSuccess) { p = nullptr; return fail(SDT_ENOMEM, "%s: %zu bytes: %s", what, bytes, hipGetErrorString(e)); }
		cap = bytes;
		return SDT_OK;
	}
	// at least `bytes`: what it holds is kept only if it was large enough already
	int reserve(size_t bytes, const char *what) { return p && cap >= bytes ? SDT_OK : get(bytes, what); }
};

// fn(std::integral_constant<int, NW>{}) for the context's key width
template <class Fn>
static void by_key_width(const sdt_ctx *c, Fn fn)
{
	if (c->nw == 1) fn(std::integral_constant<int, 1>{});
	else if (c->nw == 2) fn(std::integral_constant<int, 2>{});
	else fn(std::integral_constant<int, 4>{});
}

// the geometry of a strip kernel over reads of up to max_read_len bases, or the refusal of reads that no strip holds
static int strip_plan(const sdt_ctx *c, uint64_t nreads, uint64_t max_read_len, StripGeometry *geo)
{
	*geo = strip_geometry(c->K, nreads, max_read_len, c->cu_count, wave_blocks_forced());
	if (!geo->fits)
		return fail(SDT_EINVAL, "reads of %llu bases do not fit the per-wavefront LDS strip (%llu k-mers, 16384 at most)",
		            (unsigned long long)geo->max_read_len, (unsigned long long)geo->mk);
	return SDT_OK;
}

// Enqueue a strip kernel for one device-resident batch.  fn(nw, geo, hv) launches it: nw is a std::integral_constant of the key width,
// geo gives grid, LDS bytes, mk and waves, hv the high halves of the counts.
template <class Fn>
static int launch_strip(sdt_ctx *c, uint64_t nreads, uint64_t max_read_len, Fn fn)
{
	HiView hv;
	int rc = hi_prepare(c, &hv);
	if (rc != SDT_OK) return rc;
	StripGeometry geo;
	rc = strip_plan(c, nreads, max_read_len, &geo);
	if (rc != SDT_OK) return rc;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) { fn(nw, geo, hv); });
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads * geo.mk;                     // (an upper bound, as for the count kernels)
	}
	return SDT_OK;
}

// (one message for the streams of bases and of bytes)
static int offsets_descend(const StreamCheck *s) { return fail(SDT_EINVAL, "offsets not monotonic at read %llu", (unsigned long long)s->read); }

// the offsets and the length of a host stream, with the two messages; s->longest: the bases of its longest read, s->need_words: its words
static int stream_args_ok(const uint64_t *offsets, uint64_t nreads, uint64_t nwords, StreamCheck *s)
{
	*s = check_stream(offsets, nreads, nwords, TAIL_PAD);
	if (s->fault == STREAM_NOT_MONOTONIC)
		return offsets_descend(s);
	if (s->fault == STREAM_TOO_SHORT)
		return fail(SDT_EINVAL, "packed_words too short: need %llu words incl. %d pad words", (unsigned long long)s->need_words, TAIL_PAD);
	return SDT_OK;
}

// A checked host batch through the device in pieces (sdt_read_plan.h: next_piece): a run of reads, the words that hold them and their
// offsets, rebased to the piece's first word.  step = 2 keeps the mates of a pair in one piece.  body(piece) runs the stage on it and
// copies its records back; it has to wait for its kernels, because the next piece is staged in the same buffers.
struct StagedPiece {
	const uint32_t *d_words;
	const uint64_t *d_offs;
	uint64_t nwords, r0, nr, maxlen;
};
template <class Body>
static int for_each_piece(sdt_ctx *c, const uint32_t *words, const uint64_t *offsets, uint64_t nreads, uint64_t step, const char *what, Body body)
{
	uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	if (step > 1) piece_reads = piece_reads < step ? step : piece_reads - piece_reads % step;
	std::vector<uint64_t> rel;
	DevBuf d_w, d_o;
	for (uint64_t r0 = 0; r0 < nreads;) {
		const ReadPiece p = next_piece(offsets, nreads, r0, step, piece_reads, PROFILE_CHUNK_BASES, TAIL_PAD);
		const uint64_t nr = p.r1 - r0;
		rel.resize(nr + 1);
		for (uint64_t i = 0; i <= nr; i++) rel[i] = offsets[r0 + i] - (p.w0 << 4);
		const size_t wbytes = p.nwords * sizeof(uint32_t), obytes = (nr + 1) * sizeof(uint64_t);
		if (d_w.cap < wbytes || d_o.cap < obytes) HIPCHK(hipStreamSynchronize(c->stream));
		int rc = d_w.reserve(wbytes, what);
		if (rc == SDT_OK) rc = d_o.reserve(obytes, what);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpyAsync(d_w.p, words + p.w0, wbytes, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, rel.data(), obytes, hipMemcpyHostToDevice, c->stream));
		rc = body(StagedPiece{(const uint32_t *)d_w.p, (const uint64_t *)d_o.p, p.nwords, r0, nr, p.maxlen});
		if (rc != SDT_OK) return rc;
		r0 = p.r1;
	}
	return SDT_OK;
}

// The same for a checked host stream of BYTES, one per base, under the offsets of the 2-bit stream (the base qualities:
// sdt_quality.hip; sdt_read_plan.h: next_byte_piece).  A piece starts at a multiple of 4 bytes of the stream, so a read keeps its
// place within a 32-bit word; the device buffer ends at a multiple of 4, and what lies behind the last read in it is not set.
struct StagedBytePiece {
	const uint8_t *d_bytes;
	const uint64_t *d_offs;
	uint64_t nbytes, r0, nr;
};
static int byte_stream_args_ok(const uint64_t *offsets, uint64_t nreads, uint64_t nbytes, StreamCheck *s)
{
	*s = check_byte_stream(offsets, nreads, nbytes);
	if (s->fault == STREAM_NOT_MONOTONIC)
		return offsets_descend(s);
	if (s->fault == STREAM_TOO_SHORT)
		return fail(SDT_EINVAL, "quals too short: need %llu bytes", (unsigned long long)s->need_words);
	return SDT_OK;
}
template <class Body>
static int for_each_byte_piece(sdt_ctx *c, const uint8_t *bytes, const uint64_t *offsets, uint64_t nreads, const char *what, Body body)
{
	const uint64_t piece_reads = chunk_items(PROFILE_CHUNK_READS);
	std::vector<uint64_t> rel;
	DevBuf d_b, d_o;
	for (uint64_t r0 = 0; r0 < nreads;) {
		const BytePiece p = next_byte_piece(offsets, nreads, r0, piece_reads, PROFILE_CHUNK_BASES);
		const uint64_t nr = p.r1 - r0;
		rel.resize(nr + 1);
		for (uint64_t i = 0; i <= nr; i++) rel[i] = offsets[r0 + i] - p.b0;
		const size_t bbytes = (p.nbytes + 3) & ~(size_t)3, obytes = (nr + 1) * sizeof(uint64_t);
		if (d_b.cap < bbytes || d_o.cap < obytes) HIPCHK(hipStreamSynchronize(c->stream));
		int rc = d_b.reserve(bbytes, what);
		if (rc == SDT_OK) rc = d_o.reserve(obytes, what);
		if (rc != SDT_OK) return rc;
		if (p.nbytes) HIPCHK(hipMemcpyAsync(d_b.p, bytes + p.b0, p.nbytes, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, rel.data(), obytes, hipMemcpyHostToDevice, c->stream));
		rc = body(StagedBytePiece{(const uint8_t *)d_b.p, (const uint64_t *)d_o.p, p.nbytes, r0, nr});
		if (rc != SDT_OK) return rc;
		r0 = p.r1;
	}
	return SDT_OK;
}

// The two counters of a strip kernel,d_cov_flags[0] (reads longer than max_read_len) and [2] (the stage's own: edits, reads kept):
// zeroed before the launch; read back after it, which waits for the kernel.  fl[] is filled before [0] is turned into the refusal.
static int flags_begin(sdt_ctx *c)
{
	const int rc = flags_reserve(c);
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemsetAsync(c->d_cov_flags, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->d_cov_flags + 2, 0, sizeof(unsigned long long), c->stream));
	return SDT_OK;
}
static int flags_end(sdt_ctx *c, const char *what, uint64_t max_read_len, unsigned long long fl[3])
{
	HIPCHK(hipMemcpyAsync(fl, c->d_cov_flags, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (fl[0])
		return fail(SDT_EINVAL, "%s: %llu reads are longer than max_read_len = %llu; their records have kmers = 0xFFFFFFFF", what, fl[0],
		            (unsigned long long)max_read_len);
	return SDT_OK;
}

// the grid of a kernel that gives every wavefront one item and strides over the rest (sdt_dedup.hip, sdt_clip.hip)
static int wave_grid(const sdt_ctx *c, uint64_t items)
{
	return (int)wave_blocks(items, TPB / 64, c->cu_count, wave_blocks_forced());
}

// ---- the reads kept in HBM ----
static int kept_ready(const sdt_ctx *c)
{
	if (!(c->flags & SDT_FLAG_KEEP_READS) && c->kept.empty())
		return fail(SDT_ESTATE, "the reads were not kept: init with SDT_FLAG_KEEP_READS (or hand them over with sdt_gpu_keep_reads)");
	return SDT_OK;
}

// every kept read's ordinal lies in the caller's array_name[out_capacity]; *total: the kept reads, *most: those of the largest batch,
// *npick: one past the largest ordinal
static int kept_span(const sdt_ctx *c, uint64_t out_capacity, const char *array_name, uint64_t *total, uint64_t *most, uint64_t *npick)
{
	const int rc = kept_ready(c);
	if (rc != SDT_OK) return rc;
	*total = *most = *npick = 0;
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		const uint64_t last = kb.ord_base + (kb.nreads - 1) * kb.ord_stride;
		if (last >= out_capacity)
			return fail(SDT_EFULL, "a kept read has ordinal %llu, %s[] holds %llu records", (unsigned long long)last, array_name,
			            (unsigned long long)out_capacity);
		*total += kb.nreads;
		if (kb.nreads > *most) *most = kb.nreads;
		if (last + 1 > *npick) *npick = last + 1;
	}
	return SDT_OK;
}

// The state rule of every kept form, with its one message: no batch whose launch is still queued; also_counted: and none that is
// counted and not yet synchronised (sdt_gpu_finish_count ends both).  Who passes what today:
//   true   search_ready, and so the forms on the counted table (profile_, correct_, trim_, select_kept_reads); sdt_gpu_complexity_kept_reads
//   false  sdt_gpu_dedup_kept_reads, clip_kept_reads, overlap_kept_pairs, merge_kept_pairs, screen_kept_reads, sdt_gpu_fetch_kept_batch
// The table-free forms read the kept reads only, and those are whole once their copy is; that complexity_ is stricter than its
// siblings is how it was written, not a need of its kernel.  A change of the rule is a change of these arguments.
static int kept_drained(const sdt_ctx *c, const char *entry, bool also_counted)
{
	if (c->staged_head < c->staged.size() || (also_counted && (c->sk.pending_kmers || c->kmers_since_sync || c->hard_since_sync)))
		return fail(SDT_ESTATE, "%s: batches were pushed and not drained: call sdt_gpu_finish_count first", entry);
	return SDT_OK;
}

// the dense records of one kept batch from the device to their ordinals in out[] (nothing else of out[] is touched)
template <class Rec>
static int scatter_by_ordinal(void *out, const sdt_ctx::KeptBatch &kb, const DevBuf &d_rec, std::vector<Rec> &tmp)
{
	HIPCHK(hipMemcpy(tmp.data(), d_rec.p, kb.nreads * sizeof(Rec), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < kb.nreads; i++)
		memcpy((char *)out + (kb.ord_base + i * kb.ord_stride) * sizeof(Rec), &tmp[i], sizeof(Rec));
	return SDT_OK;
}

// The kept form, batch by batch: dense records of `most` reads on the device, device_fn(kb, d_rec) runs the stage on one non-empty
// batch and waits for it, and the records go to their ordinals in out[] on the host.
template <class Rec, class DeviceFn>
static int for_each_kept_batch(sdt_ctx *c, void *out, uint64_t most, const char *what, DeviceFn device_fn)
{
	DevBuf d_r;
	int rc = d_r.get(most * sizeof(Rec), what);
	if (rc != SDT_OK) return rc;
	std::vector<Rec> tmp(most);
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		rc = device_fn(kb, (Rec *)d_r.p);
		if (rc == SDT_OK) rc = scatter_by_ordinal(out, kb, d_r, tmp);
		if (rc != SDT_OK) return rc;
	}
	return SDT_OK;
}

// ---- the record stages that need no counted table (clip, overlap, complexity, quality, screen, dedup, merge) ----
// One kernel that counts what it keeps in a 64-bit word on the device: the word zeroed, the launch between the events of
// sdt_gpu_kernel_time (as timed_reads reads, not k-mers), the word read back, which waits, and added to *n_kept.  fn(grid, counter)
// issues the one hipLaunchKernelGGL; grid: every wavefront one of grid_items and strides over the rest.
template <class Fn>
static int launch_counted(sdt_ctx *c, const DevBuf &ctr_buf, uint64_t grid_items, uint64_t timed_reads, uint64_t *n_kept, Fn fn)
{
	unsigned long long *ctr = (unsigned long long *)ctr_buf.p, kept = 0;
	HIPCHK(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	fn(wave_grid(c, grid_items), ctr);
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = timed_reads;
	}
	HIPCHK(hipMemcpyAsync(&kept, ctr, sizeof kept, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (n_kept) *n_kept += kept;
	return SDT_OK;
}

// The staged host form of a stage with records and a keep mask: device_fn(piece, d_rec, d_keep, &kept) runs the stage on one piece
// and waits for it; its records go to rec + piece.r0, its mask to keep + piece.r0 (keep may be NULL), the sum of kept to *n_kept.
template <class Rec, class DeviceFn>
static int staged_records(sdt_ctx *c, const uint32_t *words, const uint64_t *offsets, uint64_t nreads, uint64_t step, const char *what, void *rec,
                          uint8_t *keep, uint64_t *n_kept, DeviceFn device_fn)
{
	DevBuf d_r, d_k;
	uint64_t kept = 0;
	const int rc = for_each_piece(c, words, offsets, nreads, step, what, [&](const StagedPiece &p) -> int {
		int rc = d_r.reserve(p.nr * sizeof(Rec), what);
		if (rc == SDT_OK) rc = d_k.reserve(p.nr, what);
		if (rc == SDT_OK) rc = device_fn(p, (Rec *)d_r.p, (uint8_t *)d_k.p, &kept);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipMemcpy((Rec *)rec + p.r0, d_r.p, p.nr * sizeof(Rec), hipMemcpyDeviceToHost));
		if (keep) HIPCHK(hipMemcpy(keep + p.r0, d_k.p, p.nr, hipMemcpyDeviceToHost));
		return SDT_OK;
	});
	if (rc == SDT_OK && n_kept) *n_kept = kept;
	return rc;
}

// the pair ranges of a kept form: ascending, disjoint, whole pairs (sdt_read_plan.h: check_pair_ranges), with the messages
static int pair_ranges_ok(const uint64_t *pair_ranges, uint64_t n_ranges)
{
	if (n_ranges && !pair_ranges)
		return fail(SDT_EINVAL, "NULL argument");
	PairRangeFault fault;
	const uint64_t bad = check_pair_ranges(pair_ranges, n_ranges, &fault);
	if (fault == PAIR_RANGE_NOT_PAIRS)
		return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) does not hold whole pairs", (unsigned long long)bad,
		            (unsigned long long)pair_ranges[2 * bad], (unsigned long long)pair_ranges[2 * bad + 1]);
	if (fault == PAIR_RANGE_OVERLAPS)
		return fail(SDT_EINVAL, "pair range %llu = [%llu, %llu) starts before range %llu ends: ranges are ascending and disjoint",
		            (unsigned long long)bad, (unsigned long long)pair_ranges[2 * bad], (unsigned long long)pair_ranges[2 * bad + 1],
		            (unsigned long long)(bad - 1));
	return SDT_OK;
}

// The kept form over pairs: mates sit in different kept batches, so the records of ALL nord ordinals are on the device at once,
// preset to "no read" (0xFF), and the units are stretches of single reads and of pairs (sdt_read_plan.h: cut_unit_stretches; nord may
// cut a pair: its first mate is a unit, the kernel finds no second).  The caller reserves d_segs with its other buffers.
struct KeptUnits {
	std::vector<UnitStretch> segs;
	uint64_t units = 0;
	DevBuf d_segs;
	KeptUnits(const uint64_t *pair_ranges, uint64_t n_ranges, uint64_t nord) : segs(2 * n_ranges + 1)
	{
		segs.resize(cut_unit_stretches(pair_ranges, n_ranges, nord, segs.data(), &units));
	}
	size_t bytes() const { return segs.size() * sizeof(UnitStretch); }
	// (segs has to stay until the stream was waited for)
	int upload(sdt_ctx *c)
	{
		HIPCHK(hipMemcpyAsync(d_segs.p, segs.data(), bytes(), hipMemcpyHostToDevice, c->stream));
		return SDT_OK;
	}
	Units on_device() const { return Units{(const UnitStretch *)d_segs.p, (uint32_t)segs.size(), UnitStretch{0, 0, 1}, units}; }
};

// where the bases of every ordinal are, and their fingerprint for sdt_dedup.hip: d_ent[nord] zeroed, then k_read_fp
// (sdt_dedup_kernels.cuh) per kept batch
static int kept_entries(sdt_ctx *c, uint64_t nord, const DevBuf &d_ent)
{
	HIPCHK(hipMemsetAsync(d_ent.p, 0, nord * sizeof(DedupEnt), c->stream));
	for (const auto &kb : c->kept) {
		if (!kb.nreads) continue;
		hipLaunchKernelGGL(k_read_fp, dim3(wave_grid(c, kb.nreads)), dim3(TPB), 0, c->stream, kb.d_words, kb.d_offs, kb.nreads, (uint64_t *)nullptr,
		                   (DedupEnt *)d_ent.p, kb.ord_base, kb.ord_stride);
		HIPCHK(hipGetLastError());
	}
	return SDT_OK;
}

// the records by ordinal back in blocks; those of ordinals that no kept read has (verdict == absent) stay as the caller had them
template <class Rec>
static int fetch_present(void *out, const DevBuf &d_rec, uint64_t nord, uint32_t absent)
{
	const uint64_t block = 1ULL << 22;
	std::vector<Rec> tmp((size_t)(nord < block ? nord : block));
	for (uint64_t o0 = 0; o0 < nord; o0 += block) {
		const uint64_t k = nord - o0 < block ? nord - o0 : block;
		HIPCHK(hipMemcpy(tmp.data(), (const Rec *)d_rec.p + o0, k * sizeof(Rec), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < k; i++)
			if (tmp[i].verdict != absent) memcpy((Rec *)out + o0 + i, &tmp[i], sizeof(Rec));
	}
	return SDT_OK;
}
