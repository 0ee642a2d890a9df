// sdt_compact.hpp -- the host side of the compaction of a 2-bit stream, shared by sdt_select.hip (whole kept reads) and sdt_trim.hip
// (a kept range per read): two scans, a placement kernel of the caller's, k_compact_words; and the host form around it.  And the
// proof that the 24-byte records of the other stages are records of sdt_trim.hip's compaction.
#pragma once
#include "sdt_readstage.hpp"
#include "sdt_select_kernels.cuh"
#include <rocprim/rocprim.hpp>
#include <cstddef>

// the records of another stage go to sdt_gpu_compact_trimmed through a pointer cast: start, len and verdict sit where sdt_read_trim has them
template <class T>
constexpr bool trim_layout_compatible()
{
	return offsetof(T, start) == offsetof(sdt_read_trim, start) && offsetof(T, len) == offsetof(sdt_read_trim, len) &&
	       offsetof(T, verdict) == offsetof(sdt_read_trim, verdict) && sizeof(T) == sizeof(sdt_read_trim);
}

// The compaction of one device-resident stream, checked arguments.  len_of(r) / flag_of(r): the bases read r contributes and whether it
// contributes any, for r in [0, nreads] (0 at nreads).  place(grid, new_off, rank, src): enqueues the kernel that writes d_out_offs[rank[r]]
// and src[rank[r]] = where the bases of output read rank[r] start in the input.  what: the caller's name for the message.
template <class LenOf, class FlagOf, class Place>
static int compact_stream(sdt_ctx *c, const char *what, const uint32_t *d_words, uint64_t nreads, LenOf len_of, FlagOf flag_of, Place place,
                          uint32_t *d_out_words, uint64_t out_words_cap, uint64_t *d_out_offs, uint64_t *n_out_reads, uint64_t *n_out_words)
{
	DevBuf new_off, rank, src, tmp;
	const size_t m = (size_t)nreads + 1;
	int rc = new_off.get(m * sizeof(uint64_t), "compaction offsets");
	if (rc == SDT_OK) rc = rank.get(m * sizeof(uint64_t), "compaction ranks");
	if (rc == SDT_OK) rc = src.get(m * sizeof(uint64_t), "compaction sources");
	if (rc != SDT_OK) return rc;
	const auto lens = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), len_of);
	const auto flags = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), flag_of);
	size_t tb1 = 0, tb2 = 0;
	HIPCHK(rocprim::exclusive_scan(nullptr, tb1, lens, (uint64_t *)new_off.p, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	HIPCHK(rocprim::exclusive_scan(nullptr, tb2, flags, (uint64_t *)rank.p, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	rc = tmp.get(tb1 > tb2 ? tb1 : tb2, "compaction scan");
	if (rc != SDT_OK) return rc;
	HIPCHK(rocprim::exclusive_scan(tmp.p, tb1, lens, (uint64_t *)new_off.p, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	HIPCHK(rocprim::exclusive_scan(tmp.p, tb2, flags, (uint64_t *)rank.p, uint64_t(0), m, rocprim::plus<uint64_t>(), c->stream));
	place(scan_grid(c, m), (const uint64_t *)new_off.p, (const uint64_t *)rank.p, (uint64_t *)src.p);
	HIPCHK(hipGetLastError());
	uint64_t bases = 0, kept = 0;
	HIPCHK(hipMemcpyAsync(&bases, (uint64_t *)new_off.p + nreads, sizeof bases, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&kept, (uint64_t *)rank.p + nreads, sizeof kept, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	const uint64_t nw = (bases + 15) >> 4;
	if (n_out_reads) *n_out_reads = kept;
	if (n_out_words) *n_out_words = nw;
	if (out_words_cap < nw + TAIL_PAD)
		return fail(SDT_EFULL, "%s: the kept reads take %llu words and %d pad words, out_words holds %llu", what,
		            (unsigned long long)nw, TAIL_PAD, (unsigned long long)out_words_cap);
	hipLaunchKernelGGL(k_compact_words, dim3(scan_grid(c, nw + TAIL_PAD)), dim3(TPB), 0, c->stream, d_words, (const uint64_t *)d_out_offs,
	                   (const uint64_t *)src.p, kept, nw, d_out_words);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->stream));             // (the scratch arrays go when this returns)
	return SDT_OK;
}

// The compaction of a host stream, checked pointers: the whole stream at once, because the output of pieces would meet in the middle
// of words.  tally(i, bases, kept): adds what read i keeps by the caller's host array to the two sums, or refuses the record.
// sel / sel_bytes: that array, uploaded for device(d_words, d_offs, d_sel, d_out_words, out_words_cap, d_out_offs, &reads, &words),
// the caller's device form.  What the output takes is known before anything is staged: nothing is staged for one that does not fit.
template <class Tally, class Device>
static int compact_host(sdt_ctx *c, const char *what, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                        Tally tally, const void *sel, size_t sel_bytes, Device device, uint32_t *out_words, uint64_t out_words_cap,
                        uint64_t *out_offsets, uint64_t *n_out_reads, uint64_t *n_out_words)
{
	StreamCheck in;
	int rc = stream_args_ok(offsets, nreads, nwords, &in);
	uint64_t bases = 0, kept = 0;
	for (uint64_t i = 0; i < nreads && rc == SDT_OK; i++) rc = tally(i, bases, kept);
	if (rc != SDT_OK) return rc;
	const uint64_t need = (bases + 15) >> 4;
	if (out_words_cap < need + TAIL_PAD) {
		if (n_out_reads) *n_out_reads = kept;
		if (n_out_words) *n_out_words = need;
		return fail(SDT_EFULL, "%s: the kept reads take %llu words and %d pad words, out_words holds %llu", what, (unsigned long long)need, TAIL_PAD,
		            (unsigned long long)out_words_cap);
	}
	SDT_ENTER(c);
	DevBuf d_w, d_o, d_s, d_ow, d_oo;
	rc = d_w.get(in.need_words * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_o.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc == SDT_OK) rc = d_s.get(sel_bytes, "compaction staging");
	if (rc == SDT_OK) rc = d_ow.get((need + TAIL_PAD) * sizeof(uint32_t), "compaction staging");
	if (rc == SDT_OK) rc = d_oo.get((nreads + 1) * sizeof(uint64_t), "compaction staging");
	if (rc != SDT_OK) return rc;
	const uint64_t zero = 0;
	if (nreads) {
		HIPCHK(hipMemcpyAsync(d_w.p, packed_words, in.need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_o.p, offsets, (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_s.p, sel, sel_bytes, hipMemcpyHostToDevice, c->stream));
	} else {
		HIPCHK(hipMemcpyAsync(d_o.p, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
	}
	uint64_t got_reads = 0, got_words = 0;
	rc = device((const uint32_t *)d_w.p, (const uint64_t *)d_o.p, d_s.p, (uint32_t *)d_ow.p, need + TAIL_PAD, (uint64_t *)d_oo.p, &got_reads, &got_words);
	if (rc != SDT_OK) return rc;
	if (got_reads != kept || got_words != need)
		return fail(SDT_EHIP, "%s: the device kept %llu reads in %llu words, the host counted %llu in %llu", what, (unsigned long long)got_reads,
		            (unsigned long long)got_words, (unsigned long long)kept, (unsigned long long)need);
	HIPCHK(hipMemcpy(out_words, d_ow.p, (need + TAIL_PAD) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out_offsets, d_oo.p, (kept + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (n_out_reads) *n_out_reads = kept;
	if (n_out_words) *n_out_words = need;
	return SDT_OK;
}
