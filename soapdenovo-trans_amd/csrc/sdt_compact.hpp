// sdt_compact.hpp -- the host side of the compaction of a 2-bit stream, shared by sdt_select.hip (whole kept reads) and sdt_trim.hip
// (a kept range per read): two scans, a placement kernel of the caller's, k_compact_words.
#pragma once
#include "sdt_ctx.hpp"
#include "sdt_select_kernels.cuh"
#include <rocprim/rocprim.hpp>

struct DevBuf {                                          // freed on every way out
	void *p = nullptr;
	~DevBuf() { if (p) (void)hipFree(p); }
	int get(size_t bytes, const char *what)
	{
		if (p) { (void)hipFree(p); p = nullptr; }
		const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
		if (e != hipSuccess) { p = nullptr; return fail(SDT_ENOMEM, "%s: %zu bytes: %s", what, bytes, hipGetErrorString(e)); }
		return SDT_OK;
	}
};

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
