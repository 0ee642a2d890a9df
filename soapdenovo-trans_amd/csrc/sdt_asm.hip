// sdt_asm.hip -- an assembly scored against the counted node table (the rule: include/sdt_gpu.h): per sequence a support record, per
// node of the table how often the assembly holds it, and from the two the copy-number spectrum = k_asm_support and k_asm_spectrum
// (sdt_asm_kernels.cuh).  Nothing here writes the table: the tally is one byte per slot of the context's own, from asm_begin to
// asm_end, and it is tied to the state of the table it was begun on -- search_cache_drop (sdt_ctx.hpp) marks it stale wherever counts
// or slots change, and a stale tally is refused.  State rules and staging are those of the read stages (sdt_readstage.hpp); there is no
// strip of LDS and so no limit on the length of a sequence.
#include "sdt_readstage.hpp"
#include "sdt_asm_kernels.cuh"
#include <cstddef>

static_assert(sizeof(sdt_seq_support) == sizeof(SeqSupport) && offsetof(sdt_seq_support, sum) == 0 && offsetof(sdt_seq_support, kmers) == 8 &&
                  offsetof(sdt_seq_support, longest_at) == 28,
              "include/sdt_gpu.h and the kernel agree");
static_assert(SDT_ASM_CN_COLS == ASM_CN_COLS && SDT_ASM_MAX_ROWS == ASM_MAX_ROWS, "include/sdt_gpu.h and the kernel agree");

// a tally that add and spectrum may use: begun, and on the table as it was then
static int asm_open(const sdt_ctx *c, const char *what)
{
	if (!c->asmt.open)
		return fail(SDT_ESTATE, "%s: no assembly is being scored: call sdt_gpu_asm_begin first", what);
	if (c->asmt.stale || c->asmt.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_asm_begin", what);
	return SDT_OK;
}

static void asm_free(sdt_ctx *c)
{
	if (c->asmt.cn) (void)hipFree(c->asmt.cn);
	if (c->asmt.totals) (void)hipFree(c->asmt.totals);
	c->asmt = sdt_ctx::AsmTally();
}

// the workgroups of k_asm_spectrum: scan_grid, raised until no workgroup visits 2^32 slots (its LDS counters are 32-bit)
static int spectrum_grid(const sdt_ctx *c)
{
	uint64_t g = (uint64_t)scan_grid(c, c->slots);
	const uint64_t most = (1ULL << 32) - TPB;
	while ((c->slots / (g * TPB) + 1) * TPB > most) g *= 2;
	return (int)g;
}

// one device-resident batch, checked arguments: k_asm_support enqueued on the context's stream
static int support_device(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nseqs, SeqSupport *d_out)
{
	HiView hv;
	int rc = flags_reserve(c);                               // (hi_prepare counts the slots with a high half in d_cov_flags[1])
	if (rc == SDT_OK) rc = hi_prepare(c, &hv);
	if (rc != SDT_OK) return rc;
	const int g = wave_grid(c, nseqs);
	const uint32_t mc = c->asmt.min_count > 1 ? c->asmt.min_count : 1u;
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_asm_support<NW>, dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, nseqs, c->K, table_of<NW>(c), hv, mc, c->asmt.cn, d_out,
		                   c->asmt.totals);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nseqs;                                   // (sequences, not k-mers: their lengths are on the device only)
	}
	return SDT_OK;
}

extern "C" {

int sdt_gpu_asm_begin(sdt_ctx *c, const sdt_asm_params *params)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!params)
		return fail(SDT_EINVAL, "sdt_asm_params is NULL");
	if (params->rows < 2 || params->rows > SDT_ASM_MAX_ROWS)
		return fail(SDT_EINVAL, "sdt_asm_params.rows = %u: 2 to %u", params->rows, SDT_ASM_MAX_ROWS);
	if (params->flags)
		return fail(SDT_EINVAL, "sdt_asm_params.flags = 0x%x: no flag is defined", params->flags);
	if (params->reserved)
		return fail(SDT_EINVAL, "sdt_asm_params.reserved = %u: it must be 0", params->reserved);
	int rc = search_ready(c, "sdt_gpu_asm_begin");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const size_t cn_bytes = (size_t)((c->slots + 3) / 4) * sizeof(uint32_t), tot_bytes = (4 + (size_t)ASM_MAX_ROWS * ASM_CN_COLS) * sizeof(unsigned long long);
	if (c->asmt.cn && c->asmt.slots != c->slots) asm_free(c);
	c->asmt.open = false;
	if (!c->asmt.cn) {
		hipError_t e = hipMalloc((void **)&c->asmt.cn, cn_bytes);
		if (e == hipSuccess) e = hipMalloc((void **)&c->asmt.totals, tot_bytes);
		if (e != hipSuccess) {
			asm_free(c);
			return fail(SDT_ENOMEM, "the assembly tally: %zu bytes, one per table slot: %s", cn_bytes, hipGetErrorString(e));
		}
	}
	HIPCHK(hipMemsetAsync(c->asmt.cn, 0, cn_bytes, c->stream));
	HIPCHK(hipMemsetAsync(c->asmt.totals, 0, tot_bytes, c->stream));
	c->asmt.slots = c->slots;
	c->asmt.min_count = params->min_count;
	c->asmt.rows = params->rows;
	c->asmt.stale = false;
	c->asmt.open = true;
	return SDT_OK;
}

int sdt_gpu_asm_add_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nseqs, void *d_out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nseqs == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets)
		return fail(SDT_EINVAL, "NULL argument");
	if ((uintptr_t)d_out & 7)
		return fail(SDT_EINVAL, "d_out = %p: it must be 8-byte aligned", d_out);
	int rc = asm_open(c, "sdt_gpu_asm_add");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_asm_add");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	return support_device(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nseqs, (SeqSupport *)d_out);
}

int sdt_gpu_asm_add(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nseqs, sdt_seq_support *out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nseqs == 0)
		return SDT_OK;
	if (!packed_words || !offsets)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = asm_open(c, "sdt_gpu_asm_add");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_asm_add");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nseqs, nwords, &in);
	if (rc != SDT_OK) return rc;
	if (in.longest >> 32)
		return fail(SDT_EINVAL, "a sequence of %llu bases: the fields of sdt_seq_support are 32-bit", (unsigned long long)in.longest);
	SDT_ENTER(c);
	DevBuf d_r;
	return for_each_piece(c, packed_words, offsets, nseqs, 1, "assembly staging", [&](const StagedPiece &p) -> int {
		int rc = out ? d_r.reserve(p.nr * sizeof(SeqSupport), "assembly staging") : SDT_OK;
		if (rc == SDT_OK) rc = support_device(c, p.d_words, p.d_offs, p.nr, out ? (SeqSupport *)d_r.p : nullptr);
		if (rc != SDT_OK) return rc;
		if (out) HIPCHK(hipMemcpyAsync(out + p.r0, d_r.p, p.nr * sizeof(SeqSupport), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));             // (the next piece is staged in the same buffers)
		return SDT_OK;
	});
}

int sdt_gpu_asm_spectrum(sdt_ctx *c, uint64_t *matrix, uint64_t totals[4])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!matrix && !totals)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = asm_open(c, "sdt_gpu_asm_spectrum");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_asm_spectrum");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	const uint32_t rows = c->asmt.rows;
	const size_t mbytes = (size_t)rows * ASM_CN_COLS * sizeof(unsigned long long);
	unsigned long long *d_matrix = c->asmt.totals + 4;
	if (matrix) {
		HIPCHK(hipMemsetAsync(d_matrix, 0, mbytes, c->stream));
		const int g = spectrum_grid(c);
		by_key_width(c, [&](auto nw) {
			constexpr int NW = decltype(nw)::value;
			hipLaunchKernelGGL(k_asm_spectrum<NW>, dim3(g), dim3(TPB), (size_t)rows * ASM_CN_COLS * sizeof(uint32_t), c->stream, table_of<NW>(c),
			                   (const uint8_t *)c->asmt.cn, rows, d_matrix);
		});
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(matrix, d_matrix, mbytes, hipMemcpyDeviceToHost, c->stream));
	}
	if (totals) HIPCHK(hipMemcpyAsync(totals, c->asmt.totals, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

int sdt_gpu_asm_end(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));                 // (an add of the device form may still be running)
	asm_free(c);
	return SDT_OK;
}

} // extern "C"
