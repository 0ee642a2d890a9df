// sdt_asm_kernels.cuh -- an assembly scored against the counted node table (the rule: include/sdt_gpu.h).  The table is asked the other
// way round: not "what is the count of this k-mer" but "which nodes do these sequences cover, and how often".  Nothing here writes ent
// or aux; the one thing written by slot is the tally cn, one byte per slot, which the context owns beside the table.
//   k_asm_support<NW>  : one wavefront per SEQUENCE, grid-stride, 64 consecutive k-mer positions per step, lane i at position 64 step +
//                        i (the shape of k_screen_reads).  A lane builds its own k-mer (global_kmer), takes the canonical strand and
//                        probes the table as k_profile_reads does (lookup_count_slot: the same loads as lookup_count, the high half
//                        through the same HiView); a found k-mer bumps its node's byte of cn.  There is NO strip of counts in LDS:
//                        what profile needs the strip for is the median, and nothing here is an order statistic -- found, solid and
//                        sum are lane accumulators reduced once per sequence, and the gaps come from ONE ballot of the weak lanes per
//                        step: their starts are mask & ~(mask << 1 | carry), the longest run is found by walking the runs of the 64-bit
//                        mask with count-trailing-zeros, with the run that reaches bit 63 carried into the next step.  The wavefront's
//                        index goes through readfirstlane, so the sequence, its offsets, the mask and the whole run walk are scalar.
//                        That is what lifts profile's limit of 16 384 k-mers: a sequence of any length costs no memory.
//                        Lane 0 writes the record; the four totals leave with one 64-bit atomic each per WAVEFRONT, at its end.
//   cn_bump            : CDNA has no byte atomics, so four tallies share a 32-bit word and a lane adds 1 << 8 b with a 32-bit
//                        compare-and-swap, and only while the byte is below 255: the add can then never carry into the neighbouring
//                        byte, and a saturated byte is left alone.  The first expected value is a plain load; it may be stale, which
//                        costs one failed swap (the swap returns the word as the memory side has it) -- and a byte that reads 255 IS
//                        255, because a tally never shrinks.  Exact under any contention: a swap that fails does so because another
//                        lane's succeeded.  A poly-A stretch puts all 64 lanes of a step on one byte: at most 64 rounds, then the byte
//                        is saturated after 255 k-mers and costs a load.  (A wave-level merge of equal slots in front of the swap
//                        would take the rounds away; it is not needed for exactness and is left out.)
//   k_asm_spectrum<NW> : a grid-stride scan over the slots: the entry (empty?  the count's low half from val >> 48), aux & 0xFFFF
//                        (the high half), the tally byte; one LDS histogram of rows x 8 32-bit counters per workgroup; the non-zero
//                        counters go out with 64-bit global atomics, as k_qc_reads flushes.
// Why no LDS counter wraps.  A counter grows by at most 1 per slot that its workgroup visits.  A workgroup visits at most
// ceil(slots / (gridDim.x * TPB)) * TPB slots, and the host (sdt_asm.hip: spectrum_grid) raises the grid until that is below 2^32,
// whatever SDT_SCAN_BLOCKS says.
#pragma once
#include "sdt_search_kernels.cuh"

namespace sdt {

struct SeqSupport {                                      // == sdt_seq_support of include/sdt_gpu.h
	uint64_t sum;
	uint32_t kmers, found, solid, gaps, longest_gap, longest_at;
};
static_assert(sizeof(SeqSupport) == 32, "sdt_seq_support is 32 bytes");

constexpr int ASM_CN_COLS = 8;                           // SDT_ASM_CN_COLS
constexpr uint32_t ASM_MAX_ROWS = 1024;                  // SDT_ASM_MAX_ROWS
constexpr uint32_t ASM_CN_MAX = 255;

// one more occurrence for the node in `slot`, saturating at 255
__device__ inline void cn_bump(uint32_t *cn, uint64_t slot)
{
	uint32_t *w = cn + (slot >> 2);
	const uint32_t sh = (uint32_t)(slot & 3) * 8;
	uint32_t seen = *w;
	while (((seen >> sh) & 0xFFu) != ASM_CN_MAX) {
		const uint32_t was = atomicCAS(w, seen, seen + (1u << sh));
		if (was == seen) break;
		seen = was;
	}
}

// the gaps of a sequence, step by step; every field is uniform over the wavefront
struct GapWalk {
	uint64_t run, run_at;                                // the weak run that reached the end of the last step: its length, its first k-mer
	uint64_t best, best_at;                              // the longest closed run, the first among equals
	uint64_t gaps;
};

__device__ inline void gap_close(GapWalk &g, uint64_t len, uint64_t at)
{
	if (len > g.best) {
		g.best = len;
		g.best_at = at;
	}
}

// mask: the weak lanes of the step whose lane 0 is k-mer p0 (a lane past the sequence's last k-mer is never weak)
__device__ inline void gap_step(GapWalk &g, uint64_t mask, uint64_t p0)
{
	g.gaps += (uint64_t)__popcll(mask & ~((mask << 1) | (g.run ? 1ULL : 0ULL)));
	uint64_t m = mask;
	if (g.run) {
		const uint64_t t = ~m ? (uint64_t)__builtin_ctzll(~m) : 64;         // how far the carried run goes on
		g.run += t;
		if (t == 64) return;
		gap_close(g, g.run, g.run_at);
		g.run = 0;
		m &= ~((1ULL << t) - 1ULL);
	}
	while (m) {
		const uint64_t s = (uint64_t)__builtin_ctzll(m), up = ~(m >> s);
		const uint64_t len = up ? (uint64_t)__builtin_ctzll(up) : 64;       // (up == 0: s == 0 and all 64 lanes are weak)
		if (s + len == 64) {                                                // reaches the step's end: carried, not closed
			g.run = len;
			g.run_at = p0 + s;
			return;
		}
		gap_close(g, len, p0 + s);
		m &= ~(((1ULL << len) - 1ULL) << s);
	}
}

// min_count: already max(min_count, 1).  out: nullptr = tally only.  totals[4]: sequences, k-mers, found, solid.
template <int NW>
__global__ __launch_bounds__(TPB) void k_asm_support(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nseqs, int K,
                                                     Table<NW> tbl, HiView hv, uint32_t min_count, uint32_t *cn, SeqSupport *__restrict__ out,
                                                     unsigned long long *totals)
{
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	uint64_t t_seqs = 0, t_kmers = 0, t_found = 0, t_solid = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + (uint64_t)wave; r < nseqs; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const uint64_t start = offs[r], len = offs[r + 1] - start;
		const uint64_t nk = len >= (uint64_t)K ? len - (uint64_t)K + 1 : 0;
		uint32_t nfound = 0, nsolid = 0;
		unsigned long long sum = 0;
		GapWalk g = {0, 0, 0, nk, 0};
		for (uint64_t p0 = 0; p0 < nk; p0 += 64) {
			const uint64_t p = p0 + (uint64_t)lane;
			bool weak = false;
			if (p < nk) {
				const Key<NW> fw = global_kmer<NW>(words, start + p, K);
				const Key<NW> rc = key_revcomp<NW>(fw, K);
				bool f;
				uint64_t slot = 0;
				const uint32_t c = lookup_count_slot<NW>(tbl, key_less<NW>(fw, rc) ? fw : rc, hv, f, slot);
				if (f) cn_bump(cn, slot);
				nfound += f;
				sum += c;
				weak = c < min_count;
				nsolid += !weak;
			}
			gap_step(g, __ballot(weak), p0);
		}
		if (g.run) gap_close(g, g.run, g.run_at);
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) {
			nfound += __shfl_xor(nfound, d);
			nsolid += __shfl_xor(nsolid, d);
			sum += __shfl_xor(sum, d);
		}
		if (lane == 0 && out) out[r] = SeqSupport{sum, (uint32_t)nk, nfound, nsolid, (uint32_t)g.gaps, (uint32_t)g.best, (uint32_t)g.best_at};
		t_seqs++;
		t_kmers += nk;
		t_found += nfound;
		t_solid += nsolid;
	}
	if (lane == 0) {
		if (t_seqs) atomicAdd(totals + 0, (unsigned long long)t_seqs);
		if (t_kmers) atomicAdd(totals + 1, (unsigned long long)t_kmers);
		if (t_found) atomicAdd(totals + 2, (unsigned long long)t_found);
		if (t_solid) atomicAdd(totals + 3, (unsigned long long)t_solid);
	}
}

// matrix[r * 8 + c] += the occupied slots with min(count, rows - 1) = r and min(cn, 7) = c.  LDS: rows * 8 32-bit counters.
template <int NW>
__global__ __launch_bounds__(TPB) void k_asm_spectrum(Table<NW> tbl, const uint8_t *__restrict__ cn, uint32_t rows, unsigned long long *matrix)
{
	extern __shared__ uint32_t smem_spectrum[];
	const uint32_t cells = rows * ASM_CN_COLS;
	for (uint32_t i = threadIdx.x; i < cells; i += TPB) smem_spectrum[i] = 0;
	__syncthreads();
	const uint64_t slots = tbl.slots();
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		uint64_t key0, val;
		if constexpr (NW == 1) {
			const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(tbl.ent + s);
			key0 = kv.x;
			val = kv.y;
		} else {
			key0 = tbl.ent[s].key[0];
			val = tbl.ent[s].val;
		}
		if (key0 == KEY_EMPTY) continue;
		const uint32_t count = (uint32_t)(val >> 48) | ((tbl.aux[s] & 0xFFFFu) << 16);
		const uint32_t row = count < rows - 1 ? count : rows - 1, c = cn[s];
		atomicAdd(&smem_spectrum[row * ASM_CN_COLS + (c < (uint32_t)ASM_CN_COLS - 1 ? c : (uint32_t)ASM_CN_COLS - 1)], 1u);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < cells; i += TPB) {
		const uint32_t v = smem_spectrum[i];
		if (v) atomicAdd(matrix + i, (unsigned long long)v);
	}
}

} // namespace sdt
