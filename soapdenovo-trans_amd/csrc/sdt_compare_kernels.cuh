// sdt_compare_kernels.cuh -- two counted node tables compared (the rule: include/sdt_gpu.h).  One table is WALKED slot by slot, the
// other is PROBED with the k-mer of every occupied slot; nothing here writes ent or aux of either.
//   k_cmp_scan<NW, ONLY_ABSENT> : a grid-stride scan of the walked table's slots, one lane per slot, with k_asm_spectrum's entry load
//                        (key + val in one 16-byte load for 1-word keys).  The walked node's count is taken directly: val >> 48 and
//                        aux & 0xFFFF, no hash.  The stored key is canonical already, so it goes to lookup_count on the OTHER table
//                        as it is, through that table's HiView.
//                        ONLY_ABSENT = false (pass 1, A walked): every occupied slot bumps the cell [min(cA, rows - 1)][min(cB, cols - 1)]
//                        of the workgroup's matrix in LDS and feeds totals [0], [3] and, when B has the node, [2], [5], [6], [7].
//                        ONLY_ABSENT = true  (pass 2, B walked): every occupied slot feeds [1] and [4]; only a k-mer that A does NOT
//                        hold bumps a cell, and that cell is [0][min(cB, cols - 1)] -- the shared nodes were placed by pass 1.
//                        The totals are lane accumulators of 64 bits: one butterfly per wavefront at its end, then one 64-bit atomic
//                        per total and wavefront.  The matrix leaves like k_asm_spectrum's: its non-zero cells by 64-bit atomics.
//   k_cmp_select<NW>   : the same walk and probe over A.  A lane whose counts lie in the ranges takes a record slot from ap_append
//                        (sdt_append.cuh: one atomic per chunk of AP_CH records, not one per wavefront) and writes NW key words and
//                        one word cA | cB << 32.  Past the capacity ap_append says AP_NONE and the lane only counts: the number of
//                        matches is a lane accumulator, reduced per wavefront, one 64-bit atomic each -- exact whatever the capacity.
// Why no LDS counter wraps.  As in sdt_asm_kernels.cuh: a cell grows by at most 1 per slot its workgroup visits, a workgroup visits
// at most ceil(slots / (gridDim.x * TPB)) * TPB slots, and the host (sdt_compare.hip: cmp_grid, the argument of sdt_asm.hip's
// spectrum_grid) raises the grid until that is below 2^32, whatever SDT_SCAN_BLOCKS says.
// Occupancy.  The LDS of k_cmp_scan is rows x cols 32-bit counters, sized by the call and not by SDT_CMP_MAX_CELLS: the largest matrix
// (16 384 cells, 64 KiB) leaves room for two workgroups of 256 lanes on a CU of 160 KiB, 8 of its 32 wavefront slots; the command
// line's default of 64 x 64 (16 KiB) lets the registers decide, 8 workgroups.  The probe is a dependent random read per lane, so the
// wavefronts in flight are what hides it: the price of a large matrix is measured in profiles/table_compare.
#pragma once
#include "sdt_search_kernels.cuh"
#include "sdt_append.cuh"

namespace sdt {

constexpr uint32_t CMP_MAX_CELLS = 16384;                // SDT_CMP_MAX_CELLS
constexpr int CMP_TOTALS = 8;

// the entry in slot s of the walked table: false = empty; else its key and its 32-bit count
template <int NW>
__device__ inline bool cmp_walk(const Table<NW> &tbl, uint64_t s, Key<NW> &k, uint32_t &count)
{
	uint64_t val;
	if constexpr (NW == 1) {
		const ulonglong2 kv = *reinterpret_cast<const ulonglong2 *>(tbl.ent + s);
		k.w[0] = kv.x;
		val = kv.y;
	} else {
		const Entry<NW> *e = tbl.ent + s;
#pragma unroll
		for (int w = 0; w < NW; w++) k.w[w] = e->key[w];
		val = e->val;
	}
	if (k.w[0] == KEY_EMPTY) return false;
	count = (uint32_t)(val >> 48) | ((tbl.aux[s] & 0xFFFFu) << 16);
	return true;
}

__device__ inline unsigned long long cmp_wave_sum(unsigned long long v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// walked / other: see above.  hv: the high halves of OTHER.  LDS: rows * cols 32-bit counters.  totals[8], matrix[rows * cols].
template <int NW, bool ONLY_ABSENT>
__global__ __launch_bounds__(TPB) void k_cmp_scan(Table<NW> walked, Table<NW> other, HiView hv, uint32_t rows, uint32_t cols,
                                                  unsigned long long *matrix, unsigned long long *totals)
{
	extern __shared__ uint32_t smem_cmp[];
	const uint32_t cells = rows * cols;
	for (uint32_t i = threadIdx.x; i < cells; i += TPB) smem_cmp[i] = 0;
	__syncthreads();
	unsigned long long t_nodes = 0, t_sum = 0, t_both = 0, t_min = 0, t_sum_w = 0, t_sum_o = 0;
	const uint64_t slots = walked.slots();
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		Key<NW> k;
		uint32_t cw;
		if (!cmp_walk<NW>(walked, s, k, cw)) continue;
		bool found;
		const uint32_t co = lookup_count<NW>(other, k, hv, found);
		t_nodes++;
		t_sum += cw;
		if constexpr (ONLY_ABSENT) {
			if (!found) atomicAdd(&smem_cmp[cw < cols - 1 ? cw : cols - 1], 1u);
		} else {
			if (found) {
				t_both++;
				t_min += cw < co ? cw : co;
				t_sum_w += cw;
				t_sum_o += co;
			}
			atomicAdd(&smem_cmp[(cw < rows - 1 ? cw : rows - 1) * cols + (co < cols - 1 ? co : cols - 1)], 1u);
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < cells; i += TPB) {
		const uint32_t v = smem_cmp[i];
		if (v) atomicAdd(matrix + i, (unsigned long long)v);
	}
	t_nodes = cmp_wave_sum(t_nodes);
	t_sum = cmp_wave_sum(t_sum);
	if constexpr (!ONLY_ABSENT) {
		t_both = cmp_wave_sum(t_both);
		t_min = cmp_wave_sum(t_min);
		t_sum_w = cmp_wave_sum(t_sum_w);
		t_sum_o = cmp_wave_sum(t_sum_o);
	}
	if ((threadIdx.x & 63) == 0) {
		if (t_nodes) atomicAdd(totals + (ONLY_ABSENT ? 1 : 0), t_nodes);
		if (t_sum) atomicAdd(totals + (ONLY_ABSENT ? 4 : 3), t_sum);
		if constexpr (!ONLY_ABSENT) {
			if (t_both) atomicAdd(totals + 2, t_both);
			if (t_min) atomicAdd(totals + 5, t_min);
			if (t_sum_w) atomicAdd(totals + 6, t_sum_w);
			if (t_sum_o) atomicAdd(totals + 7, t_sum_o);
		}
	}
}

struct CmpRange {                                        // == sdt_cmp_range of include/sdt_gpu.h
	uint32_t min_a, max_a, min_b, max_b;
};

// chunks: records of NW + 1 words in the chunks of `out` (nullptr with out.cap_chunks == 0: count only).  matched: one counter.
template <int NW>
__global__ __launch_bounds__(TPB) void k_cmp_select(Table<NW> a, Table<NW> b, HiView hv, CmpRange rg, uint64_t *__restrict__ chunks, ApOut out,
                                                    unsigned long long *matched)
{
	__shared__ WaveApp app[TPB / 64];
	ap_init(app);
	__syncthreads();
	unsigned long long mine = 0;
	const uint64_t slots = a.slots();
	for (uint64_t s = blockIdx.x * (uint64_t)TPB + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * TPB) {
		Key<NW> k;
		uint32_t ca;
		if (!cmp_walk<NW>(a, s, k, ca)) continue;
		if (ca < rg.min_a || ca > rg.max_a) continue;        // (in front of the probe: probing first was measured, 11.4 against 10.3 ms)
		bool found;
		const uint32_t cb = lookup_count<NW>(b, k, hv, found);
		if (cb < rg.min_b || cb > rg.max_b) continue;
		mine++;
		const unsigned long long at = ap_append(app, out);
		if (at == AP_NONE) continue;
		uint64_t *rec = chunks + at * (unsigned long long)(NW + 1);
#pragma unroll
		for (int w = 0; w < NW; w++) rec[w] = k.w[w];
		rec[NW] = (uint64_t)ca | ((uint64_t)cb << 32);
	}
	ap_finish(app, out);
	mine = cmp_wave_sum(mine);
	if ((threadIdx.x & 63) == 0 && mine) atomicAdd(matched, mine);
}

} // namespace sdt
