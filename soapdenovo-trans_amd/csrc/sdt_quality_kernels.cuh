// sdt_quality_kernels.cuh -- reads trimmed and filtered by their base qualities on the device (the rule: include/sdt_gpu.h).  Needs no
// table, no LDS and not the bases; every read is decided on its own by one wavefront:
//   k_quality_reads : a lane owns 4 consecutive quality bytes, taken as ONE aligned 32-bit load: the byte address is rounded down to
//                     a multiple of 4, and what lies before the read's start (`lead` bytes, 0 to 3) and past its end is masked.  A
//                     wavefront takes 256 bytes per step.  With P the sum of s_i = q_i - cut_q before the step, and everything
//                     below relative to it (32-bit: 256 * 93 fits):
//                       the lane's four local prefixes and one wave-wide inclusive sum scan of the lane totals give x, the prefix
//                       sum behind each of its bases;
//                       one wave-wide prefix minimum of x * 256 + (position in the step) -- one 32-bit key, so that the minimum
//                       carries its index and ties go to the smaller index -- gives what lies before the lane, and the lane walks
//                       its four bases from there, against the minimum carried from the earlier steps (which wins a tie: it is
//                       earlier);
//                       every base is a candidate end b with gain x - minimum; the lane's best key (gain descending, a ascending,
//                       b descending) is one 64-bit value, and one wave-wide maximum picks the step's best.
//                     What is carried from step to step is wave-uniform (readfirstlane / readlane): P and the minimum M in 64 bits,
//                     M's index, and the best (gain, a, b).  a_b never decreases with b, so a later candidate of equal gain wins iff
//                     it has the same a.
//                     With [a, b) known, the steps that meet it are walked once more (their bytes were just read) for the bases
//                     below low_q and the expected errors: two masked wave sums per step, the totals in 64 bits.  One 64-bit
//                     division per read, on uniform values.  Lane 0 writes the record and the keep byte.
// The only loops are over the steps, bounded by L / 256 + 2: there is no limit on the read length.  No lane waits for another; one
// atomic per wavefront counts the reads kept.
#pragma once
#include "sdt_clip_kernels.cuh"

namespace sdt {

struct ReadQuality {                                     // == sdt_read_quality of include/sdt_gpu.h
	uint32_t span, low, ee_ppm, start, len, verdict;
};
static_assert(sizeof(ReadQuality) == 24, "sdt_read_quality is six 32-bit words");

constexpr int QUALITY_STEP = 256;                        // bytes a wavefront takes per step: 4 per lane

// the four bytes the lane owns in step `step` of a read that starts `lead` bytes into the word at q4 and has L bytes: zero where the
// word lies wholly outside the read (it is then not loaded: nothing past the last word of the last read is touched)
__device__ inline uint32_t quality_word(const uint32_t *q4, uint64_t step, int lane, uint64_t lead_L)
{
	const uint64_t w0 = step * QUALITY_STEP + 4 * (uint64_t)lane;
	return w0 < lead_L ? q4[w0 >> 2] : 0u;
}

static __global__ __launch_bounds__(TPB) void k_quality_reads(const uint8_t *__restrict__ quals, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                              QualityParams P, ReadQuality *__restrict__ out, uint8_t *__restrict__ keep,
                                                              unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	constexpr int32_t NONE = 0x7fffffff;
	constexpr long long NO_KEY = (long long)(1ULL << 63);
	uint32_t mine = 0;
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + wave; r < nreads; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const uint64_t o0 = offs[r], L = offs[r + 1] - o0;
		const uint64_t lead = o0 & 3, lead_L = lead + L;         // positions [lead, lead_L) of the words at q4 are the read
		const uint32_t *q4 = (const uint32_t *)(quals + (o0 - lead));
		const uint64_t steps = L ? (lead_L + QUALITY_STEP - 1) / QUALITY_STEP : 0;
		// wave-uniform, carried over the steps: boundary j lies before base j; P = P_j at the step's first boundary
		long long Pc = 0, Mc = 0, Bg = 0;
		uint64_t aM = 0, Ba = 0, Bb = 0;
		for (uint64_t s = 0; s < steps; s++) {
			const uint32_t w = quality_word(q4, s, lane, lead_L);
			const uint64_t pos0 = s * QUALITY_STEP + 4 * (uint64_t)lane;          // position of the lane's first byte
			int32_t x[4];
			bool ok[4];
			int32_t t = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				ok[k] = pos0 + k >= lead && pos0 + k < lead_L;
				const int32_t q = (int32_t)quality_of(w >> (8 * k) & 255u, P.phred_offset);
				t += ok[k] ? q - (int32_t)P.cut_q : 0;
				x[k] = t;
			}
			// inclusive sum of the lane totals
			int32_t incl = t;
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const int32_t u = __shfl_up(incl, d);
				if (lane >= d) incl += u;
			}
			const int32_t excl = incl - t;
			// the minimum of the prefix sums behind the lane's bases, with its position in the step
			int32_t mn = NONE;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				x[k] += excl;
				const int32_t key = x[k] * QUALITY_STEP + (4 * lane + k);
				if (ok[k] && key < mn) mn = key;
			}
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const int32_t u = __shfl_up(mn, d);
				if (lane >= d && u < mn) mn = u;
			}
			int32_t before = __shfl_up(mn, 1);                                    // of the lanes below this one
			if (lane == 0) before = NONE;
			// the carried minimum relative to P: 0 at most.  Nothing in a step goes below -256 * 93, so a value far below that is
			// held at -2^30: it is never beaten, and differences are only taken from what beats it
			const long long Mrel = Mc - Pc;
			const int32_t Mr = Mrel < -(1LL << 30) ? -(1 << 30) : (int32_t)Mrel;
			// d: how far the minimum so far lies below the carried one (0: the carried one holds, acode 0); acode - 1: its position
			int32_t d = 0, acode = 0;
			if (before != NONE && (before >> 8) < Mr) { d = (before >> 8) - Mr; acode = 1 + (before & 255); }
			long long best = NO_KEY;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				if (!ok[k]) continue;
				if (x[k] - Mr < d) { d = x[k] - Mr; acode = 1 + 4 * lane + k; }
				// x - Mr - d >= 0 is the gain as far as Mr is Mrel; a ascending, b descending
				const long long key = (long long)(x[k] - Mr - d) * (1 << 17) + ((511 - acode) << 8) + (4 * lane + k);
				if (key > best) best = key;
			}
#pragma unroll
			for (int dd = 32; dd > 0; dd >>= 1) {
				const long long u = __shfl_xor(best, dd);
				if (u > best) best = u;
			}
			const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)best), bhi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)best >> 32));
			const long long stepbest = (long long)((unsigned long long)bhi << 32 | blo);
			const uint64_t j0 = s * QUALITY_STEP + 1 - lead;                      // boundary behind position 0 of the step (mod 2^64)
			if (stepbest != NO_KEY) {
				// the key holds x - Mr - d; the gain is x - Mrel - d
				const long long gain = (stepbest >> 17) + (Mr - Mrel);
				const uint32_t ac = 511u - (uint32_t)(stepbest >> 8 & 511), bp = (uint32_t)stepbest & 255u;
				const uint64_t a = ac ? j0 + (ac - 1) : aM, b = j0 + bp;
				if (gain > Bg || (gain == Bg && a == Ba)) { Bg = gain; Ba = a; Bb = b; }
			}
			const int32_t all = __builtin_amdgcn_readlane(mn, 63), T = __builtin_amdgcn_readlane(incl, 63);
			if (all != NONE && (all >> 8) < Mr) { Mc = Pc + (all >> 8); aM = j0 + (uint32_t)(all & 255); }
			Pc += T;
		}
		// the measures of [Ba, Bb): positions [lead + Ba, lead + Bb)
		uint64_t low = 0, E = 0;
		if (Bb > Ba) {
			const uint64_t pa = lead + Ba, pb = lead + Bb;
			for (uint64_t s = pa / QUALITY_STEP; s <= (pb - 1) / QUALITY_STEP; s++) {
				const uint32_t w = quality_word(q4, s, lane, lead_L);
				const uint64_t pos0 = s * QUALITY_STEP + 4 * (uint64_t)lane;
				uint32_t nl = 0, e = 0;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const uint32_t q = quality_of(w >> (8 * k) & 255u, P.phred_offset);
					if (pos0 + k >= pa && pos0 + k < pb) { nl += q < P.low_q ? 1u : 0u; e += QUALITY_EE_PPM[q]; }
				}
#pragma unroll
				for (int dd = 32; dd > 0; dd >>= 1) {                             // 256 * 10^6 fits 32 bits
					nl += __shfl_xor(nl, dd);
					e += __shfl_xor(e, dd);
				}
				low += __builtin_amdgcn_readfirstlane(nl);
				E += __builtin_amdgcn_readfirstlane(e);
			}
		}
		const uint64_t n = Bb - Ba;
		ReadQuality rec = {(uint32_t)n, (uint32_t)low, n ? (uint32_t)(E / n) : 0u, (uint32_t)Ba, (uint32_t)n, CLIP_CLIPPED};
		if (n < (P.min_len > 1 ? P.min_len : 1u) || 100 * low > (uint64_t)P.max_low_pct * n || (P.max_ee_ppm != 0 && rec.ee_ppm > P.max_ee_ppm)) {
			rec.start = rec.len = 0;
			rec.verdict = CLIP_DROPPED;
		} else if (n == L) rec.verdict = CLIP_WHOLE;
		if (rec.len) mine++;
		if (lane == 0) {
			out[r] = rec;
			if (keep) keep[r] = rec.len ? 1 : 0;
		}
	}
	if (lane == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
