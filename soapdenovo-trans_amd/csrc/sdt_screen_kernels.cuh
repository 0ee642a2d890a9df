// sdt_screen_kernels.cuh -- reads screened against reference sequences on the device (the rule: include/sdt_gpu.h).  Needs no counted
// table and no LDS.  The set is a hash table of its own, canonical k-mer (11 <= k <= 31: one word) -> the smallest reference that holds
// it: open addressing, linear probing, slots of 16 bytes so that a probe is one 16-byte load; an empty slot is all ones (a key is below
// 2^62, and key 0, poly-A / poly-T, is a key like any other).
//   k_screen_build  : one lane per base of the staged reference stream, grid-stride.  The lane finds its sequence by bisection in the
//                     offsets and gives up where its k-mer would cross the sequence's end.  It builds its k-mer from the two or
//                     three words that hold it (screen_kmer), takes the canonical form, claims a slot with a 64-bit compare-and-swap
//                     on the key, and folds its reference in with a 32-bit atomic minimum, whether it claimed the slot or found its
//                     key there.  The claimer counts the k-mer: one atomic per wavefront at the end.
//   k_screen_lookup : one lane per key, the same probe.
//   k_screen_reads  : one wavefront per UNIT (a read, or the two mates of a pair), grid-stride.  It walks the unit's reads 64 k-mer
//                     positions per step, lane i at position 64 step + i.  Every lane builds its own k-mer as above: no rolling
//                     state crosses lanes, and no word outside the k-mer is loaded.  hits grows by the popcount of the 64-lane
//                     ballot; the smallest reference comes from one wave minimum per step that has a hit.  Both are wave-uniform.
//                     After the last read lane 0 decides the unit and writes the records and keep bytes of its reads.
// The only loops are over the steps and the probes; a probe ends because the table always has an empty slot.  No lane waits for
// another; one atomic per wavefront counts the reads kept.
#pragma once
#include "sdt_clip_kernels.cuh"

namespace sdt {

using ReadScreen = ScreenRec;                            // == sdt_read_screen of include/sdt_gpu.h
static_assert(sizeof(ReadScreen) == 24, "sdt_read_screen is six 32-bit words");

struct alignas(16) ScreenSlot {
	uint64_t key;
	uint32_t ref, pad;
};
static_assert(sizeof(ScreenSlot) == 16, "a probe is one 16-byte load");
constexpr uint64_t SCREEN_EMPTY = ~0ULL;

struct ScreenTable {
	ScreenSlot *slot;
	uint64_t mask;                                       // slots - 1
	uint32_t k;
};

// the k bases from base `at` of the stream w (16 per word, the first in the most significant pair) as a right-aligned integer; only
// the words that hold one of them are read (11 <= k <= 31: two or three words)
__device__ inline uint64_t screen_kmer(const uint32_t *w, uint64_t at, uint32_t k)
{
	const uint32_t sh = (uint32_t)(at & 15), last = sh + k - 1;
	const uint32_t *p = w + (at >> 4);
	const uint64_t hi = (uint64_t)p[0] << 32 | (last >= 16 ? p[1] : 0u);
	uint64_t v = hi << (2 * sh);
	if (last >= 32) v |= (uint64_t)p[2] >> (32 - 2 * sh);                              // (then sh > 0)
	return v >> (64 - 2 * k);
}

// the smaller of a right-aligned k-mer and its reverse complement
__device__ inline uint64_t screen_canonical(uint64_t x, uint32_t k)
{
	const uint64_t rc = rev2bit(x ^ 0xAAAAAAAAAAAAAAAAULL) >> (64 - 2 * k);
	return x < rc ? x : rc;
}

// ref(x) of a canonical k-mer, SCREEN_NO_REF if the set does not hold it
__device__ inline uint32_t screen_probe(const ScreenTable &T, uint64_t x)
{
	const uint4 *tab = (const uint4 *)T.slot;
	for (uint64_t i = mix64(x) & T.mask;; i = (i + 1) & T.mask) {
		const uint4 s = tab[i];
		const uint64_t key = (uint64_t)s.y << 32 | s.x;
		if (key == x) return s.z;
		if (key == SCREEN_EMPTY) return SCREEN_NO_REF;
	}
}

static __global__ __launch_bounds__(TPB) void k_screen_build(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nseqs,
                                                             const uint32_t *__restrict__ ref_of_seq, ScreenTable T,
                                                             unsigned long long *n_kmers)
{
	const uint64_t base0 = offs[0], nbases = offs[nseqs] - base0;
	uint32_t mine = 0;
	for (uint64_t g = blockIdx.x * (uint64_t)TPB + threadIdx.x; g < nbases; g += (uint64_t)gridDim.x * TPB) {
		const uint64_t b = base0 + g;
		uint64_t lo = 0, hi = nseqs;                                                   // the last sequence that starts at or before b
		while (hi - lo > 1) {
			const uint64_t mid = lo + ((hi - lo) >> 1);
			if (offs[mid] <= b) lo = mid; else hi = mid;
		}
		if (b + T.k > offs[lo + 1]) continue;                                          // (b < offs[lo + 1]: the sequences behind lo start past b)
		const uint64_t x = screen_canonical(screen_kmer(words, b, T.k), T.k);
		const uint32_t ref = ref_of_seq[lo];
		for (uint64_t i = mix64(x) & T.mask;; i = (i + 1) & T.mask) {
			const unsigned long long old = atomicCAS((unsigned long long *)&T.slot[i].key, (unsigned long long)SCREEN_EMPTY, (unsigned long long)x);
			if (old == SCREEN_EMPTY) mine++;
			if (old == SCREEN_EMPTY || old == x) {
				atomicMin(&T.slot[i].ref, ref);
				break;
			}
		}
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		mine += __shfl_xor(mine, d);
	if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_kmers, (unsigned long long)mine);
}

static __global__ __launch_bounds__(TPB) void k_screen_lookup(const uint64_t *__restrict__ keys, uint64_t n, ScreenTable T, uint32_t *__restrict__ refs)
{
	for (uint64_t i = blockIdx.x * (uint64_t)TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
		const uint64_t x = keys[i];
		refs[i] = x >> (2 * T.k) ? SCREEN_NO_REF : screen_probe(T, screen_canonical(x, T.k));
	}
}

// stride: the reads of a unit, 1 or 2; unit u is the reads stride * u ..
static __global__ __launch_bounds__(TPB) void k_screen_reads(DenseReads reads, uint64_t nunits, uint32_t stride, ScreenTable T, ScreenParams P,
                                                             ReadScreen *__restrict__ out, uint8_t *__restrict__ keep, unsigned long long *n_kept)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t mine = 0;
	for (uint64_t u = blockIdx.x * (uint64_t)(TPB / 64) + wave; u < nunits; u += (uint64_t)gridDim.x * (TPB / 64)) {
		ReadScreen rec[2] = {};
		bool matched = false;
#pragma unroll
		for (uint32_t m = 0; m < 2; m++) {
			if (m >= stride) break;
			const ReadRef rd = reads.ref(u * stride + m);
			const uint64_t L = rd.len, nk = L >= T.k ? L - T.k + 1 : 0;
			uint64_t hits = 0;
			uint32_t best = SCREEN_NO_REF;
			for (uint64_t p0 = 0; p0 < nk; p0 += 64) {
				const uint64_t p = p0 + lane;
				uint32_t ref = SCREEN_NO_REF;
				if (p < nk) ref = screen_probe(T, screen_canonical(screen_kmer(rd.w, rd.sh + p, T.k), T.k));
				const uint64_t hit = __ballot(ref != SCREEN_NO_REF);
				if (hit) {                                                             // (wave-uniform)
					hits += __popcll(hit);
#pragma unroll
					for (int d = 32; d > 0; d >>= 1) {
						const uint32_t o = __shfl_xor(ref, d);
						if (o < ref) ref = o;
					}
					if (ref < best) best = ref;
				}
			}
			rec[m] = ReadScreen{(uint32_t)nk, (uint32_t)hits, best, 0, (uint32_t)L, 0};
			matched = matched || screen_read_matched(nk, hits, P);
		}
		const bool dropped = !(P.flags & SCREEN_PER_READ) && screen_unit_dropped(matched, P.flags);
		if (!dropped) mine += stride;
		if (lane == 0) {
#pragma unroll
			for (uint32_t m = 0; m < 2; m++) {
				if (m >= stride) break;
				if (dropped) { rec[m].len = 0; rec[m].verdict = 1; }
				out[u * stride + m] = rec[m];
				if (keep) keep[u * stride + m] = dropped ? 0 : 1;
			}
		}
	}
	if (lane == 0 && mine) atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
