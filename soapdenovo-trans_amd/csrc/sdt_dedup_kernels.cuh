// sdt_dedup_kernels.cuh -- exact copies of a read or of a read pair dropped on the device (the rule: include/sdt_gpu.h).  A hash set
// over whole reads whose answer does not depend on the hash function, on the order of the atomics or on the launch geometry:
//   k_read_fp       : one wavefront per read: a 64-bit fingerprint of the read's BASES.  Lane i takes bases [32 i, 32 i + 32) as one
//                     64-bit value (read_chunk: a funnel shift of up to three words, zero past the read's end), mixes it with its
//                     chunk index; the chunks are summed mod 2^64, the length is mixed in last.
//   a ROUND over the units (a read, or the two mates of a pair) that are not resolved yet, three kernels, no lane ever waits:
//   k_dedup_insert  : one lane per unit: the unit's fingerprint (mates in order, or sorted under SDT_DEDUP_MATE_SWAP; salted per
//                     round) claims a slot by a CAS on the slot's fingerprint word, then the smallest unit index of the slot is kept
//                     by an atomic on its representative word.  Nothing is compared.
//   k_dedup_resolve : one wavefront per unit: finds its slot and the representative r.  r is the unit itself: kept.  Else its reads
//                     are compared with r's, lengths first, then 32-base chunks, lane i chunk i, i + 64, ...: equal: dropped, first =
//                     r's id, one atomic add on the slot's copy counter; different (a true collision of fingerprints): the unit
//                     stays unresolved and meets its own class again in the next round.
//   k_dedup_finish  : one lane per unit resolved in this round: the slot's counter into copies, the record to every read of the
//                     unit, keep[].
// Every unit of a class has the same fingerprint, so a class is resolved or put off as a whole, and the class of a slot's smallest
// unit is always resolved: the rounds end.  Every loop is bounded by the read length, the table size or the number of stretches.
#pragma once
#include "sdt_internal.hpp"
#include "sdt_read_plan.h"

namespace sdt {

struct ReadDup {                                         // == sdt_read_dup of include/sdt_gpu.h
	uint64_t first;
	uint32_t copies, verdict;
};
static_assert(sizeof(ReadDup) == 16, "sdt_read_dup is 16 bytes");

constexpr uint32_t DUP_KEPT = 0, DUP_DROPPED = 1;
constexpr uint32_t DUP_ABSENT = 0xFFFFFFFFu;             // verdict of a record that no read has written (kept form: the array is preset)
constexpr uint64_t DUP_UNRESOLVED = ~0ULL;               // first of a unit's leading record while the unit is not resolved
constexpr uint32_t DEDUP_SWAP = 1u;                      // SDT_DEDUP_MATE_SWAP

// where a read's bases are: w = the word that holds the first base, sh = that base's place in it (0 .. 15), len bases
struct ReadRef {
	const uint32_t *w;
	uint32_t sh;
	uint64_t len;
};

// bases [32 c, 32 c + 32) of the read as one 64-bit value, first base in the most significant pair, zero past the read's end
// (32 c < len).  Only words that hold a base of the chunk are read: nothing depends on the words behind the read.
__device__ inline uint64_t read_chunk(const ReadRef &r, uint64_t c)
{
	const uint64_t left = r.len - (c << 5);
	const uint32_t nb = left < 32 ? (uint32_t)left : 32u, last = r.sh + nb - 1;          // the chunk's last base, counted from word 2 c
	const uint32_t *w = r.w + (c << 1);
	const uint64_t hi = (uint64_t)w[0] << 32 | (last >= 16 ? w[1] : 0u);
	uint64_t v = hi << (2 * r.sh);
	if (last >= 32) v |= (uint64_t)w[2] >> (32 - 2 * r.sh);                            // (then sh > 0)
	return nb == 32 ? v : v & ~(~0ULL >> (2 * nb));
}

// read_chunk from any base: bases [q, q + 32) of the read (q < len) as one 64-bit value, first base in the most significant pair, zero
// past the read's end.  Only words that hold a base of the window are read.  (sdt_clip_kernels.cuh)
__device__ inline uint64_t read_window(const ReadRef &r, uint64_t q)
{
	const uint64_t left = r.len - q, at = r.sh + q;
	const uint32_t nb = left < 32 ? (uint32_t)left : 32u, sh = (uint32_t)(at & 15), last = sh + nb - 1;
	const uint32_t *w = r.w + (at >> 4);
	const uint64_t hi = (uint64_t)w[0] << 32 | (last >= 16 ? w[1] : 0u);
	uint64_t v = hi << (2 * sh);
	if (last >= 32) v |= (uint64_t)w[2] >> (32 - 2 * sh);                              // (then sh > 0)
	return nb == 32 ? v : v & ~(~0ULL >> (2 * nb));
}

// the entry of a read ordinal in the kept form: lensh = 1 << 63 | len << 4 | sh; all zero: no kept read has this ordinal
struct DedupEnt {
	uint64_t fp;
	const uint32_t *w;
	uint64_t lensh;
};
static_assert(sizeof(DedupEnt) == DEDUP_ENT_BYTES, "the entry of an ordinal is 24 bytes");

// the reads as the round kernels see them: a dense stream with a fingerprint per read, or the entries by ordinal
struct DenseReads {
	const uint32_t *words;
	const uint64_t *offs, *fp;
	uint64_t n;
	__device__ bool has(uint64_t r) const { return r < n; }
	__device__ uint64_t fp_of(uint64_t r) const { return fp[r]; }
	__device__ ReadRef ref(uint64_t r) const
	{
		const uint64_t s = offs[r];
		return ReadRef{words + (s >> 4), (uint32_t)(s & 15), offs[r + 1] - s};
	}
};
struct KeptReads {
	const DedupEnt *ent;
	uint64_t n;
	__device__ bool has(uint64_t r) const { return r < n && ent[r].lensh != 0; }
	__device__ uint64_t fp_of(uint64_t r) const { return ent[r].fp; }
	__device__ ReadRef ref(uint64_t r) const
	{
		const DedupEnt e = ent[r];
		return ReadRef{e.w, (uint32_t)(e.lensh & 15), (e.lensh << 1) >> 5};
	}
};

// read r's fingerprint to fp[r] (dense form) or its entry to ent[ord_base + r * ord_stride] (kept form)
static __global__ __launch_bounds__(TPB) void k_read_fp(const uint32_t *__restrict__ words, const uint64_t *__restrict__ offs, uint64_t nreads,
                                                        uint64_t *__restrict__ fp, DedupEnt *__restrict__ ent, uint64_t ord_base,
                                                        uint64_t ord_stride)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint64_t r = blockIdx.x * (uint64_t)(TPB / 64) + wave; r < nreads; r += (uint64_t)gridDim.x * (TPB / 64)) {
		const uint64_t s = offs[r];
		const ReadRef rd = {words + (s >> 4), (uint32_t)(s & 15), offs[r + 1] - s};
		const uint64_t nchunks = (rd.len + 31) >> 5;
		uint64_t h = 0;
		for (uint64_t c = lane; c < nchunks; c += 64)
			h += mix64(read_chunk(rd, c) ^ ((c + 1) * 0x9E3779B97F4A7C15ULL));
#pragma unroll
		for (int d = 32; d > 0; d >>= 1)
			h += __shfl_xor(h, d);
		h = mix64(h ^ mix64(rd.len + 0x632BE59BD9B4E019ULL));
		if (lane == 0) {
			if (ent) ent[ord_base + r * ord_stride] = DedupEnt{h, rd.w, 1ULL << 63 | rd.len << 4 | rd.sh};
			else fp[r] = h;
		}
	}
}

// the units: segs == NULL: the one stretch `dense`
struct Units {
	const UnitStretch *segs;
	uint32_t nsegs;
	UnitStretch dense;
	uint64_t n;
};

// unit u: its id (the index / ordinal of its first read, there or not) and the n reads of it that are there: r0, and r1 when n == 2
struct Unit {
	uint64_t id, r0, r1;
	int n;
};

template <class Reads>
__device__ inline Unit unit_of(const Units &U, const Reads &reads, uint64_t u)
{
	UnitStretch sg = U.dense;
	if (U.segs) {                                                        // the last stretch that starts at or before u
		uint32_t lo = 0, hi = U.nsegs;
		while (hi - lo > 1) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (U.segs[mid].unit0 <= u) lo = mid; else hi = mid;
		}
		sg = U.segs[lo];
	}
	Unit t;
	t.id = sg.ord0 + (u - sg.unit0) * sg.stride;
	const bool h0 = reads.has(t.id), h1 = sg.stride == 2 && reads.has(t.id + 1);
	t.r0 = h0 ? t.id : t.id + 1;
	t.r1 = t.id + 1;
	t.n = (int)h0 + (int)h1;
	return t;
}

struct DedupSlot {
	unsigned long long fp;         // 0: empty
	unsigned long long rep;        // ~ of the smallest unit index that holds this fingerprint (0: none yet)
	unsigned long long copies;     // units of the resolved class
};
static_assert(sizeof(DedupSlot) == DEDUP_SLOT_BYTES, "a slot is 24 bytes");

struct DedupRound {
	DedupSlot *tab;
	uint64_t mask;                 // slots - 1
	uint64_t salt, fp_mask;        // fp_mask: all ones (SDT_DEDUP_FP_BITS: the low bits that are kept)
	uint32_t flags;
	int first;                     // the first round: every unit is unresolved
};

// the fingerprint of a unit in this round, never 0.  A single read and a pair never share one on purpose; nothing depends on it.
template <class Reads>
__device__ inline uint64_t unit_fp(const DedupRound &R, const Reads &reads, const Unit &t)
{
	uint64_t x;
	if (t.n == 1) x = mix64(reads.fp_of(t.r0) ^ 0xA0761D6478BD642FULL);
	else {
		uint64_t a = reads.fp_of(t.r0), b = reads.fp_of(t.r1);
		if ((R.flags & DEDUP_SWAP) && b < a) { const uint64_t s = a; a = b; b = s; }
		x = mix64(mix64(a ^ 0xE7037ED1A0B428DBULL) + b * 0x9E3779B97F4A7C15ULL);
	}
	x = mix64(x ^ R.salt) & R.fp_mask;
	return x ? x : 1ULL << 63;
}

__device__ inline uint64_t slot_load(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot that holds fp, or ~0 when the probe meets an empty slot first (or, after the whole table, none)
__device__ inline uint64_t slot_find(const DedupRound &R, uint64_t fp)
{
	uint64_t s = mix64(fp) & R.mask;
	for (uint64_t i = 0; i <= R.mask; i++, s = (s + 1) & R.mask) {
		const uint64_t cur = slot_load(&R.tab[s].fp);
		if (cur == fp) return s;
		if (cur == 0) return ~0ULL;
	}
	return ~0ULL;
}

template <class Reads>
static __global__ __launch_bounds__(TPB) void k_dedup_insert(Reads reads, Units U, DedupRound R, ReadDup *__restrict__ dup)
{
	for (uint64_t u = blockIdx.x * (uint64_t)TPB + threadIdx.x; u < U.n; u += (uint64_t)gridDim.x * TPB) {
		const Unit t = unit_of(U, reads, u);
		if (!t.n) continue;
		if (R.first) dup[t.r0].first = DUP_UNRESOLVED;
		else if (dup[t.r0].first != DUP_UNRESOLVED) continue;
		const uint64_t fp = unit_fp(R, reads, t);
		uint64_t s = mix64(fp) & R.mask;
		bool found = false;
		for (uint64_t i = 0; i <= R.mask && !found; i++) {
			uint64_t cur = slot_load(&R.tab[s].fp);
			if (cur == 0) {
				cur = atomicCAS(&R.tab[s].fp, 0ULL, (unsigned long long)fp);
				if (cur == 0) cur = fp;
			}
			if (cur == fp) found = true;
			else s = (s + 1) & R.mask;
		}
		if (!found) continue;                                            // (load <= 1/2: cannot be; the unit would stay unresolved)
		const unsigned long long mine = ~(unsigned long long)u;
		if (slot_load(&R.tab[s].rep) < mine) atomicMax(&R.tab[s].rep, mine);
	}
}

// wave-uniform: are reads a and b the same length and the same bases
__device__ inline bool reads_equal(const ReadRef &a, const ReadRef &b, int lane)
{
	if (a.len != b.len) return false;
	const uint64_t nchunks = (a.len + 31) >> 5;
	for (uint64_t c0 = 0; c0 < nchunks; c0 += 64) {
		const uint64_t c = c0 + lane;
		const bool diff = c < nchunks && read_chunk(a, c) != read_chunk(b, c);
		if (__any(diff)) return false;
	}
	return true;
}

template <class Reads>
static __global__ __launch_bounds__(TPB) void k_dedup_resolve(Reads reads, Units U, DedupRound R, ReadDup *__restrict__ dup,
                                                              unsigned long long *unresolved)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t open = 0;
	for (uint64_t u = blockIdx.x * (uint64_t)(TPB / 64) + wave; u < U.n; u += (uint64_t)gridDim.x * (TPB / 64)) {
		const Unit t = unit_of(U, reads, u);
		if (!t.n || dup[t.r0].first != DUP_UNRESOLVED) continue;
		const uint64_t s = slot_find(R, unit_fp(R, reads, t));
		if (s == ~0ULL) { open++; continue; }
		const uint64_t r = ~slot_load(&R.tab[s].rep);
		uint64_t first = t.id;
		bool same = r == u;
		if (!same && r < U.n) {
			const Unit o = unit_of(U, reads, r);
			if (o.n == t.n) {
				const ReadRef a0 = reads.ref(t.r0), b0 = reads.ref(o.r0);
				if (t.n == 1) same = reads_equal(a0, b0, lane);
				else {
					const ReadRef a1 = reads.ref(t.r1), b1 = reads.ref(o.r1);
					same = reads_equal(a0, b0, lane) && reads_equal(a1, b1, lane);
					if (!same && (R.flags & DEDUP_SWAP)) same = reads_equal(a0, b1, lane) && reads_equal(a1, b0, lane);
				}
			}
			first = o.id;
		}
		if (!same) { open++; continue; }
		if (lane == 0) {
			dup[t.r0] = ReadDup{first, 0u, r == u ? DUP_KEPT : DUP_DROPPED};      // copies == 0: resolved in this round
			atomicAdd(&R.tab[s].copies, 1ULL);
		}
	}
	if (lane == 0 && open) atomicAdd(unresolved, (unsigned long long)open);
}

template <class Reads>
static __global__ __launch_bounds__(TPB) void k_dedup_finish(Reads reads, Units U, DedupRound R, ReadDup *__restrict__ dup,
                                                             uint8_t *__restrict__ keep, unsigned long long *n_kept)
{
	uint32_t mine = 0;
	for (uint64_t u0 = blockIdx.x * (uint64_t)TPB; u0 < U.n; u0 += (uint64_t)gridDim.x * TPB) {
		const uint64_t u = u0 + threadIdx.x;
		if (u >= U.n) continue;
		const Unit t = unit_of(U, reads, u);
		if (!t.n) continue;
		ReadDup rec = dup[t.r0];
		if (rec.first == DUP_UNRESOLVED || rec.copies != 0) continue;
		const uint64_t s = slot_find(R, unit_fp(R, reads, t));
		const uint64_t n = s == ~0ULL ? 1 : slot_load(&R.tab[s].copies);      // (the slot is there: the unit was resolved through it)
		rec.copies = n < 0xFFFFFFFFULL ? (uint32_t)n : 0xFFFFFFFFu;
		const uint8_t k = rec.verdict == DUP_KEPT ? 1 : 0;
		dup[t.r0] = rec;
		if (keep) keep[t.r0] = k;
		if (t.n == 2) {
			dup[t.r1] = rec;
			if (keep) keep[t.r1] = k;
		}
		if (rec.verdict == DUP_KEPT) mine += (uint32_t)t.n;
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
		mine += __shfl_xor(mine, d);
	if ((threadIdx.x & 63) == 0 && mine)
		atomicAdd(n_kept, (unsigned long long)mine);
}

} // namespace sdt
