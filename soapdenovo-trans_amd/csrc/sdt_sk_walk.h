// sdt_sk_walk.h -- the arithmetic of the one-lane-per-read walk of the level-1 scatter (sdt_sk_scatter_seq.cuh) that touches the packed
// base stream: the register window a lane takes its bases from, and the cut of a run's bases out of the tile in one pass.  Plain C++
// over <stdint.h>: the kernel and tools/sk_walk_check.cpp (a stand-alone program under ASan + UBSan, tests/test_sk_walk_host.py)
// include this file.  The stream: 16 bases per 32-bit word, first base in bits 31..30.
#pragma once
#include <stdint.h>
#include "sdt_sk_record2.h"

namespace sdt {

// 32 bits of the 64 bits hi:lo from `sh` bits below the top on, 0 <= sh < 32
SDT_SK_HD inline uint32_t sk_funnel32(uint32_t hi, uint32_t lo, int sh)
{
	return (uint32_t)(((((uint64_t)hi << 32) | lo) << sh) >> 32);
}
// the same for a constant 0 < SH < 32: one v_alignbit_b32 (left to itself the compiler shifts 64-bit pairs)
template <int SH> SDT_SK_HD inline uint32_t sk_funnel32c(uint32_t hi, uint32_t lo)
{
	static_assert(SH > 0 && SH < 32, "a funnel shift inside the pair");
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbit(hi, lo, 32 - SH);
#else
	return (hi << SH) | (lo >> (32 - SH));
#endif
}

// ---- the base window -------------------------------------------------------------------------------------------------------------
// A lane walks its read one base per step.  Fetching every base from the tile costs a word index, an address, an LDS read, a per-lane
// shift, a field extract and a wait in front of the hash, sixteen times over for the same word.  Instead the lane holds the next bases
// in `cur`, the next one in bits 31..30: a step looks at the top two bits and shifts cur left by two.  Every sixteen steps cur is
// empty and is refilled: 16 bases that straddle two stream words at the lane's constant bit offset 2 * (first base & 15), funnelled out
// of the word kept from the last refill (w0) and the next one, read there and then: one LDS read and one wait per sixteen steps.  (A
// read issued a refill ahead was tried: the value then lives across the branch, and every step pays a register move and a wait.)
// Every lane refills at the same steps whether or not its read still has bases (a scalar test), so the word index is clamped to the
// tile's last readable word: lanes whose read is over read harmless words, and a word a read's bases lie in is never clamped.
struct SkBaseWin {
	uint32_t cur;              // the bases not yet taken, next one on top (16 after a refill)
	uint32_t w0;               // stream word wi - 1 (clamped)
	int wi;                    // next stream word to read
	int sh;                    // 2 * (first base & 15)
};
constexpr int SK_WIN_BASES = 16;         // steps between refills

SDT_SK_HD inline int sk_win_clamp(int wi, int last) { return wi < last ? wi : last; }

// before the first step: the window is empty (the first step refills), the word the first base lies in is read
SDT_SK_HD inline void sk_win_init(SkBaseWin &w, const uint32_t *words, int first_base, int last)
{
	w.sh = 2 * (first_base & 15);
	w.wi = (first_base >> 4) + 1;
	w.cur = 0;
	w.w0 = words[sk_win_clamp(w.wi - 1, last)];
}
// at steps 0, 16, 32, ...
SDT_SK_HD inline void sk_win_refill(SkBaseWin &w, const uint32_t *words, int last)
{
	const uint32_t w1 = words[sk_win_clamp(w.wi, last)];
	w.cur = sk_funnel32(w.w0, w1, w.sh);
	w.w0 = w1;
	w.wi++;
}
// one step: the next base
SDT_SK_HD inline uint32_t sk_win_take(SkBaseWin &w)
{
	const uint32_t b = w.cur >> 30;
	w.cur <<= 2;
	return b;
}

// ---- the rolling canonical m-mer ---------------------------------------------------------------------------------------------------
// fw: the bases so far, newest in bits 1..0, never masked (the m-mer is its low 2 m bits).  rv: the same bases in reverse order, newest
// in bits 31..30, not complemented (the m-mer's reverse is its top 2 m bits).  Both take a base in one funnel shift.  The canonical
// m-mer is the smaller of the two strands right-aligned; shifting both to the top of a word keeps their order, so
// min(fw << s, rv ^ 0xAAAAAAAA) >> s, s = 32 - 2 m, is that minimum: what rv holds below its top 2 m bits decides only between equals.
struct SkRoll { uint32_t fw, rv; };

// the state after the first m - 1 bases, `first` = those bases right-aligned, first base most significant
SDT_SK_HD inline uint32_t sk_roll_rev16(uint32_t x)                // the 16 two-bit groups in reverse order
{
	x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
	x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
	x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
	return (x >> 16) | (x << 16);
}
SDT_SK_HD inline void sk_roll_init(SkRoll &r, uint32_t first)
{
	r.fw = first;
	r.rv = sk_roll_rev16(first);
}
// base `cur >> 30` enters (cur: SkBaseWin::cur before sk_win_take); returns the canonical m-mer, s = 32 - 2 m
SDT_SK_HD inline uint32_t sk_roll_step(SkRoll &r, uint32_t cur, int s)
{
	r.fw = sk_funnel32c<2>(r.fw, cur);                           // fw << 2 | base
	r.rv = sk_funnel32c<30>(r.fw, r.rv);                         // base << 30 | rv >> 2
	const uint32_t f = r.fw << s, c = r.rv ^ 0xAAAAAAAAu;
	return (f < c ? f : c) >> s;
}

// ---- the cut of a record ---------------------------------------------------------------------------------------------------------
// `len` >= 1 bases from base p of the stream on as BW 64-bit words, first base most significant, zero behind the last base.  Every
// stream word the record can span is read once (2 BW + 1 of them), neighbours are funnelled by the one bit offset of p, and the tail
// is masked per 32-bit piece from the bits that are left of the record there.  The funnel is written as the hardware's right funnel
// shift by (32 - offset) & 31; at offset 0 that returns the LOWER word, so the words are then read from one word earlier: words[-1]
// must be readable (the tile has LDS_LEAD words in front).  Words more than `pad` behind the first are clamped to `last`, the tile's
// last readable word: with pad = the readable words behind the last base (TAIL_PAD) nothing else can lie past it, and what a clamped
// word delivers is masked away.
template <int BW, int PAD = 4> SDT_SK_HD inline void sk_cut_bases(const uint32_t *words, int p, int len, int last, uint64_t (&out)[BW])
{
	int off = 2 * (p & 15);                                      // bit offset of base p in its word
#if defined(__HIP_DEVICE_COMPILE__)
	asm("" : "+v"(off));                                         // (or 32 - off, of which the funnel takes five bits, becomes p * 30: a multiply)
#endif
	const int rot = (32 - off) & 31;
	const int base = ((2 * p + 31) >> 5) - 1;                    // p >> 4, one less at offset 0
	uint32_t w[2 * BW + 1];
	for (int j = 0; j <= 2 * BW; j++)
		w[j] = words[j <= PAD ? base + j : sk_win_clamp(base + j, last)];
	for (int k = 0; k < BW; k++) {
		uint32_t o[2];
		for (int h = 0; h < 2; h++) {
			const int i = 2 * k + h;
#if defined(__HIP_DEVICE_COMPILE__)
			const uint32_t v = __builtin_amdgcn_alignbit(w[i], w[i + 1], (uint32_t)rot);
#else
			const uint32_t v = rot ? (w[i] << (32 - rot)) | (w[i + 1] >> rot) : w[i + 1];
#endif
			int z = 32 * (i + 1) - 2 * len;                      // bits of this piece behind the record: <= 0 none, >= 32 all
			z = z < 0 ? 0 : (z > 32 ? 32 : z);
			o[h] = v & (uint32_t)(0xFFFFFFFFull << z);
		}
		out[k] = ((uint64_t)o[0] << 32) | o[1];
	}
}

} // namespace sdt
