// sdt_sk_record1.h -- the COMPACT level-1 record of 1-word keys without first-occurrence ordinals, and the run cap that makes it fit
// (design: sdt_superkmer.cuh; the compact level-2 record: sdt_sk_record2.h).  Plain C++ over <stdint.h>: the kernels, the host and
// tools/sk_compact1_check.cpp (a stand-alone program under UBSan, tests/test_sk_compact1_host.py) include this file.
//
// The level-1 scatter writes a record and the level-2 scatter reads it straight back; level 2 then keeps 16 bytes of it.  Without
// ordinals nobody reads the read ordinal and the position of the 24-byte record's header (46 of its 64 bits), so what level 1 has
// to hand over is the compact level-2 record plus the level-2 bucket -- 8 + l2bits bits of header behind the bases:
//   word 0   bases 0..31, first base most significant
//   word 1   bases 32.. in the high bits | l2 << 8 | (n - 1) << 2 | has_prev << 1 | has_next        (every bit between: zero)
// With a 10-bit level-2 bucket word 1 has room for 23 bases: 55 in all (54 with 11 or 12 bits), and a run of n k-mers with its two
// context bases is n + K + 1 of them: at most 54 - K k-mers (23 at K = 31, 25 at K = 29, 31 at K = 23, 32 for K <= 22).  A record
// is 16 bytes, a level-1 chunk of 32 is 512 bytes of whole 64-byte blocks, and level 2 gets its record by clearing the l2 field.
#pragma once
#include <stdint.h>
#include "sdt_sk_record2.h"

namespace sdt {

constexpr int SK_REC1C_WORDS = 2;                // 64-bit words of a compact level-1 record

// (SDT_SK_COMPACT1=0: an A/B build in which these keys keep the 24-byte level-1 records, profiles/l1_compact)
#ifndef SDT_SK_COMPACT1
#define SDT_SK_COMPACT1 1
#endif
// the same two facts as the compact level-2 record
SDT_SK_HD inline bool sk_compact1(int nw, bool track_first) { return SDT_SK_COMPACT1 && sk_compact2(nw, track_first); }

// bits of the header field (level-2 bucket, n - 1, context flags) and its mask; bases the record holds in front of it
SDT_SK_HD inline int sk_rec1c_hdr_bits(int l2bits) { return 8 + l2bits; }
SDT_SK_HD inline uint64_t sk_rec1c_hdr_mask(int l2bits) { return (1ULL << sk_rec1c_hdr_bits(l2bits)) - 1ULL; }
SDT_SK_HD inline int sk_rec1c_bases(int l2bits) { return 32 + (64 - sk_rec1c_hdr_bits(l2bits)) / 2; }

// longest run a compact level-1 record can hold: the compact level-2 record's cap, and n + K - 1 bases + 2 context bases in front
// of the header field
SDT_SK_HD inline int sk_max_run1(int K, int l2bits)
{
	const int n2 = sk_max_run(K, 1, true), n1 = sk_rec1c_bases(l2bits) - K - 1;
	return n1 < n2 ? n1 : n2;
}

// the header field of a run (the low bits of the 24-byte record's header: sk_header)
SDT_SK_HD inline uint64_t sk_rec1c_hdr(uint32_t l2, int n, int has_prev, int has_next, int l2bits)
{
	return ((uint64_t)(l2 & ((1u << l2bits) - 1u)) << 8) | ((uint64_t)(n - 1) << 2) | ((uint64_t)has_prev << 1) | (uint64_t)has_next;
}
// header field (or a whole 24-byte header: its high bits are dropped) + the two base words, zero padded behind the run -> compact
SDT_SK_HD inline void sk_pack1(uint64_t hdr, uint64_t b0, uint64_t b1, int l2bits, uint64_t &w0, uint64_t &w1)
{
	const uint64_t m = sk_rec1c_hdr_mask(l2bits);
	w0 = b0;
	w1 = (b1 & ~m) | (hdr & m);
}
// ... and back: the base words as they were, a header with the level-2 bucket, n and the context flags (ordinal and position: zero)
SDT_SK_HD inline void sk_unpack1(uint64_t w0, uint64_t w1, int l2bits, uint64_t &hdr, uint64_t &b0, uint64_t &b1)
{
	const uint64_t m = sk_rec1c_hdr_mask(l2bits);
	hdr = w1 & m;
	b0 = w0;
	b1 = w1 & ~m;
}
SDT_SK_HD inline uint32_t sk_rec1c_l2(uint64_t w1, int l2bits) { return (uint32_t)(w1 >> 8) & ((1u << l2bits) - 1u); }
SDT_SK_HD inline int sk_rec1c_n(uint64_t w1) { return (int)((w1 >> 2) & 31u) + 1; }

// the step to the compact level-2 record: the level-2 bucket is where that record lies, its bits are cleared -- bit for bit what
// the packing of sdt_sk_record2.h makes of the 24-byte record of the same run
SDT_SK_HD inline void sk_rec1c_to_rec2c(uint64_t w0, uint64_t w1, int l2bits, uint64_t &v0, uint64_t &v1)
{
	v0 = w0;
	v1 = w1 & ~(sk_rec1c_hdr_mask(l2bits) & ~0xFFULL);
}

} // namespace sdt
