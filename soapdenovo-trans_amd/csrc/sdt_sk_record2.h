// sdt_sk_record2.h -- the run cap of a super-k-mer record and the COMPACT level-2 record of 1-word keys (design: sdt_superkmer.cuh).
// Plain C++ over <stdint.h>: the kernels, the host and tools/sk_compact_check.cpp (a stand-alone program under UBSan,
// tests/test_sk_compact_host.py) include this one file.
//
// Without first-occurrence ordinals a level-2 record of a 1-word key needs nothing of its 8-byte header but n - 1 and the two
// context flags: the level-2 bucket is where the record lies, read ordinal and position are read under TRACK only.  A run of n
// k-mers is n + K - 1 bases + 2 context bases; capped at 60 bases the record is 120 bits of bases + one byte: 16 bytes, a group of
// four is ONE aligned 64-byte block, a chunk of 16 is 256 bytes.
//   word 0   bases 0..31, first base most significant (word 1 of the 24-byte record)
//   word 1   bases 32..59 in the high 56 bits | (n - 1) << 2 | has_prev << 1 | has_next
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SDT_SK_HD __host__ __device__
#else
#define SDT_SK_HD
#endif

namespace sdt {

constexpr int SK_MAX_RUN = 64;                   // k-mers per record (6-bit field holds n - 1)
constexpr int SK_REC2C_WORDS = 2;                // 64-bit words of a compact level-2 record
constexpr int SK_REC2C_BASES = 60;               // bases it holds
constexpr int SK_REC2C_MAX_RUN = 32;             // n - 1 and the flags share one byte (and the count stage's tile is laid out for 32)

// The compact form is used by 1-word keys without first-occurrence ordinals -- the two facts every stage derives it from, both fixed when
// the context is made.  (SDT_SK_COMPACT2=0: an A/B build in which they keep the 24-byte records, profiles/l2_compact.)
#ifndef SDT_SK_COMPACT2
#define SDT_SK_COMPACT2 1
#endif
SDT_SK_HD inline bool sk_compact2(int nw, bool track_first) { return SDT_SK_COMPACT2 && nw == 1 && !track_first; }

// longest run a record can hold: n + K - 1 bases + 2 context bases must fit the base words.  The 24 / 40 / 56-byte records take
// a power of two; the compact record takes what fits 60 bases (28 at K = 31, 30 at K = 29, 32 for K <= 27).
SDT_SK_HD inline int sk_max_run(int K, int nw, bool compact = false)
{
	const int cap = 32 * (nw == 1 ? 2 : (nw == 2 ? 4 : 6)) - K - 1;
	int n = SK_MAX_RUN;
	while (n > cap)
		n >>= 1;
	if (compact && nw == 1) {
		const int c = SK_REC2C_BASES - K - 1;
		const int m = c < SK_REC2C_MAX_RUN ? c : SK_REC2C_MAX_RUN;
		if (m < n)
			n = m;
	}
	return n;
}
// the strip kernel of level 1 cuts full records at multiples of the cap in the read (j & (ncap - 1)): it gets the largest power of two
SDT_SK_HD inline int sk_pow2_floor(int n)
{
	int p = 1;
	while (2 * p <= n)
		p *= 2;
	return p;
}

// 24-byte record (header, bases 0..31, bases 32..63 zero padded) -> compact; the record holds at most 60 bases and n <= 32
SDT_SK_HD inline void sk_pack2(uint64_t hdr, uint64_t b0, uint64_t b1, uint64_t &w0, uint64_t &w1)
{
	w0 = b0;
	w1 = (b1 & ~0xFFULL) | (hdr & 0xFFULL);
}
// ... and back: the base words as they were (low byte clear), a header with the same n and context flags (its level-2 field is
// zero: identical records still share every bit the dedupe compares, and the bucket they lie in decided the rest)
SDT_SK_HD inline void sk_unpack2(uint64_t w0, uint64_t w1, uint64_t &hdr, uint64_t &b0, uint64_t &b1)
{
	hdr = w1 & 0xFFULL;
	b0 = w0;
	b1 = w1 & ~0xFFULL;
}

} // namespace sdt
