// sk_compact1_check.cpp -- CPU: the compact level-1 record of 1-word keys without ordinals and its run cap (csrc/sdt_sk_record1.h):
//   * for every K in 17..31, a level-2 bucket of 10, 11 and 12 bits, every run length n from 1 to the cap, all four combinations of
//     the context flags, random bases and level-2 buckets that include 0 and all ones: sk_pack1 / sk_unpack1 round-trip (both base
//     words, the bucket, n and the flags come back), every bit between the record's last base and the bucket field is zero;
//   * the step to the compact level-2 record equals, bit for bit, sk_pack2 of the 24-byte record of the same run (header with a
//     random read ordinal and position, bases zero padded behind the run), and its bucket bits are zero;
//   * sk_max_run1 never admits a run that does not fit in front of the bucket field or the compact level-2 record, and admits the
//     longest one that does (54 - K with a 10-bit bucket: 23 at K = 31, 32 for K <= 22).
// Built with -fsanitize=undefined by tests/test_sk_compact1_host.py (shifts by 64 are the likely slip).  Prints
// "sk_compact1_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../soapdenovo-trans_amd/csrc/sdt_sk_record1.h"
#include "../soapdenovo-trans_amd/csrc/sdt_sk_record2.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("sk_compact1_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

// `len` random bases, first base most significant, zero padded: word k holds bases 32 k .. 32 k + 31
static void random_bases(std::mt19937_64 &rng, int len, bool all_t, uint64_t (&w)[2])
{
	for (int k = 0; k < 2; k++) {
		const int keep = len - 32 * k;
		w[k] = keep <= 0 ? 0 : (all_t ? ~0ULL : rng());
		if (keep > 0 && keep < 32)
			w[k] &= ~0ULL << (64 - 2 * keep);
	}
}

// the header of the 24-byte record (sk_header of sdt_superkmer.cuh) for a level-2 bucket of l2bits bits
static uint64_t header24(uint64_t read_ord, uint32_t pos, uint32_t l2, int n, int hp, int hn, int l2bits)
{
	const uint32_t posmask = (1u << (22 - l2bits)) - 1u, l2mask = (1u << l2bits) - 1u;
	return (read_ord << 30) | ((uint64_t)(pos & posmask) << (8 + l2bits)) | ((uint64_t)(l2 & l2mask) << 8) | ((uint64_t)(n - 1) << 2) | ((uint64_t)hp << 1) | (uint64_t)hn;
}

int main(void)
{
	std::mt19937_64 rng(20261019);
	unsigned long long records = 0;
	for (int l2bits = 10; l2bits <= 12; l2bits++) {
		const int bases = sk_rec1c_bases(l2bits), hb = sk_rec1c_hdr_bits(l2bits);
		CHECK(hb == 8 + l2bits && 2 * (bases - 32) + hb <= 64 && 2 * (bases + 1 - 32) + hb > 64, "l2bits %d: %d bases in front of %d bits", l2bits, bases, hb);
		CHECK(bases == (l2bits == 10 ? 55 : 54), "l2bits %d: %d bases", l2bits, bases);
		const uint32_t l2max = (1u << l2bits) - 1u;
		for (int K = 17; K <= 31; K++) {
			const int cap = sk_max_run1(K, l2bits);
			CHECK(cap >= 1 && cap <= sk_max_run(K, 1, true) && cap <= SK_REC2C_MAX_RUN, "K %d l2bits %d: cap %d", K, l2bits, cap);
			CHECK(cap + K - 1 + 2 <= bases, "K %d l2bits %d: a run of %d k-mers with both context bases is %d bases", K, l2bits, cap, cap + K + 1);
			// the longest that fits: one more k-mer would not fit the bases or the level-2 record
			CHECK(cap == sk_max_run(K, 1, true) || cap + 1 + K - 1 + 2 > bases, "K %d l2bits %d: cap %d is not the longest run that fits", K, l2bits, cap);
			const int want = bases - 1 - K < 32 ? bases - 1 - K : 32;
			CHECK(cap == want, "K %d l2bits %d: cap %d, expected %d", K, l2bits, cap, want);
			if (l2bits == 10)
				CHECK(cap == (K <= 22 ? 32 : 54 - K), "K %d: cap %d", K, cap);
			for (int n = 1; n <= cap; n++)
				for (int flags = 0; flags < 4; flags++)
					for (int rep = 0; rep < 8; rep++) {
						const int hp = flags >> 1, hn = flags & 1, len = hp + n + K - 1 + hn;
						uint64_t b[2];
						random_bases(rng, len, rep == 2 || rep == 3, b);         // (all T: ones right up to the bucket field)
						const uint32_t l2 = rep == 0 || rep == 2 ? 0u : (rep == 1 || rep == 3 ? l2max : (uint32_t)rng() & l2max);
						const uint64_t h = header24(rng() >> 30, (uint32_t)rng(), l2, n, hp, hn, l2bits);
						CHECK((h & sk_rec1c_hdr_mask(l2bits)) == sk_rec1c_hdr(l2, n, hp, hn, l2bits), "K %d n %d: the header field is the 24-byte header's low bits", K, n);
						uint64_t w0, w1, x0, x1;
						sk_pack1(h, b[0], b[1], l2bits, w0, w1);
						sk_pack1(sk_rec1c_hdr(l2, n, hp, hn, l2bits), b[0], b[1], l2bits, x0, x1);
						CHECK(w0 == x0 && w1 == x1, "K %d n %d: the high bits of a whole header leak into the record", K, n);
						// padding: nothing between the last base and the bucket field
						CHECK(w0 == b[0], "K %d n %d: word 0", K, n);
						for (int bit = hb; bit < 64 - 2 * (len > 32 ? len - 32 : 0); bit++)
							CHECK(((w1 >> bit) & 1u) == 0, "K %d l2bits %d n %d flags %d: bit %d of word 1 is not zero", K, l2bits, n, flags, bit);
						CHECK(sk_rec1c_l2(w1, l2bits) == l2 && sk_rec1c_n(w1) == n, "K %d n %d: l2 %u n %d read back as %u %d", K, n, l2, n, sk_rec1c_l2(w1, l2bits), sk_rec1c_n(w1));
						uint64_t h2, c0, c1;
						sk_unpack1(w0, w1, l2bits, h2, c0, c1);
						CHECK(c0 == b[0] && c1 == b[1], "K %d l2bits %d n %d flags %d: base words %016llx %016llx came back as %016llx %016llx", K, l2bits, n, flags,
						      (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)c0, (unsigned long long)c1);
						CHECK(h2 == (h & sk_rec1c_hdr_mask(l2bits)), "K %d n %d flags %d: header %llx of %llx", K, n, flags, (unsigned long long)h2, (unsigned long long)h);
						CHECK((int)((h2 >> 2) & 63u) + 1 == n && (int)((h2 >> 1) & 1u) == hp && (int)(h2 & 1u) == hn && (uint32_t)(h2 >> 8) == l2, "K %d n %d flags %d: header %llx",
						      K, n, flags, (unsigned long long)h2);
						// level-1 compact -> level-2 compact == the packing of the 24-byte record of the same run
						uint64_t v0, v1, p0, p1;
						sk_rec1c_to_rec2c(w0, w1, l2bits, v0, v1);
						sk_pack2(h, b[0], b[1], p0, p1);
						CHECK(v0 == p0 && v1 == p1, "K %d l2bits %d n %d flags %d l2 %u: level 2 gets %016llx %016llx, from the 24-byte record %016llx %016llx", K, l2bits, n, flags, l2,
						      (unsigned long long)v0, (unsigned long long)v1, (unsigned long long)p0, (unsigned long long)p1);
						CHECK(((v1 >> 8) & l2max) == 0, "K %d n %d: the bucket bits are not cleared", K, n);
						records++;
					}
		}
	}
	CHECK(sk_compact1(1, false) == (SDT_SK_COMPACT1 != 0) && !sk_compact1(1, true) && !sk_compact1(2, false) && !sk_compact1(4, false), "who takes the compact form");
	printf("sk_compact1_check: ok (%llu records)\n", records);
	return 0;
}
