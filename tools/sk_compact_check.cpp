// sk_compact_check.cpp -- CPU: the compact level-2 record of 1-word keys and the run cap that makes it fit (csrc/sdt_sk_record2.h):
//   * for every K in 17..31, every run length n from 1 to the cap, all four combinations of the context flags and random bases, a
//     24-byte record laid out as the level-1 scatter lays it out (header, bases zero padded behind the run) goes through
//     sk_pack2 / sk_unpack2: both base words, n and the flags come back, the level-2 field of the header comes back as zero, and in
//     the packed form every bit behind the record's last base and in front of the header byte is zero;
//   * sk_max_run in the compact case never admits a run that does not fit 60 bases or the header byte, admits the longest one that
//     does (28 at K = 31, 30 at K = 29, 32 for K <= 27), and leaves the 24 / 40 / 56-byte records' caps alone; the strip kernel's
//     cap is the largest power of two below it.
// Built with -fsanitize=undefined by tests/test_sk_compact_host.py (shifts by 64 are the likely slip).  Prints
// "sk_compact_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../soapdenovo-trans_amd/csrc/sdt_sk_record2.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("sk_compact_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

// `len` random bases, first base most significant, zero padded: word k holds bases 32 k .. 32 k + 31
static void random_bases(std::mt19937_64 &rng, int len, uint64_t (&w)[2])
{
	for (int k = 0; k < 2; k++) {
		const int keep = len - 32 * k;
		w[k] = keep <= 0 ? 0 : rng();
		if (keep > 0 && keep < 32)
			w[k] &= ~0ULL << (64 - 2 * keep);
	}
}

// the header of the 24-byte record (sk_header of sdt_superkmer.cuh; the compact form keeps its low byte only)
static uint64_t header(uint64_t read_ord, uint32_t pos, uint32_t l2, int n, int hp, int hn)
{
	return (read_ord << 30) | ((uint64_t)(pos & 0xFFFu) << 18) | ((uint64_t)(l2 & 0x3FFu) << 8) | ((uint64_t)(n - 1) << 2) | ((uint64_t)hp << 1) | (uint64_t)hn;
}

static int pow2_at_most(int cap)
{
	int n = 64;
	while (n > cap)
		n >>= 1;
	return n;
}

int main(void)
{
	std::mt19937_64 rng(20261019);
	unsigned long long records = 0;
	for (int K = 17; K <= 31; K++) {
		const int cap = sk_max_run(K, 1, true);
		CHECK(cap >= 1 && cap <= SK_REC2C_MAX_RUN, "K %d: cap %d", K, cap);
		CHECK(cap + K - 1 + 2 <= SK_REC2C_BASES, "K %d: a run of %d k-mers with both context bases is %d bases", K, cap, cap + K + 1);
		// the longest that fits: one more k-mer would not
		CHECK(cap == SK_REC2C_MAX_RUN || cap + 1 + K - 1 + 2 > SK_REC2C_BASES, "K %d: cap %d is not the longest run that fits", K, cap);
		CHECK(cap <= sk_max_run(K, 1, false), "K %d: the compact cap %d is past the 24-byte record's %d", K, cap, sk_max_run(K, 1, false));
		CHECK(cap == (K <= 27 ? 32 : 59 - K), "K %d: cap %d", K, cap);
		const int strip = sk_pow2_floor(cap);
		CHECK(strip <= cap && 2 * strip > cap && (strip & (strip - 1)) == 0, "K %d: strip cap %d of %d", K, strip, cap);
		for (int n = 1; n <= cap; n++)
			for (int flags = 0; flags < 4; flags++)
				for (int rep = 0; rep < 8; rep++) {
					const int hp = flags >> 1, hn = flags & 1, len = hp + n + K - 1 + hn;
					uint64_t b[2];
					random_bases(rng, len, b);
					const uint64_t h = header(rng() >> 30, (uint32_t)rng(), (uint32_t)rng(), n, hp, hn);
					uint64_t w0, w1;
					sk_pack2(h, b[0], b[1], w0, w1);
					// padding: nothing between the last base and the header byte
					for (int p = len; p < 64 - 4; p++) {
						const uint64_t word = p < 32 ? w0 : w1;
						CHECK(((word >> (62 - 2 * (p & 31))) & 3u) == 0, "K %d n %d flags %d: base slot %d of the packed record is not zero", K, n, flags, p);
					}
					uint64_t h2, c0, c1;
					sk_unpack2(w0, w1, h2, c0, c1);
					CHECK(c0 == b[0] && c1 == b[1], "K %d n %d flags %d: base words %016llx %016llx came back as %016llx %016llx", K, n, flags,
					      (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)c0, (unsigned long long)c1);
					CHECK((int)((h2 >> 2) & 63u) + 1 == n && (int)((h2 >> 1) & 1u) == hp && (int)(h2 & 1u) == hn, "K %d n %d flags %d: header %llx", K, n, flags, (unsigned long long)h2);
					CHECK((h2 >> 8) == 0 && h2 == (h & 0xFFu), "K %d n %d flags %d: header %llx of %llx", K, n, flags, (unsigned long long)h2, (unsigned long long)h);
					records++;
				}
	}
	// the other records keep their caps: a power of two, n + K + 1 bases within the base words
	for (int nw = 1; nw <= 4; nw *= 2) {
		const int bases = 32 * (nw == 1 ? 2 : (nw == 2 ? 4 : 6));
		const int k_lo = nw == 1 ? 13 : (nw == 2 ? 33 : 65), k_hi = nw == 1 ? 31 : (nw == 2 ? 63 : 127);
		for (int K = k_lo; K <= k_hi; K++) {
			const int cap = sk_max_run(K, nw, false);
			CHECK(cap == sk_max_run(K, nw), "the default is the full record");
			CHECK(cap == pow2_at_most(bases - K - 1) && cap + K + 1 <= bases, "nw %d K %d: cap %d", nw, K, cap);
			CHECK(sk_pow2_floor(cap) == cap, "nw %d K %d: cap %d is no power of two", nw, K, cap);
		}
	}
	CHECK(sk_compact2(1, false) && !sk_compact2(1, true) && !sk_compact2(2, false) && !sk_compact2(4, false), "who takes the compact form");
	printf("sk_compact_check: ok (%llu records)\n", records);
	return 0;
}
