// sk_walk_check.cpp -- CPU: the base window, the rolling canonical m-mer and the one-pass record cut of the level-1 scatter's read walk
// (csrc/sdt_sk_walk.h) against the stream accessors the kernel used before (sk_stream_mmer, sk_stream_word of sdt_superkmer.cuh,
// sk_canon_mmer of sdt_minimizer.cuh: HIP headers, restated here in their host form):
//   * for every start phase 0..15 and every read length 1..300: the window, refilled every 16 steps, yields the read's bases one by
//     one, and walks on 64 steps past the read's end without reading past `last` -- with the stream's four pad words behind the read
//     and with none at all (the read ends in the last readable word: the clamp decides every refill near the end);
//   * for every m in 7..15 and random reads: sk_roll_step returns the canonical m-mer of the m bases that end at the step;
//   * for every start offset 0..31 and every length 1..60: sk_cut_bases<2> equals sk_stream_word + tail mask word by word (the 24-byte
//     record's base words), and so does what sk_pack1 makes of either (the 16-byte record); sk_cut_bases<4>, the 2-word keys' form,
//     the same for lengths 1..128.  The tile is a heap block of exactly the readable words, one lead word in front: a read past
//     either end stops the program.
// Built with -fsanitize=address,undefined by tests/test_sk_walk_host.py.  Prints "sk_walk_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
#include "../soapdenovo-trans_amd/csrc/sdt_sk_walk.h"
#include "../soapdenovo-trans_amd/csrc/sdt_sk_record1.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("sk_walk_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

constexpr int PAD = 4;                           // TAIL_PAD of sdt_kmer.cuh: readable words past a tile's last base

// sdt_superkmer.cuh
static uint32_t ref_stream_mmer(const uint32_t *words, int p, int m)
{
	const int s = 2 * p, wi = s >> 5, sh = s & 31;
	const uint64_t win = ((uint64_t)words[wi] << 32) | words[wi + 1];
	return (uint32_t)((win << sh) >> (64 - 2 * m));
}
static uint64_t ref_stream_word(const uint32_t *words, int p)
{
	const int s = 2 * p, wi = s >> 5, sh = s & 31;
	const uint64_t hi = ((uint64_t)words[wi] << 32) | words[wi + 1];
	return sh ? ((hi << sh) | ((uint64_t)words[wi + 2] >> (32 - sh))) : hi;
}
// sdt_minimizer.cuh
static uint32_t ref_canon_mmer(uint32_t fw, int m)
{
	uint32_t rc = 0;
	for (int i = 0; i < m; i++)
		rc |= (((fw >> (2 * i)) & 3u) ^ 2u) << (2 * (m - 1 - i));
	return fw < rc ? fw : rc;
}

// what the walk asks of the window: init at the read's base m - 1, a refill every 16 steps
static unsigned long long check_window(std::mt19937_64 &rng)
{
	unsigned long long steps = 0;
	for (int pad = 0; pad <= PAD; pad += PAD)
		for (int phase = 0; phase < 16; phase++)
			for (int len = 1; len <= 300; len++) {
				const int first = 16 * (int)(rng() % 3) + phase;
				const int nwords = (first + len + 15) / 16 + pad, last = nwords - 1;
				// the reference reads one word past the word of a base: a longer copy for it
				std::vector<uint32_t> ref((size_t)nwords + 2, 0);
				for (int i = 0; i < nwords; i++)
					ref[(size_t)i] = (uint32_t)rng();
				std::vector<uint32_t> tile(ref.begin(), ref.begin() + nwords);         // exactly the readable words
				SkBaseWin w;
				sk_win_init(w, tile.data(), first, last);
				CHECK(w.sh == 2 * phase, "phase %d: shift %d", phase, w.sh);
				for (int t = 0; t < len + 64; t++) {
					if ((t & (SK_WIN_BASES - 1)) == 0)
						sk_win_refill(w, tile.data(), last);
					const uint32_t b = sk_win_take(w);
					CHECK(b < 4, "a base is two bits");
					if (t < len)
						CHECK(b == ref_stream_mmer(ref.data(), first + t, 1), "pad %d phase %d len %d: base %d of the read is %u, the stream has %u", pad, phase, len, t, b,
						      ref_stream_mmer(ref.data(), first + t, 1));
					steps++;
				}
				CHECK(w.wi <= (first >> 4) + 2 + (len + 64) / 16, "the word index ran away: %d", w.wi);
			}
	return steps;
}

static unsigned long long check_roll(std::mt19937_64 &rng)
{
	unsigned long long mmers = 0;
	for (int m = 7; m <= 15; m++)
		for (int rep = 0; rep < 64; rep++) {
			const int first = (int)(rng() % 40), len = m + (int)(rng() % 200);
			const int nwords = (first + len + 15) / 16 + PAD, last = nwords - 1;
			std::vector<uint32_t> tile((size_t)nwords);
			for (auto &x : tile)
				x = rep == 0 ? 0u : (rep == 1 ? ~0u : (rep == 2 ? 0x1B1B1B1Bu : (uint32_t)rng()));     // (poly-A, poly-T, ACGT repeated: fw == rc happens)
			SkRoll r;
			sk_roll_init(r, ref_stream_mmer(tile.data(), first, m) >> 2);
			SkBaseWin w;
			sk_win_init(w, tile.data(), first + m - 1, last);
			for (int t = 0; t + m <= len; t++) {                 // m-mer t = bases [first + t, first + t + m)
				if ((t & (SK_WIN_BASES - 1)) == 0)
					sk_win_refill(w, tile.data(), last);
				const uint32_t canon = sk_roll_step(r, w.cur, 32 - 2 * m);
				sk_win_take(w);
				const uint32_t want = ref_canon_mmer(ref_stream_mmer(tile.data(), first + t, m), m);
				CHECK(canon == want, "m %d rep %d: canonical m-mer %d is %08x, expected %08x", m, rep, t, canon, want);
				mmers++;
			}
		}
	return mmers;
}

template <int BW> static unsigned long long check_cut(std::mt19937_64 &rng, int max_len)
{
	unsigned long long cuts = 0;
	for (int start = 0; start < 32; start++)
		for (int len = 1; len <= max_len; len++)
			for (int rep = 0; rep < 4; rep++) {
				const int p = start + 32 * (rep & 1);
				const int nwords = (p + len + 15) / 16 + PAD, last = nwords - 1;
				std::vector<uint32_t> ref((size_t)nwords + 2 * BW + 2, 0);
				for (int i = 0; i < nwords; i++)
					ref[(size_t)i] = rep >= 2 ? ~0u : (uint32_t)rng();
				std::vector<uint32_t> tile((size_t)nwords + 1);           // one lead word (LDS_LEAD in the kernel), then the readable words
				tile[0] = (uint32_t)rng();
				for (int i = 0; i < nwords; i++)
					tile[(size_t)i + 1] = ref[(size_t)i];
				uint64_t got[BW], want[BW];
				sk_cut_bases<BW, PAD>(tile.data() + 1, p, len, last, got);
				for (int k = 0; k < BW; k++) {                       // the loop sk_emit_run had
					uint64_t wv = 0;
					if (32 * k < len) {
						wv = ref_stream_word(ref.data(), p + 32 * k);
						const int keep = len - 32 * k;
						if (keep < 32)
							wv &= ~0ULL << (64 - 2 * keep);
					}
					want[k] = wv;
				}
				for (int k = 0; k < BW; k++)
					CHECK(got[k] == want[k], "BW %d start %d len %d rep %d: word %d is %016llx, expected %016llx", BW, p, len, rep, k, (unsigned long long)got[k],
					      (unsigned long long)want[k]);
				if (BW == 2) {
					const uint64_t hdr = sk_rec1c_hdr((uint32_t)rng(), 1 + (int)(rng() % 32), (int)(rng() & 1), (int)(rng() & 1), 10);
					uint64_t g0, g1, w0, w1;
					sk_pack1(hdr, got[0], got[1], 10, g0, g1);
					sk_pack1(hdr, want[0], want[1], 10, w0, w1);
					CHECK(g0 == w0 && g1 == w1, "start %d len %d: the compact record differs", p, len);
				}
				cuts++;
			}
	return cuts;
}

int main(void)
{
	std::mt19937_64 rng(20261021);
	const unsigned long long steps = check_window(rng);
	const unsigned long long mmers = check_roll(rng);
	const unsigned long long c2 = check_cut<2>(rng, 60);
	const unsigned long long c4 = check_cut<4>(rng, 128);
	printf("sk_walk_check: ok (%llu window steps, %llu m-mers, %llu + %llu cuts)\n", steps, mmers, c2, c4);
	return 0;
}
