// read_plan_check.cpp -- CPU: what the read stages decide on the host before anything reaches the device (csrc/sdt_read_plan.h):
//   * strip_geometry: 4 / 2 / 1 wavefronts at 4 096 / 8 192 / 16 384 k-mers, the LDS bytes, the refusal one k-mer further, the grid;
//   * wave_blocks: the grid of every kernel that gives a wavefront a read, unchanged without SDT_WAVE_BLOCKS, and what the hook forces;
//   * next_piece: on ragged offsets the pieces tile the batch, keep pairs whole, respect both caps (reads AND bases), are maximal --
//     which with the tiling fixes the cut -- and name the right words; every offsets array is malloc'ed to exactly nreads + 1
//     entries, so that under AddressSanitizer a look past it is a finding;
//   * check_stream: the first read that ends before it starts, the words a stream needs, streams of no reads.
// Built with -fsanitize=address,undefined by tests/test_read_plan.py.  Prints "read_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("read_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static const uint64_t PAD = 4;

static void geometry(void)
{
	static const struct { uint64_t mk; int waves; } steps[] = {{1, 4}, {4096, 4}, {4097, 2}, {8192, 2}, {8193, 1}, {16384, 1}};
	static const int Ks[] = {13, 31, 63, 127}, cus[] = {1, 8, 256};
	for (const int K : Ks) {
		for (const auto &s : steps) {
			const StripGeometry g = strip_geometry(K, 1000, s.mk + K - 1, 256);
			CHECK(g.fits && g.mk == s.mk && g.max_read_len == s.mk + K - 1, "K %d mk %llu", K, (unsigned long long)s.mk);
			CHECK(g.waves == s.waves, "K %d mk %llu: %d waves, expected %d", K, (unsigned long long)s.mk, g.waves, s.waves);
			CHECK(g.lds_bytes == 4 * s.mk * s.waves && g.lds_bytes <= 65536, "K %d mk %llu: %u LDS bytes", K, (unsigned long long)s.mk, g.lds_bytes);
			for (const int cu : cus) {
				const uint64_t full = (uint64_t)s.waves * cu * 32;
				CHECK(strip_geometry(K, 0, s.mk + K - 1, cu).blocks == 1, "no reads");
				CHECK(strip_geometry(K, 1, s.mk + K - 1, cu).blocks == 1, "one read");
				CHECK(strip_geometry(K, full + 1, s.mk + K - 1, cu).blocks == (uint32_t)cu * 32, "one read past a full grid");
				CHECK(strip_geometry(K, full, s.mk + K - 1, cu).blocks == (uint32_t)cu * 32, "a full grid");
				CHECK(strip_geometry(K, (uint64_t)s.waves + 1, s.mk + K - 1, cu).blocks == 2, "one read past a workgroup");
			}
		}
		const StripGeometry over = strip_geometry(K, 1000, 16385 + K - 1, 256);
		CHECK(!over.fits && over.mk == 16385 && over.max_read_len == (uint64_t)16385 + K - 1, "K %d: 16 385 k-mers were not refused", K);
		CHECK(!strip_geometry(K, 1, ~0ULL, 256).fits, "K %d: the longest length there is", K);
		for (const uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)K - 1, (uint64_t)K}) {
			const StripGeometry g = strip_geometry(K, 5, len, 256);
			CHECK(g.fits && g.mk == 1 && g.max_read_len == (uint64_t)K && g.waves == 4 && g.lds_bytes == 16 && g.blocks == 2, "K %d len %llu", K,
			      (unsigned long long)len);
		}
	}
}

// wave_blocks: without a forced value the grid is what it was before the function existed (restated here as it stood); forced 1 and
// 3 with fewer and with more items than wavefronts; never 0 workgroups, never more than the items fill; and strip_geometry passes the
// forced value on
static void grids(void)
{
	static const int cus[] = {1, 8, 256};
	static const uint64_t waves[] = {1, 2, 4};
	for (const int cu : cus)
		for (const uint64_t w : waves) {
			const uint64_t full = w * cu * 32;
			for (const uint64_t items : {(uint64_t)0, (uint64_t)1, w - 1, w, w + 1, 3 * w - 1, 3 * w, 3 * w + 1, full - 1, full, full + 1, 100 * full + 7, ~(uint64_t)0}) {
				uint64_t was = items / w + (items % w != 0);
				const uint64_t cap = (uint64_t)cu * 32;
				if (was > cap) was = cap;
				if (was == 0) was = 1;
				CHECK(wave_blocks(items, w, cu, 0) == was, "%llu items, %llu waves, %d CUs: %u workgroups, %llu before", (unsigned long long)items,
				      (unsigned long long)w, cu, wave_blocks(items, w, cu, 0), (unsigned long long)was);
				for (const uint64_t forced : {(uint64_t)1, (uint64_t)3, (uint64_t)100000}) {
					const uint32_t b = wave_blocks(items, w, cu, forced);
					const uint64_t fill = items / w + (items % w != 0);
					CHECK(b >= 1 && b <= forced && (b == forced || b == (fill ? fill : 1)), "%llu items, %llu waves, forced %llu: %u workgroups",
					      (unsigned long long)items, (unsigned long long)w, (unsigned long long)forced, b);
				}
			}
			// fewer items than the forced workgroups have wavefronts: as many workgroups as the items fill; more: the forced number
			CHECK(wave_blocks(w, w, cu, 1) == 1 && wave_blocks(w - 1, w, cu, 1) == 1 && wave_blocks(1000 * w, w, cu, 1) == 1, "forced 1");
			CHECK(wave_blocks(2 * w, w, cu, 3) == 2 && wave_blocks(2 * w + 1, w, cu, 3) == 3 && wave_blocks(3 * w + 1, w, cu, 3) == 3 &&
			      wave_blocks(1000 * w, w, cu, 3) == 3, "forced 3");
			CHECK(wave_blocks(0, w, cu, 0) == 1 && wave_blocks(0, w, cu, 1) == 1 && wave_blocks(0, w, cu, 3) == 1, "no items");
		}
	// a strip kernel: one wavefront per workgroup at 16 384 k-mers, so forced 1 is a single wavefront for the whole batch
	for (const uint64_t forced : {(uint64_t)1, (uint64_t)3}) {
		const StripGeometry one = strip_geometry(31, 1000, 16000, 256, forced), four = strip_geometry(31, 1000, 150, 256, forced);
		CHECK(one.fits && one.waves == 1 && one.blocks == forced && four.fits && four.waves == 4 && four.blocks == forced, "forced %llu",
		      (unsigned long long)forced);
		CHECK(strip_geometry(31, 2, 150, 256, forced).blocks == 1 && strip_geometry(31, 0, 150, 256, forced).blocks == 1, "forced %llu, two reads",
		      (unsigned long long)forced);
	}
	CHECK(strip_geometry(31, 1000, 150, 256, 0).blocks == 250 && strip_geometry(31, 1000, 150, 256).blocks == 250, "forced 0 is no hook");
}

// nreads + 1 offsets in exactly that much memory: empty reads, reads shorter than K = 31, ordinary ones, and one longer than `longer_than`
static uint64_t *ragged_offsets(std::mt19937_64 &rng, uint64_t nreads, uint64_t longer_than)
{
	uint64_t *offs = (uint64_t *)malloc((nreads + 1) * sizeof(uint64_t));
	CHECK(offs, "malloc");
	const uint64_t giant = rng() % nreads;
	offs[0] = rng() % 40;                                // (a stream need not start at base 0 of its first word)
	for (uint64_t i = 0; i < nreads; i++) {
		const uint64_t kind = rng() % 8;
		uint64_t len = kind == 0 ? 0 : kind == 1 ? rng() % 31 : kind == 2 ? 1 + rng() % 400 : 31 + rng() % 120;
		if (i == giant) len = longer_than + 1 + rng() % 50;
		offs[i + 1] = offs[i] + len;
	}
	return offs;
}

static uint64_t pieces(void)
{
	static const uint64_t reads_caps[] = {1, 2, 7, 777}, bases_caps[] = {64, 1000, 1ULL << 29}, counts[] = {2, 6, 40, 1500};
	std::mt19937_64 rng(20240611);
	uint64_t cut = 0, by_reads = 0, by_bases = 0, lone_giants = 0;
	for (const uint64_t piece_bases : bases_caps)
		for (const uint64_t nreads : counts)
			for (int rep = 0; rep < 3; rep++) {
				uint64_t *offs = ragged_offsets(rng, nreads, piece_bases);
				for (const uint64_t step : {(uint64_t)1, (uint64_t)2})
					for (uint64_t piece_reads : reads_caps) {
						if (step > 1) piece_reads = piece_reads < step ? step : piece_reads - piece_reads % step;     // (as for_each_piece does)
						uint64_t r0 = 0;
						while (r0 < nreads) {
							const ReadPiece p = next_piece(offs, nreads, r0, step, piece_reads, piece_bases, PAD);
							const uint64_t nr = p.r1 - r0;
							CHECK(p.r1 > r0 && p.r1 <= nreads && nr % step == 0, "piece [%llu, %llu) of %llu reads, step %llu", (unsigned long long)r0,
							      (unsigned long long)p.r1, (unsigned long long)nreads, (unsigned long long)step);
							if (nr > step)
								CHECK(nr <= piece_reads && offs[p.r1] - offs[r0] <= piece_bases, "piece [%llu, %llu) breaks a cap: %llu reads, %llu bases",
								      (unsigned long long)r0, (unsigned long long)p.r1, (unsigned long long)piece_reads, (unsigned long long)piece_bases);
							else if (offs[p.r1] - offs[r0] > piece_bases)
								lone_giants++;
							if (p.r1 < nreads) {
								const bool reads_full = nr + step > piece_reads, bases_full = offs[p.r1 + step] - offs[r0] > piece_bases;
								CHECK(reads_full || bases_full, "piece [%llu, %llu) is not maximal", (unsigned long long)r0, (unsigned long long)p.r1);
								by_reads += reads_full;
								by_bases += !reads_full && bases_full;
							}
							uint64_t longest = 0;
							for (uint64_t i = r0; i < p.r1; i++)
								if (offs[i + 1] - offs[i] > longest) longest = offs[i + 1] - offs[i];
							CHECK(p.maxlen == longest, "piece [%llu, %llu): maxlen %llu, the longest read has %llu", (unsigned long long)r0,
							      (unsigned long long)p.r1, (unsigned long long)p.maxlen, (unsigned long long)longest);
							// the words: from the one that holds the first base to the pad behind the one that holds the last
							CHECK(16 * p.w0 <= offs[r0] && offs[r0] - 16 * p.w0 == (offs[r0] & 15), "piece at read %llu: first word %llu", (unsigned long long)r0,
							      (unsigned long long)p.w0);
							CHECK(p.nwords >= PAD && 16 * (p.w0 + p.nwords - PAD) >= offs[p.r1] && 16 * (p.w0 + p.nwords - PAD) < offs[p.r1] + 16,
							      "piece [%llu, %llu): words [%llu, +%llu)", (unsigned long long)r0, (unsigned long long)p.r1, (unsigned long long)p.w0,
							      (unsigned long long)p.nwords);
							r0 = p.r1;
							cut++;
						}
						CHECK(r0 == nreads, "the pieces end at read %llu of %llu", (unsigned long long)r0, (unsigned long long)nreads);
					}
				free(offs);
			}
	// the test saw what it is about: pieces closed by either cap, and reads that are a piece of their own because no cap holds them
	CHECK(by_reads > 100 && by_bases > 100 && lone_giants >= 288, "%llu / %llu / %llu", (unsigned long long)by_reads, (unsigned long long)by_bases,
	      (unsigned long long)lone_giants);
	return cut;
}

static void streams(void)
{
	const uint64_t offs[] = {3, 10, 10, 40, 35, 50, 49};
	StreamCheck s = check_stream(offs, 3, 100, PAD);
	CHECK(s.fault == STREAM_OK && s.longest == 30 && s.need_words == 3 + PAD, "three reads");
	s = check_stream(offs, 6, 100, PAD);
	CHECK(s.fault == STREAM_NOT_MONOTONIC && s.read == 3, "the first of two faults: read %llu", (unsigned long long)s.read);
	// 40 bases end in word 2: three words and the pad, not one fewer
	CHECK(check_stream(offs, 3, 3 + PAD, PAD).fault == STREAM_OK && check_stream(offs, 3, 3 + PAD, 0).need_words == 3, "exactly enough words");
	s = check_stream(offs, 3, 2 + PAD, PAD);
	CHECK(s.fault == STREAM_TOO_SHORT && s.need_words == 3 + PAD, "one word short: needs %llu", (unsigned long long)s.need_words);
	const uint64_t full[] = {0, 32};                     // (a stream that ends on a word boundary takes no further word)
	CHECK(check_stream(full, 1, 2, 0).fault == STREAM_OK && check_stream(full, 1, 1, 0).fault == STREAM_TOO_SHORT, "a word boundary");
	// no reads: no words are needed and offsets is not looked at
	s = check_stream(nullptr, 0, 0, PAD);
	CHECK(s.fault == STREAM_OK && s.need_words == 0 && s.longest == 0, "no reads, no words");
	uint64_t *one = (uint64_t *)malloc(sizeof(uint64_t));
	CHECK(one, "malloc");
	one[0] = 17;
	CHECK(check_stream(one, 0, 0, PAD).fault == STREAM_OK, "no reads behind one offset");
	free(one);
}

int main(void)
{
	geometry();
	grids();
	const uint64_t cut = pieces();
	streams();
	printf("read_plan_check: ok (%llu pieces)\n", (unsigned long long)cut);
	return 0;
}
