// quality_plan_check.cpp -- CPU: what the quality trim decides on the host (csrc/sdt_read_plan.h):
//   * check_quality_params: every refusal of include/sdt_gpu.h, each alone in otherwise valid parameters, the values next to it that
//     pass (phred_offset 0 / 33 / 64 against 1 / 32 / 34 / 63 / 65, cut_q and low_q 93 / 94, max_low_pct 100 / 101), and the order of
//     the refusals;
//   * QUALITY_EE_PPM: every entry t is 10^6 * 10^(-q / 10) rounded to the nearest integer and no tie, by the exact inequality
//     (2 t - 1)^10 10^q <= (2 10^6)^10 < (2 t + 1)^10 10^q in integers of 96 decimal digits kept here; the spot values of the header;
//     quality_of at the offset, below it, at offset + 93 and above;
//   * check_byte_stream: the two faults and what passes;
//   * next_byte_piece: for a few shapes and limits the pieces cover every read exactly once in order, a piece starts at a multiple of 4
//     bytes at most 3 before its first read, ends with its last read, holds one read at least and stays within both limits unless it is
//     a single read; a read longer than a piece is a piece of its own.
// Built with -fsanitize=address,undefined by tests/test_read_quality_host.py.  Prints "quality_plan_check: ok ..." or the first
// violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("quality_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static int checks;

static void parameters(void)
{
	const QualityParams good = {33, 20, 15, 40, 0, 0, 0, 0};
	CHECK(check_quality_params(good) == QUALITY_OK, "the defaults");
	struct { QualityParams p; QualityFault want; } cases[] = {
		{{0, 20, 15, 40, 0, 0, 0, 0}, QUALITY_OK},                 {{64, 20, 15, 40, 0, 0, 0, 0}, QUALITY_OK},
		{{1, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},       {{32, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},
		{{34, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},      {{63, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},
		{{65, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},      {{0xFFFFFFFFu, 20, 15, 40, 0, 0, 0, 0}, QUALITY_PHRED_OFFSET},
		{{33, 93, 15, 40, 0, 0, 0, 0}, QUALITY_OK},                {{33, 94, 15, 40, 0, 0, 0, 0}, QUALITY_CUT_Q},
		{{33, 0, 15, 40, 0, 0, 0, 0}, QUALITY_OK},                 {{33, 0xFFFFFFFFu, 15, 40, 0, 0, 0, 0}, QUALITY_CUT_Q},
		{{33, 20, 93, 40, 0, 0, 0, 0}, QUALITY_OK},                {{33, 20, 94, 40, 0, 0, 0, 0}, QUALITY_LOW_Q},
		{{33, 20, 0, 40, 0, 0, 0, 0}, QUALITY_OK},                 {{33, 20, 0xFFFFFFFFu, 40, 0, 0, 0, 0}, QUALITY_LOW_Q},
		{{33, 20, 15, 100, 0, 0, 0, 0}, QUALITY_OK},               {{33, 20, 15, 101, 0, 0, 0, 0}, QUALITY_MAX_LOW_PCT},
		{{33, 20, 15, 0, 0, 0, 0, 0}, QUALITY_OK},                 {{33, 20, 15, 0xFFFFFFFFu, 0, 0, 0, 0}, QUALITY_MAX_LOW_PCT},
		{{33, 20, 15, 40, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0}, QUALITY_OK},
		{{33, 20, 15, 40, 0, 0, 1, 0}, QUALITY_FLAGS},             {{33, 20, 15, 40, 0, 0, 0x80000000u, 0}, QUALITY_FLAGS},
		{{33, 20, 15, 40, 0, 0, 0, 1}, QUALITY_RESERVED},          {{33, 20, 15, 40, 0, 0, 0, 0xFFFFFFFFu}, QUALITY_RESERVED},
		// the first field of the struct's rules that is refused
		{{1, 94, 94, 101, 0, 0, 1, 1}, QUALITY_PHRED_OFFSET},      {{33, 94, 94, 101, 0, 0, 1, 1}, QUALITY_CUT_Q},
		{{33, 93, 94, 101, 0, 0, 1, 1}, QUALITY_LOW_Q},            {{33, 93, 93, 101, 0, 0, 1, 1}, QUALITY_MAX_LOW_PCT},
		{{33, 93, 93, 100, 0, 0, 1, 1}, QUALITY_FLAGS},            {{33, 93, 93, 100, 0, 0, 0, 1}, QUALITY_RESERVED},
	};
	for (const auto &c : cases) {
		CHECK(check_quality_params(c.p) == c.want, "case %d: %d, %d expected", checks, (int)check_quality_params(c.p), (int)c.want);
		checks++;
	}
}

// ---- whole numbers of up to 24 * 4 decimal digits, least significant group first: just what the inequality needs ----
enum { GROUPS = 24 };
struct Big { uint32_t g[GROUPS]; };                      // base 10 000

static Big big_of(uint64_t v)
{
	Big b;
	memset(&b, 0, sizeof b);
	for (int i = 0; v; i++, v /= 10000) b.g[i] = (uint32_t)(v % 10000);
	return b;
}
static Big big_mul(const Big &x, uint64_t m)             // m < 2^32
{
	Big r;
	uint64_t carry = 0;
	for (int i = 0; i < GROUPS; i++) {
		const uint64_t t = (uint64_t)x.g[i] * m + carry;
		r.g[i] = (uint32_t)(t % 10000);
		carry = t / 10000;
	}
	CHECK(carry == 0, "a number of more than %d digits", 4 * GROUPS);
	return r;
}
static int big_cmp(const Big &x, const Big &y)
{
	for (int i = GROUPS - 1; i >= 0; i--)
		if (x.g[i] != y.g[i]) return x.g[i] < y.g[i] ? -1 : 1;
	return 0;
}
static Big pow10_times(uint64_t v, unsigned q)           // v^10 * 10^q
{
	Big b = big_of(1);
	for (int i = 0; i < 10; i++) b = big_mul(b, v);
	for (unsigned i = 0; i < q; i++) b = big_mul(b, 10);
	return b;
}

static void table(void)
{
	const Big top = pow10_times(2000000, 0);             // (2 * 10^6)^10: 64 digits; the other side has 94 at most (t = 0, q = 93)
	for (unsigned q = 0; q <= QUALITY_MAX_Q; q++) {
		const uint64_t t = QUALITY_EE_PPM[q];
		// t - 1/2 <= 10^6 10^(-q / 10) < t + 1/2, both sides to the tenth power and times 10^q; strict on the left too: no tie
		CHECK(big_cmp(top, pow10_times(2 * t + 1, q)) < 0, "e[%u] = %llu is too small", q, (unsigned long long)t);
		if (t) CHECK(big_cmp(pow10_times(2 * t - 1, q), top) < 0, "e[%u] = %llu is too large, or a tie", q, (unsigned long long)t);
		CHECK(q == 0 || t <= QUALITY_EE_PPM[q - 1], "e[%u] rises", q);
		checks++;
	}
	static_assert(QUALITY_EE_PPM[0] == 1000000 && QUALITY_EE_PPM[1] == 794328 && QUALITY_EE_PPM[3] == 501187 && QUALITY_EE_PPM[20] == 10000 &&
	                  QUALITY_EE_PPM[30] == 1000 && QUALITY_EE_PPM[60] == 1 && QUALITY_EE_PPM[63] == 1 && QUALITY_EE_PPM[64] == 0 && QUALITY_EE_PPM[93] == 0,
	              "the spot values of include/sdt_gpu.h");
	static_assert(sizeof QUALITY_EE_PPM / sizeof QUALITY_EE_PPM[0] == 94, "94 entries");
	static_assert(quality_of(33, 33) == 0 && quality_of(32, 33) == 0 && quality_of(0, 33) == 0 && quality_of(34, 33) == 1 && quality_of(126, 33) == 93 &&
	                  quality_of(127, 33) == 93 && quality_of(255, 33) == 93 && quality_of(255, 0) == 93 && quality_of(93, 0) == 93 && quality_of(92, 0) == 92 &&
	                  quality_of(63, 64) == 0 && quality_of(104, 64) == 40 && quality_of(157, 64) == 93 && quality_of(158, 64) == 93,
	              "the quality a byte says");
}

static void streams(void)
{
	const uint64_t up[] = {5, 5, 9, 20}, down[] = {0, 7, 6, 9};
	StreamCheck s = check_byte_stream(up, 3, 20);
	CHECK(s.fault == STREAM_OK && s.need_words == 20 && s.longest == 11, "a stream that fits exactly");
	s = check_byte_stream(up, 3, 19);
	CHECK(s.fault == STREAM_TOO_SHORT && s.need_words == 20, "one byte short");
	s = check_byte_stream(down, 3, 100);
	CHECK(s.fault == STREAM_NOT_MONOTONIC && s.read == 1, "read 1 ends before it starts");
	s = check_byte_stream(NULL, 0, 0);
	CHECK(s.fault == STREAM_OK && s.need_words == 0, "no reads: the offsets are not looked at");
	checks += 4;
}

// the pieces of a stream of n reads under the two limits: a cover of every read, in order, in exactly n + 1 offsets
static void pieces_of(const uint64_t *lens, uint64_t n, uint64_t first, uint64_t piece_reads, uint64_t piece_bytes)
{
	uint64_t *offs = (uint64_t *)malloc((n + 1) * sizeof(uint64_t));
	offs[0] = first;
	for (uint64_t i = 0; i < n; i++) offs[i + 1] = offs[i] + lens[i];
	unsigned *seen = (unsigned *)calloc(n ? n : 1, sizeof(unsigned));
	uint64_t r0 = 0, npieces = 0;
	while (r0 < n) {
		const BytePiece p = next_byte_piece(offs, n, r0, piece_reads, piece_bytes);
		CHECK(p.r1 > r0 && p.r1 <= n, "piece at read %llu ends at %llu", (unsigned long long)r0, (unsigned long long)p.r1);
		CHECK((p.b0 & 3) == 0 && p.b0 <= offs[r0] && offs[r0] - p.b0 < 4, "piece at read %llu starts at byte %llu", (unsigned long long)r0, (unsigned long long)p.b0);
		CHECK(p.b0 + p.nbytes == offs[p.r1], "piece at read %llu: %llu bytes", (unsigned long long)r0, (unsigned long long)p.nbytes);
		const uint64_t nr = p.r1 - r0, own = offs[p.r1] - offs[r0];
		CHECK(nr == 1 || (nr <= (piece_reads ? piece_reads : 1) && own <= piece_bytes), "piece at read %llu: %llu reads, %llu bytes", (unsigned long long)r0,
		      (unsigned long long)nr, (unsigned long long)own);
		// greedy: the next read would not have fitted
		if (p.r1 < n && nr < (piece_reads ? piece_reads : 1)) CHECK(offs[p.r1 + 1] - offs[r0] > piece_bytes, "piece at read %llu stops early", (unsigned long long)r0);
		for (uint64_t i = r0; i < p.r1; i++) seen[i]++;
		r0 = p.r1;
		npieces++;
	}
	for (uint64_t i = 0; i < n; i++) CHECK(seen[i] == 1, "read %llu is in %u pieces", (unsigned long long)i, seen[i]);
	CHECK(n == 0 || npieces >= 1, "no piece");
	free(seen);
	free(offs);
	checks++;
}

static void pieces(void)
{
	const uint64_t ragged[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 0, 0, 255, 256, 257, 5000, 3, 0, 150, 150, 150, 1, 0};
	const uint64_t nragged = sizeof ragged / sizeof ragged[0];
	uint64_t same[40];
	for (int i = 0; i < 40; i++) same[i] = 150;
	const uint64_t cap_reads[] = {1, 2, 7, 1000, 0}, cap_bytes[] = {0, 1, 149, 150, 151, 300, 449, 4999, 5000, 1ULL << 29};
	for (uint64_t first = 0; first < 9; first++)
		for (uint64_t reads : cap_reads)
			for (uint64_t bytes : cap_bytes) {
				pieces_of(ragged, nragged, first, reads, bytes);                 // (the read of 5 000 bytes is longer than most of these pieces)
				pieces_of(same, 40, first, reads, bytes);
				pieces_of(ragged, 1, first, reads, bytes);
				pieces_of(ragged + 14, 1, first, reads, bytes);
				pieces_of(ragged, 0, first, reads, bytes);
			}
	// a read longer than a piece is a piece of its own, whatever stands around it
	const uint64_t offs[] = {6, 10, 5010, 5013};
	BytePiece p = next_byte_piece(offs, 3, 0, 7, 100);
	CHECK(p.r1 == 1 && p.b0 == 4 && p.nbytes == 6, "the read before the long one");
	p = next_byte_piece(offs, 3, 1, 7, 100);
	CHECK(p.r1 == 2 && p.b0 == 8 && p.nbytes == 5002, "the long read alone");
	p = next_byte_piece(offs, 3, 2, 7, 100);
	CHECK(p.r1 == 3 && p.b0 == 5008 && p.nbytes == 5, "the read behind it");
}

int main(void)
{
	parameters();
	table();
	streams();
	pieces();
	printf("quality_plan_check: ok (%d checks)\n", checks);
	return 0;
}
