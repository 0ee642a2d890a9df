// merge_plan_check.cpp -- CPU: what the merge of overlapping mates decides on the host (csrc/sdt_read_plan.h):
//   * check_merge_params: every refusal of include/sdt_gpu.h, each alone in otherwise valid parameters, the values next to it that pass
//     (max_len == max(min_len, 1), a phred_offset that is looked at only with qualities, an odd and an even number of dense reads),
//     and the order of the refusals;
//   * merge_decide: for every La, Lb <= 10 and every pair of inserts up to La + Lb + 1 the decision against the four lines of the rule
//     written out, under three (min_len, max_len); and for every mergeable (La, Lb, F) of the grid of mate lengths
//     0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 (825 combinations and more) a walk over every position: each p < F is covered by a or
//     by b', at least one by both unless a mate has no bases, and b' is never indexed outside [0, Lb);
//   * merge_chunks: the 64-bit values of 32 bases a merged read takes.
// Built with -fsanitize=address,undefined by tests/test_read_merge_host.py.  Prints "merge_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("merge_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static int checks;

static void parameters(void)
{
	const MergeParams good = {0, 0, 33, 0};
	CHECK(check_merge_params(good, false, 0) == MERGE_OK && check_merge_params(good, true, 600) == MERGE_OK, "the defaults");
	struct { MergeParams p; bool quals; uint64_t dense; MergeFault want; } cases[] = {
		{{0, 0, 33, 1}, false, 0, MERGE_FLAGS},          {{0, 0, 33, 0x80000000u}, true, 2, MERGE_FLAGS},
		{{30, 29, 33, 0}, false, 0, MERGE_MAX_LEN},      {{30, 30, 33, 0}, false, 0, MERGE_OK},     {{30, 0, 33, 0}, false, 0, MERGE_OK},
		{{0, 1, 33, 0}, false, 0, MERGE_OK},             {{1, 1, 33, 0}, false, 0, MERGE_OK},       {{2, 1, 33, 0}, false, 0, MERGE_MAX_LEN},
		{{0xFFFFFFFFu, 0xFFFFFFFFu, 33, 0}, false, 0, MERGE_OK},
		{{0, 0, 32, 0}, true, 0, MERGE_PHRED_OFFSET},    {{0, 0, 32, 0}, false, 0, MERGE_OK},       {{0, 0, 0, 0}, true, 0, MERGE_OK},
		{{0, 0, 64, 0}, true, 0, MERGE_OK},              {{0, 0, 65, 0}, true, 0, MERGE_PHRED_OFFSET},
		{{0, 0, 33, 0}, false, 1, MERGE_ODD_READS},      {{0, 0, 33, 0}, false, 2, MERGE_OK},
		{{0, 0, 33, 0}, true, 0xFFFFFFFFFFFFFFFFULL, MERGE_ODD_READS}, {{0, 0, 33, 0}, true, 0xFFFFFFFFFFFFFFFEULL, MERGE_OK},
		// the first line of the rules that is refused
		{{5, 4, 7, 1}, true, 3, MERGE_FLAGS},            {{5, 4, 7, 0}, true, 3, MERGE_MAX_LEN},    {{5, 5, 7, 0}, true, 3, MERGE_PHRED_OFFSET},
		{{5, 5, 33, 0}, true, 3, MERGE_ODD_READS},
	};
	for (const auto &c : cases) {
		CHECK(check_merge_params(c.p, c.quals, c.dense) == c.want, "case %d: %d, %d expected", checks, (int)check_merge_params(c.p, c.quals, c.dense),
		      (int)c.want);
		checks++;
	}
}

// the four lines of MERGEABLE in include/sdt_gpu.h, written out
static int64_t by_the_rule(uint64_t La, uint64_t Lb, uint32_t Fa, uint32_t Fb, uint32_t min_len, uint32_t max_len)
{
	const bool line1 = Fa == Fb, line2 = Fa >= 1 && Fa < La + Lb;
	if (line1 && Fa == 0) return 0;                          // a pair without overlap
	if (!line1 || !line2) return MERGE_INCONSISTENT;
	const bool line3 = Fa >= (min_len > 1 ? min_len : 1u), line4 = max_len == 0 || Fa <= max_len;
	return line3 && line4 ? (int64_t)Fa : 0;
}

static void decisions(void)
{
	const uint32_t limits[3][2] = {{0, 0}, {3, 0}, {2, 7}};
	for (uint64_t La = 0; La <= 10; La++)
		for (uint64_t Lb = 0; Lb <= 10; Lb++)
			for (uint32_t Fa = 0; Fa <= La + Lb + 1; Fa++)
				for (uint32_t Fb = 0; Fb <= La + Lb + 1; Fb++)
					for (const auto &l : limits) {
						const int64_t got = merge_decide(La, Lb, Fa, Fb, l[0], l[1]), want = by_the_rule(La, Lb, Fa, Fb, l[0], l[1]);
						CHECK(got == want, "La %llu Lb %llu Fa %u Fb %u min_len %u max_len %u: %lld, %lld by the rule", (unsigned long long)La,
						      (unsigned long long)Lb, Fa, Fb, l[0], l[1], (long long)got, (long long)want);
						checks++;
					}
	static_assert(merge_decide(150, 150, 200, 200, 0, 0) == 200 && merge_decide(150, 150, 300, 300, 0, 0) == MERGE_INCONSISTENT &&
	                  merge_decide(150, 150, 299, 299, 0, 0) == 299 && merge_decide(150, 150, 200, 201, 0, 0) == MERGE_INCONSISTENT &&
	                  merge_decide(150, 150, 0, 0, 0, 0) == 0 && merge_decide(150, 150, 200, 200, 201, 0) == 0 &&
	                  merge_decide(150, 150, 200, 200, 0, 199) == 0 && merge_decide(150, 150, 200, 200, 200, 200) == 200,
	              "a pair of 150-base reads");
	CHECK(merge_decide(0xFFFFFFFFULL, 0xFFFFFFFFULL, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0) == 0xFFFFFFFFLL, "no 32-bit wrap");
	CHECK(merge_decide(0x100000000ULL, 0x100000000ULL, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0) == 0xFFFFFFFFLL, "mates past 2^32 bases");
}

static void cover(void)
{
	const uint64_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65};
	int combos = 0;
	for (uint64_t La : lens)
		for (uint64_t Lb : lens)
			for (uint64_t F = 1; F <= La + Lb; F++) {
				const int64_t m = merge_decide(La, Lb, (uint32_t)F, (uint32_t)F, 0, 0);
				if (F == La + Lb) {
					CHECK(m == MERGE_INCONSISTENT, "La %llu Lb %llu: F = La + Lb has no column", (unsigned long long)La, (unsigned long long)Lb);
					continue;
				}
				CHECK(m == (int64_t)F, "La %llu Lb %llu F %llu", (unsigned long long)La, (unsigned long long)Lb, (unsigned long long)F);
				const long long d = (long long)F - (long long)Lb;
				uint64_t both = 0;
				for (uint64_t p = 0; p < F; p++) {
					const bool in_a = p < La, in_b = (long long)p >= d;
					if (in_b) CHECK((long long)p - d < (long long)Lb, "b' is indexed past its end at %llu", (unsigned long long)p);
					CHECK(in_a || in_b, "La %llu Lb %llu F %llu: position %llu is covered by neither mate", (unsigned long long)La,
					      (unsigned long long)Lb, (unsigned long long)F, (unsigned long long)p);
					both += in_a && in_b;
				}
				CHECK(both >= 1 || !La || !Lb, "La %llu Lb %llu F %llu: no column", (unsigned long long)La, (unsigned long long)Lb, (unsigned long long)F);
				CHECK(both == (F < La ? F : La) - (d > 0 ? (uint64_t)d : 0), "the columns are those of the shift");
				combos++;
				checks++;
			}
	CHECK(combos >= 825, "%d combinations", combos);
	static_assert(merge_chunks(0) == 0 && merge_chunks(1) == 1 && merge_chunks(32) == 1 && merge_chunks(33) == 2 && merge_chunks(2048) == 64 &&
	                  merge_chunks(2049) == 65 && merge_chunks(0xFFFFFFFFULL) == 0x8000000ULL,
	              "one 64-bit value per 32 bases, rounded up");
}

int main(void)
{
	parameters();
	decisions();
	cover();
	printf("merge_plan_check: ok (%d checks)\n", checks);
	return 0;
}
