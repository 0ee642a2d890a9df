// overlap_plan_check.cpp -- CPU: what the mate overlap decides on the host (csrc/sdt_read_plan.h):
//   * check_overlap_params: every refusal of include/sdt_gpu.h, each alone in otherwise valid parameters, the values next to it that
//     pass (max_err_pct 100 / 101, min_overlap 0 / 1, an odd and an even number of dense reads), and the order of the refusals;
//   * check_pair_ranges: the pair ranges that the kept form refuses, in an array malloc'ed to exactly 2 n words;
//   * overlap_shifts: for every La, Lb <= 40 and min_overlap <= 12 the shifts the kernel tries, d_first = min_overlap - Lb onwards,
//     are exactly the shifts of a walk over every d in (-Lb, La) whose columns number min_overlap or more.
// Built with -fsanitize=address,undefined by tests/test_read_overlap_host.py.  Prints "overlap_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("overlap_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static int checks;

static void parameters(void)
{
	const OverlapParams good = {30, 10, 0, 0};
	CHECK(check_overlap_params(good, 0) == OVERLAP_OK && check_overlap_params(good, 600) == OVERLAP_OK, "the defaults");
	struct { OverlapParams p; uint64_t dense; OverlapFault want; } cases[] = {
		{{30, 10, 0, 1}, 0, OVERLAP_FLAGS},            {{30, 10, 0, 0x80000000u}, 2, OVERLAP_FLAGS},
		{{0, 10, 0, 0}, 0, OVERLAP_MIN_OVERLAP},       {{1, 10, 0, 0}, 0, OVERLAP_OK},
		{{30, 101, 0, 0}, 0, OVERLAP_MAX_ERR_PCT},     {{30, 100, 0, 0}, 0, OVERLAP_OK},          {{30, 0, 0, 0}, 0, OVERLAP_OK},
		{{30, 0xFFFFFFFFu, 0, 0}, 4, OVERLAP_MAX_ERR_PCT},
		{{30, 10, 0, 0}, 1, OVERLAP_ODD_READS},        {{30, 10, 0, 0}, 2, OVERLAP_OK},
		{{30, 10, 0, 0}, 0xFFFFFFFFFFFFFFFFULL, OVERLAP_ODD_READS}, {{30, 10, 0, 0}, 0xFFFFFFFFFFFFFFFEULL, OVERLAP_OK},
		{{0xFFFFFFFFu, 100, 0xFFFFFFFFu, 0}, 0, OVERLAP_OK},
		// the first field of the struct's rules that is refused
		{{0, 101, 0, 1}, 3, OVERLAP_FLAGS},            {{0, 101, 0, 0}, 3, OVERLAP_MIN_OVERLAP},  {{1, 101, 0, 0}, 3, OVERLAP_MAX_ERR_PCT},
	};
	for (const auto &c : cases) {
		CHECK(check_overlap_params(c.p, c.dense) == c.want, "case %d: %d, %d expected", checks, (int)check_overlap_params(c.p, c.dense), (int)c.want);
		checks++;
	}
}

static void pair_ranges(void)
{
	struct { uint64_t v[6]; uint64_t n; PairRangeFault want; uint64_t at; } cases[] = {
		{{0, 10, 10, 20, 30, 30}, 3, PAIR_RANGES_OK, 3},
		{{3, 9, 0, 0, 0, 0}, 1, PAIR_RANGES_OK, 1},
		{{0, 10, 12, 15, 0, 0}, 2, PAIR_RANGE_NOT_PAIRS, 1},
		{{8, 4, 0, 0, 0, 0}, 1, PAIR_RANGE_NOT_PAIRS, 0},
		{{0, 10, 8, 12, 0, 0}, 2, PAIR_RANGE_OVERLAPS, 1},
		{{0, 0, 0, 0, 0, 0}, 0, PAIR_RANGES_OK, 0},
	};
	for (const auto &c : cases) {
		uint64_t *exact = (uint64_t *)malloc(c.n ? 2 * c.n * sizeof(uint64_t) : 1);
		memcpy(exact, c.v, 2 * c.n * sizeof(uint64_t));
		PairRangeFault fault;
		const uint64_t at = check_pair_ranges(c.n ? exact : nullptr, c.n, &fault);
		free(exact);
		CHECK(fault == c.want && at == c.at, "case %d: fault %d at %llu", checks, (int)fault, (unsigned long long)at);
		checks++;
	}
}

static void shifts(void)
{
	for (uint64_t La = 0; La <= 40; La++)
		for (uint64_t Lb = 0; Lb <= 40; Lb++)
			for (uint32_t mo = 1; mo <= 12; mo++) {
				// a walk over every shift of the rule
				long long first = 0, last = 0;
				uint64_t n = 0;
				for (long long d = 1 - (long long)Lb; d < (long long)La; d++) {
					const long long lo = d > 0 ? d : 0, hi = d + (long long)Lb < (long long)La ? d + (long long)Lb : (long long)La;
					if (hi - lo >= (long long)mo) {
						if (!n) first = d;
						CHECK(!n || d == last + 1, "La %llu Lb %llu min_overlap %u: the shifts are not consecutive at %lld", (unsigned long long)La,
						      (unsigned long long)Lb, mo, d);
						last = d;
						n++;
					}
				}
				CHECK(overlap_shifts(La, Lb, mo) == n, "La %llu Lb %llu min_overlap %u: %llu shifts, %llu by the walk", (unsigned long long)La,
				      (unsigned long long)Lb, mo, (unsigned long long)overlap_shifts(La, Lb, mo), (unsigned long long)n);
				CHECK(!n || (first == (long long)mo - (long long)Lb && last == (long long)La - (long long)mo), "La %llu Lb %llu min_overlap %u: [%lld, %lld]",
				      (unsigned long long)La, (unsigned long long)Lb, mo, first, last);
				checks++;
			}
	static_assert(overlap_shifts(150, 150, 30) == 241, "241 shifts, four steps of 64, for a pair of 150-base reads under the default");
	CHECK(overlap_shifts(0xFFFFFFFFULL, 0xFFFFFFFFULL, 1) == 2 * 0xFFFFFFFFULL - 1, "no 32-bit wrap");
	CHECK(overlap_shifts(10, 0xFFFFFFFFFFULL, 0xFFFFFFFFu) == 0, "a mate shorter than min_overlap");
}

int main(void)
{
	parameters();
	pair_ranges();
	shifts();
	printf("overlap_plan_check: ok (%d checks)\n", checks);
	return 0;
}
