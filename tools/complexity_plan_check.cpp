// complexity_plan_check.cpp -- CPU: what the low-complexity filter decides on the host (csrc/sdt_read_plan.h):
//   * check_complexity_params: every refusal of include/sdt_gpu.h, each alone in otherwise valid parameters, the values next to it that
//     pass (max_score_pct 0 / 1 / 100 / 101, max_low_pct 100 / 101, max_low_pct 0 / 1 under SDT_COMPLEXITY_TRIM), and the order of the
//     refusals;
//   * complexity_windows and the window bounds: for every L <= 300 they are the windows of the rule as written (W = max(1,
//     ceil(L / 32) - 1), window j = [32 j, min(32 j + 64, L))), and a walk over every base finds that every base is in a window, that
//     bases [32 k, 32 k + 32) are covered by the windows k - 1 and k that exist and by no other (what the kernel's sweep relies on),
//     that the last window ends at L and that it has more than 32 bases unless it is the only one.
// Built with -fsanitize=address,undefined by tests/test_read_complexity_host.py.  Prints "complexity_plan_check: ok ..." or the first
// violation.
#include <stdio.h>
#include <stdlib.h>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("complexity_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static int checks;

static void parameters(void)
{
	const ComplexityParams good = {10, 50, 0, 0};
	CHECK(check_complexity_params(good) == COMPLEXITY_OK, "the defaults");
	struct { ComplexityParams p; ComplexityFault want; } cases[] = {
		{{10, 50, 0, 2}, COMPLEXITY_FLAGS},                  {{10, 0, 0, 3}, COMPLEXITY_FLAGS},               {{10, 50, 0, 0x80000000u}, COMPLEXITY_FLAGS},
		{{10, 0, 0, COMPLEXITY_TRIM}, COMPLEXITY_OK},
		{{0, 50, 0, 0}, COMPLEXITY_MAX_SCORE_PCT},           {{1, 50, 0, 0}, COMPLEXITY_OK},
		{{101, 50, 0, 0}, COMPLEXITY_MAX_SCORE_PCT},         {{100, 50, 0, 0}, COMPLEXITY_OK},                {{0xFFFFFFFFu, 50, 0, 0}, COMPLEXITY_MAX_SCORE_PCT},
		{{10, 101, 0, 0}, COMPLEXITY_MAX_LOW_PCT},           {{10, 100, 0, 0}, COMPLEXITY_OK},                {{10, 0, 0, 0}, COMPLEXITY_OK},
		{{10, 0xFFFFFFFFu, 0, 0}, COMPLEXITY_MAX_LOW_PCT},
		{{10, 1, 0, COMPLEXITY_TRIM}, COMPLEXITY_TRIM_MAX_LOW_PCT}, {{10, 100, 0, COMPLEXITY_TRIM}, COMPLEXITY_TRIM_MAX_LOW_PCT},
		{{100, 100, 0xFFFFFFFFu, 0}, COMPLEXITY_OK},         {{1, 0, 0xFFFFFFFFu, COMPLEXITY_TRIM}, COMPLEXITY_OK},
		// the first field of the struct's rules that is refused
		{{0, 101, 0, 2}, COMPLEXITY_FLAGS},                  {{0, 101, 0, COMPLEXITY_TRIM}, COMPLEXITY_MAX_SCORE_PCT},
		{{10, 101, 0, COMPLEXITY_TRIM}, COMPLEXITY_MAX_LOW_PCT},
	};
	for (const auto &c : cases) {
		CHECK(check_complexity_params(c.p) == c.want, "case %d: %d, %d expected", checks, (int)check_complexity_params(c.p), (int)c.want);
		checks++;
	}
}

static void windows(void)
{
	CHECK(complexity_windows(0) == 0, "a read of no bases has no window");
	for (uint64_t L = 1; L <= 300; L++) {
		const uint64_t W = complexity_windows(L), ceil32 = (L + 31) / 32;
		CHECK(W == (ceil32 - 1 > 1 ? ceil32 - 1 : 1), "L %llu: %llu windows", (unsigned long long)L, (unsigned long long)W);
		// the cover of every base, in an array of exactly L counters, and the first and the last window that holds it
		unsigned *cover = (unsigned *)calloc(L, sizeof(unsigned));
		uint64_t *first = (uint64_t *)malloc(L * sizeof(uint64_t)), *last = (uint64_t *)malloc(L * sizeof(uint64_t));
		for (uint64_t j = 0; j < W; j++) {
			const uint64_t b = complexity_window_begin(j), e = complexity_window_end(j, L);
			CHECK(b == 32 * j && e == (32 * j + 64 < L ? 32 * j + 64 : L) && b < e && e <= L, "L %llu window %llu = [%llu, %llu)", (unsigned long long)L,
			      (unsigned long long)j, (unsigned long long)b, (unsigned long long)e);
			CHECK(W == 1 || j + 1 < W || e - b > 32, "L %llu: the last window has %llu bases", (unsigned long long)L, (unsigned long long)(e - b));
			CHECK(j + 1 < W ? e - b == 64 : e == L, "L %llu window %llu ends at %llu", (unsigned long long)L, (unsigned long long)j, (unsigned long long)e);
			for (uint64_t i = b; i < e; i++) {
				if (!cover[i]++) first[i] = j;
				last[i] = j;
			}
		}
		for (uint64_t i = 0; i < L; i++) {
			const uint64_t k = i / 32, lo = k ? k - 1 : 0, hi = k < W ? k : W - 1;
			CHECK(cover[i] >= 1 && first[i] == lo && last[i] == hi && cover[i] == hi - lo + 1, "L %llu base %llu: %u windows, %llu to %llu",
			      (unsigned long long)L, (unsigned long long)i, cover[i], (unsigned long long)first[i], (unsigned long long)last[i]);
		}
		free(cover); free(first); free(last);
		checks++;
	}
	static_assert(complexity_windows(150) == 4 && complexity_window_begin(3) == 96 && complexity_window_end(3, 150) == 150, "[0,64) [32,96) [64,128) [96,150)");
	static_assert(complexity_windows(64) == 1 && complexity_windows(65) == 2 && complexity_windows(33) == 1 && complexity_windows(1) == 1, "the rule's examples");
	CHECK(complexity_windows(0xFFFFFFFFULL) == 0x7FFFFFFULL && complexity_window_end(0x7FFFFFEULL, 0xFFFFFFFFULL) == 0xFFFFFFFFULL, "no 32-bit wrap");
}

int main(void)
{
	parameters();
	windows();
	printf("complexity_plan_check: ok (%d checks)\n", checks);
	return 0;
}
