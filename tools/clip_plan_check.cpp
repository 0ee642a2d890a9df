// clip_plan_check.cpp -- CPU: what the adapter and tail clipping decides on the host (csrc/sdt_read_plan.h):
//   * check_clip_params: every refusal of include/sdt_gpu.h, each alone in otherwise valid parameters, and the values next to it
//     that pass;
//   * check_adapter_set: every refusal with the index of the adapter, in arrays malloc'ed to exactly n + 1 offsets and n ends, at
//     the boundaries 128 / 129 bases and 256 / 257 adapters;
//   * split_adapter: on random adapters at every start base of a word, chunk c of a 3' adapter holds bases [32 c, 32 c + 32) from
//     the top, chunk c of a 5' adapter bases [m - 32 c - 32, m - 32 c) from the bottom, and nothing else is set.
// Built with -fsanitize=address,undefined by tests/test_read_clip_host.py.  Prints "clip_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("clip_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static int checks;

static void parameters(void)
{
	const ClipParams good = {5, 10, 0, 10, 20, 1, 4, 0};
	CHECK(check_clip_params(good) == CLIP_OK, "the defaults");
	struct { ClipParams p; ClipFault want; } cases[] = {
		{{5, 10, 0, 10, 20, 1, 4, 1}, CLIP_FLAGS},        {{5, 10, 0, 10, 20, 1, 4, 0x80000000u}, CLIP_FLAGS},
		{{0, 10, 0, 10, 20, 1, 4, 0}, CLIP_MIN_OVERLAP},  {{1, 10, 0, 10, 20, 1, 4, 0}, CLIP_OK},
		{{5, 101, 0, 10, 20, 1, 4, 0}, CLIP_MAX_ERR_PCT}, {{5, 100, 0, 10, 20, 1, 4, 0}, CLIP_OK},  {{5, 0, 0, 10, 20, 1, 4, 0}, CLIP_OK},
		{{5, 10, 0, 10, 101, 1, 4, 0}, CLIP_TAIL_ERR_PCT}, {{5, 10, 0, 10, 100, 1, 4, 0}, CLIP_OK},
		{{5, 10, 0, 10, 20, 16, 4, 0}, CLIP_TAIL3_BASES}, {{5, 10, 0, 10, 20, 15, 4, 0}, CLIP_OK},
		{{5, 10, 0, 10, 20, 1, 16, 0}, CLIP_TAIL5_BASES}, {{5, 10, 0, 10, 20, 1, 15, 0}, CLIP_OK},
		{{5, 10, 0, 0, 20, 1, 0, 0}, CLIP_MIN_TAIL},      {{5, 10, 0, 0, 20, 0, 8, 0}, CLIP_MIN_TAIL},  {{5, 10, 0, 0, 20, 0, 0, 0}, CLIP_OK},
		{{5, 10, 0xFFFFFFFFu, 0xFFFFFFFFu, 20, 1, 4, 0}, CLIP_OK},
	};
	for (const auto &c : cases) {
		CHECK(check_clip_params(c.p) == c.want, "case %d: %d, %d expected", checks, (int)check_clip_params(c.p), (int)c.want);
		checks++;
	}
}

// the set of the given lengths and ends in arrays of exactly the sizes the check may read
static ClipFault set_fault(const std::vector<uint64_t> &lens, const std::vector<uint8_t> &ends, uint32_t min_overlap, uint64_t *index, int64_t dent = -1)
{
	const uint64_t n = lens.size();
	uint64_t *offs = (uint64_t *)malloc((n + 1) * sizeof(uint64_t));
	uint8_t *e = (uint8_t *)malloc(n ? n : 1);
	offs[0] = 3;
	for (uint64_t i = 0; i < n; i++) offs[i + 1] = offs[i] + lens[i];
	if (dent >= 0) offs[dent + 1] = offs[dent] - 1;          // adapter `dent` ends before it starts
	if (n) memcpy(e, ends.data(), n);
	const ClipFault f = check_adapter_set(offs, e, n, min_overlap, index);
	free(offs);
	free(e);
	checks++;
	return f;
}

static void adapter_sets(void)
{
	uint64_t at = 77;
	CHECK(set_fault({}, {}, 5, &at) == CLIP_OK && at == 0, "no adapters");
	CHECK(set_fault({33, 58, 128, 5}, {0, 0, 1, 1}, 5, &at) == CLIP_OK && at == 4, "a good set");
	CHECK(set_fault({33, 129, 20}, {0, 0, 0}, 5, &at) == CLIP_ADAPTER_LONG && at == 1, "129 bases");
	CHECK(set_fault({33, 128, 20}, {0, 0, 0}, 5, &at) == CLIP_OK, "128 bases");
	CHECK(set_fault({33, 20, 0}, {0, 0, 0}, 5, &at) == CLIP_ADAPTER_EMPTY && at == 2, "0 bases");
	CHECK(set_fault({4, 20}, {0, 0}, 5, &at) == CLIP_ADAPTER_SHORT && at == 0, "shorter than min_overlap");
	CHECK(set_fault({5, 20}, {0, 0}, 5, &at) == CLIP_OK, "as long as min_overlap");
	CHECK(set_fault({1}, {1}, 1, &at) == CLIP_OK, "one base under min_overlap 1");
	CHECK(set_fault({33, 20, 40}, {0, 1, 2}, 5, &at) == CLIP_ADAPTER_END && at == 2, "ends = 2");
	CHECK(set_fault({33, 20, 40}, {0, 255, 0}, 5, &at) == CLIP_ADAPTER_END && at == 1, "ends = 255");
	CHECK(set_fault({33, 20, 40}, {0, 1, 0}, 5, &at, 1) == CLIP_OFFSETS && at == 1, "offsets descend");
	CHECK(set_fault(std::vector<uint64_t>(256, 31), std::vector<uint8_t>(256, 1), 5, &at) == CLIP_OK && at == 256, "256 adapters");
	CHECK(set_fault(std::vector<uint64_t>(257, 31), std::vector<uint8_t>(257, 1), 5, &at) == CLIP_TOO_MANY && at == 257, "257 adapters");
	// too many comes first: nothing of the arrays is read
	uint64_t none = 0;
	CHECK(check_adapter_set(&none, nullptr, 1000, 5, &at) == CLIP_TOO_MANY, "1000 adapters");
}

static void splits(void)
{
	std::mt19937_64 rng(20241018);
	for (uint32_t m : {1u, 2u, 15u, 16u, 17u, 31u, 32u, 33u, 63u, 64u, 65u, 96u, 127u, 128u})
		for (uint32_t lead = 0; lead < 16; lead++)
			for (uint8_t end = 0; end < 2; end++) {
				std::vector<uint8_t> bases(m);
				for (auto &b : bases) b = (uint8_t)(rng() & 3);
				const uint64_t total = lead + m, nw = (total + 15) >> 4;
				uint32_t *words = (uint32_t *)calloc(nw, sizeof(uint32_t));           // exactly the words that hold a base
				for (uint64_t k = 0; k < lead; k++) words[k >> 4] |= 3u << (30 - 2 * (k & 15));      // filler in front
				for (uint32_t k = 0; k < m; k++) words[(lead + k) >> 4] |= (uint32_t)bases[k] << (30 - 2 * ((lead + k) & 15));
				const uint64_t offs[3] = {0, lead, total};
				const uint8_t ends[2] = {0, end};
				const ClipAdapter a = split_adapter(words, offs, ends, 1);
				free(words);
				CHECK(a.m == m && a.id == 1, "m = %u", m);
				uint64_t want[CLIP_ADAPTER_CHUNKS] = {0, 0, 0, 0};
				for (uint32_t k = 0; k < m; k++) {
					if (end == 0) want[k / 32] |= (uint64_t)bases[k] << (62 - 2 * (k % 32));
					else want[(m - 1 - k) / 32] |= (uint64_t)bases[k] << (2 * ((m - 1 - k) % 32));
				}
				for (uint32_t c = 0; c < CLIP_ADAPTER_CHUNKS; c++)
					CHECK(a.chunk[c] == want[c], "m = %u lead = %u end = %u chunk %u: %016llx, %016llx expected", m, lead, end, c,
					      (unsigned long long)a.chunk[c], (unsigned long long)want[c]);
				checks++;
			}
}

int main(void)
{
	parameters();
	adapter_sets();
	splits();
	printf("clip_plan_check: ok (%d checks)\n", checks);
	return 0;
}
