// dedup_plan_check.cpp -- CPU: what the duplicate filter and the kept-form unit list decide on the host (csrc/sdt_read_plan.h):
//   * dedup_table_slots: a power of two, at least 2 x units (load <= 1/2), less than 4 x units beyond one unit;
//   * check_pair_ranges: the first range that runs backwards, holds half a pair or starts before its predecessor ends;
//   * cut_unit_stretches: on random ranges and every cut n_ord, the stretches name exactly the units that a walk over the ordinals
//     finds -- single reads outside the ranges, pairs inside, a pair that n_ord cuts as a unit of its first mate -- in ascending
//     order, without empty stretches, in an array malloc'ed to exactly the promised 2 * n_ranges + 1 entries.
// Built with -fsanitize=address,undefined by tests/test_read_dedup_host.py.  Prints "dedup_plan_check: ok ..." or the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
#include "../soapdenovo-trans_amd/csrc/sdt_read_plan.h"

using namespace sdt;

#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			printf("dedup_plan_check: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                                      \
			printf("\n");                                             \
			exit(1);                                                  \
		}                                                             \
	} while (0)

static void table(void)
{
	for (uint64_t units = 0; units < 5000; units++) {
		const uint64_t s = dedup_table_slots(units);
		CHECK(s >= 2 && (s & (s - 1)) == 0, "%llu units: %llu slots", (unsigned long long)units, (unsigned long long)s);
		CHECK(s >= 2 * units, "%llu units: %llu slots", (unsigned long long)units, (unsigned long long)s);
		if (units > 1) CHECK(s < 4 * units, "%llu units: %llu slots", (unsigned long long)units, (unsigned long long)s);
	}
	for (int b = 12; b < 40; b++)
		for (int d = -1; d <= 1; d++) {
			const uint64_t units = (1ULL << b) + d, s = dedup_table_slots(units);
			CHECK((s & (s - 1)) == 0 && s >= 2 * units && s < 4 * units, "2^%d %+d units: %llu slots", b, d, (unsigned long long)s);
		}
	CHECK(DEDUP_SLOT_BYTES <= 24 && DEDUP_ENT_BYTES <= 24 && DEDUP_MAX_ROUNDS == 64, "the budget of the header");
}

static void faults(void)
{
	PairRangeFault f;
	const uint64_t good[] = {3, 11, 11, 15, 20, 20, 30, 32};
	CHECK(check_pair_ranges(good, 4, &f) == 4 && f == PAIR_RANGES_OK, "touching and empty ranges");
	CHECK(check_pair_ranges(nullptr, 0, &f) == 0 && f == PAIR_RANGES_OK, "no ranges");
	const uint64_t half[] = {0, 4, 6, 9}, back[] = {0, 4, 10, 8}, over[] = {0, 10, 8, 12}, order[] = {10, 20, 0, 10};
	CHECK(check_pair_ranges(half, 2, &f) == 1 && f == PAIR_RANGE_NOT_PAIRS, "half a pair");
	CHECK(check_pair_ranges(back, 2, &f) == 1 && f == PAIR_RANGE_NOT_PAIRS, "a range that runs backwards");
	CHECK(check_pair_ranges(over, 2, &f) == 1 && f == PAIR_RANGE_OVERLAPS, "overlap");
	CHECK(check_pair_ranges(order, 2, &f) == 1 && f == PAIR_RANGE_OVERLAPS, "descending");
}

static uint64_t stretches(void)
{
	std::mt19937_64 rng(20240917);
	uint64_t cut_pairs = 0, checked = 0;
	for (int rep = 0; rep < 400; rep++) {
		const uint64_t n_ranges = rng() % 5;
		uint64_t *pr = (uint64_t *)malloc((n_ranges ? 2 * n_ranges : 1) * sizeof(uint64_t));
		UnitStretch *out = (UnitStretch *)malloc((2 * n_ranges + 1) * sizeof(UnitStretch));
		CHECK(pr && out, "malloc");
		uint64_t at = rng() % 4;
		for (uint64_t i = 0; i < n_ranges; i++) {
			pr[2 * i] = at;
			pr[2 * i + 1] = at + 2 * (rng() % 6);
			at = pr[2 * i + 1] + (rng() % 3 ? rng() % 5 : 0);
		}
		PairRangeFault f;
		CHECK(check_pair_ranges(pr, n_ranges, &f) == n_ranges && f == PAIR_RANGES_OK, "rep %d", rep);
		for (uint64_t n_ord = 0; n_ord <= at + 3; n_ord++) {
			// the walk: (id, mates) of every unit that has an ordinal below n_ord
			std::vector<uint64_t> ids, strides;
			for (uint64_t o = 0; o < n_ord;) {
				uint64_t i = 0;
				while (i < n_ranges && !(pr[2 * i] <= o && o < pr[2 * i + 1])) i++;
				ids.push_back(o);
				strides.push_back(i < n_ranges ? 2 : 1);
				if (i < n_ranges && o + 1 == n_ord) cut_pairs++;
				o += i < n_ranges ? 2 : 1;
			}
			uint64_t units = ~0ULL, counted = ~0ULL;
			const uint64_t n = cut_unit_stretches(pr, n_ranges, n_ord, out, &units);
			CHECK(n <= 2 * n_ranges + 1 && units == ids.size(), "rep %d n_ord %llu: %llu stretches, %llu units of %zu", rep, (unsigned long long)n_ord,
			      (unsigned long long)n, (unsigned long long)units, ids.size());
			CHECK(cut_unit_stretches(pr, n_ranges, n_ord, nullptr, &counted) == n && counted == units, "counting only");
			for (uint64_t s = 0; s < n; s++) {
				const uint64_t end = s + 1 < n ? out[s + 1].unit0 : units;
				CHECK(out[s].unit0 < end && (out[s].stride == 1 || out[s].stride == 2), "rep %d: stretch %llu is empty", rep, (unsigned long long)s);
				CHECK(s == 0 ? out[s].unit0 == 0 : out[s].ord0 > out[s - 1].ord0, "rep %d: stretch %llu out of order", rep, (unsigned long long)s);
				for (uint64_t u = out[s].unit0; u < end; u++, checked++)
					CHECK(out[s].ord0 + (u - out[s].unit0) * out[s].stride == ids[u] && out[s].stride == strides[u],
					      "rep %d n_ord %llu: unit %llu", rep, (unsigned long long)n_ord, (unsigned long long)u);
			}
		}
		free(pr);
		free(out);
	}
	CHECK(cut_pairs > 50, "%llu pairs cut by n_ord", (unsigned long long)cut_pairs);
	return checked;
}

int main(void)
{
	table();
	faults();
	const uint64_t checked = stretches();
	printf("dedup_plan_check: ok (%llu units)\n", (unsigned long long)checked);
	return 0;
}
