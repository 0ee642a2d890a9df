// layout_plan_check.cpp -- csrc/sdt_layout_plan.h on the CPU: the growth schedule of the layout replay against a simulation that
// makes every put, and against growth lines recorded from the reference (tests/golden/unit_*.txt).
//
//   layout_plan_check [init SIZE MAX] [grow COUNT SIZE MAX] [prime N NEXT] ...
//       init SIZE MAX        a fresh set has SIZE slots and grows at the put that finds MAX keys
//       grow COUNT SIZE MAX  the put that finds COUNT keys grows the set to SIZE slots, which hold MAX keys
//       prime N NEXT         find_next_prime_kh(N) == NEXT
//
// Build: c++ -std=c++17 -O1 -g -fsanitize=address,undefined -o layout_plan_check layout_plan_check.cpp
// (tests/test_layout_plan_host.py does, and passes the lines of the fixtures)
#include "../soapdenovo-trans_amd/csrc/sdt_layout_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "layout_plan_check: %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// ---- a set, put by put: only the counters of the reference's table (put_kmerset / encap_kmerset, newhash.c), written without the
// header.  The products are the ones csrc/host/graph/graph.c documents: float at init, the float 0.77f widened to double afterwards.
struct SimSet { unsigned long long size, count, max; };
static bool sim_passes_for_prime(unsigned long long num)
{
	if (num < 4) return true;
	if (!(num & 1)) return false;
	const unsigned long long bound = (unsigned long long)sqrt((float)num);      // (exclusive: the reference's bound)
	unsigned long long d = 3;
	while (d < bound && num % d) d += 2;
	return d >= bound;
}
static void sim_init(SimSet &S, unsigned long long init_size)
{
	S.size = init_size;
	S.count = 0;
	S.max = (unsigned long long)(S.size * 0.77f);
}
static bool sim_make_room(SimSet &S)                      // before a put; true: the table grew
{
	if (S.count + 1 <= S.max) return false;
	const double load = (double)0.77f;
	unsigned long long n = S.size;
	for (bool enough = false; !enough; enough = n * load >= (double)(S.count + 1)) {
		n += n < 0xFFFFFFFu ? n : 0xFFFFFFu;
		n |= 1;
		while (!sim_passes_for_prime(n)) n += 2;
	}
	S.size = n;
	S.max = (unsigned long long)(n * load);
	return true;
}
static std::vector<sdt::RpGen> simulate(unsigned long long keys, unsigned long long init_size, bool *additive)
{
	SimSet S;
	sim_init(S, init_size);
	std::vector<sdt::RpGen> gens;
	unsigned long long lo = 0;
	for (unsigned long long id = 0; id < keys; id++) {
		const unsigned long long before = S.size;
		if (sim_make_room(S)) {
			if (before >= 0xFFFFFFFu && additive) *additive = true;
			gens.push_back(sdt::RpGen{(uint32_t)lo, (uint32_t)id, (uint32_t)before});
			lo = id;
		}
		S.count++;
	}
	gens.push_back(sdt::RpGen{(uint32_t)lo, (uint32_t)keys, (uint32_t)S.size});
	return gens;
}

static bool same_schedule(const sdt::RpSchedule &a, const sdt::RpSchedule &b)
{
	if (a.gens.size() != b.gens.size() || a.tab0 != b.tab0 || a.tab_total != b.tab_total || a.max_size != b.max_size || a.max_gens != b.max_gens || a.qbits != b.qbits)
		return false;
	for (size_t s = 0; s < a.gens.size(); s++) {
		if (a.gens[s].size() != b.gens[s].size()) return false;
		for (size_t g = 0; g < a.gens[s].size(); g++)
			if (a.gens[s][g].lo != b.gens[s][g].lo || a.gens[s][g].hi != b.gens[s][g].hi || a.gens[s][g].size != b.gens[s][g].size) return false;
	}
	return true;
}

static void check_against_simulation(void)
{
	for (const unsigned long long init_size : {1031ULL, 3ULL}) {
		// the sizes around the first two growths of 1031 slots (793 and 1588 keys), an empty set, one key, a million, and one whose last
		// growth starts past 2^28 - 1 slots (the additive step: from 271018903 slots, or from 402653189 when the set began with 3)
		const uint64_t sizes[] = {0, 1, 792, 793, 794, 1588, 1589, 1000000, init_size == 3 ? 320000000ULL : 210000000ULL};
		const int p = (int)(sizeof sizes / sizeof sizes[0]);
		sdt::RpSchedule sch;
		const sdt::RpPlanStatus st = sdt::rp_schedule(sizes, p, init_size == 3 ? 2 : 1, init_size == 3, sch);
		CHECK(st == sdt::RP_PLAN_OK, "init %llu: status %d", init_size, (int)st);
		CHECK((int)sch.gens.size() == p && (int)sch.tab0.size() == p, "init %llu: %zu sets", init_size, sch.gens.size());
		uint64_t total = 0, max_size = 0;
		size_t max_gens = 0;
		bool additive = false;
		for (int s = 0; s < p; s++) {
			const std::vector<sdt::RpGen> want = simulate(sizes[s], init_size, &additive);
			const std::vector<sdt::RpGen> &got = sch.gens[s];
			CHECK(got.size() == want.size(), "init %llu, %llu keys: %zu generations, simulated %zu", init_size, (unsigned long long)sizes[s], got.size(), want.size());
			for (size_t g = 0; g < got.size() && g < want.size(); g++)
				CHECK(got[g].lo == want[g].lo && got[g].hi == want[g].hi && got[g].size == want[g].size,
				      "init %llu, %llu keys, generation %zu: [%u, %u) in %u slots, simulated [%u, %u) in %u", init_size, (unsigned long long)sizes[s], g,
				      got[g].lo, got[g].hi, got[g].size, want[g].lo, want[g].hi, want[g].size);
			CHECK(sch.tab0[s] == total, "set %d starts at slot %llu, the sets before it have %llu", s, (unsigned long long)sch.tab0[s], (unsigned long long)total);
			total += want.back().size;
			if (want.back().size > max_size) max_size = want.back().size;
			if (want.size() > max_gens) max_gens = want.size();
		}
		CHECK(additive, "init %llu: no growth took the additive step", init_size);
		CHECK(sch.tab_total == total && sch.max_size == max_size && sch.max_gens == max_gens, "init %llu: totals %llu %llu %zu, simulated %llu %llu %zu", init_size,
		      (unsigned long long)sch.tab_total, (unsigned long long)sch.max_size, sch.max_gens, (unsigned long long)total, (unsigned long long)max_size, max_gens);
		CHECK((1ULL << sch.qbits) > max_size && (1ULL << (sch.qbits - 1)) <= max_size, "%d slot bits for %llu slots", sch.qbits, (unsigned long long)max_size);
		// small_init counts only in the variants of more than one word: every (variant, small_init) with this initial size gives this schedule
		int others = 0;
		for (int variant : {1, 2, 4})
			for (int small = 0; small < 2; small++) {
				if ((small && variant != 1) != (init_size == 3)) continue;
				sdt::RpSchedule other;
				CHECK(sdt::rp_schedule(sizes, p, variant, small, other) == sdt::RP_PLAN_OK && same_schedule(sch, other), "variant %d, small_init %d: another schedule", variant, small);
				others++;
			}
		CHECK(others == (init_size == 3 ? 2 : 4), "init %llu: %d (variant, small_init) pairs", init_size, others);
	}
	// the same schedule whatever the neighbours: a set alone
	const uint64_t one = 1589;
	sdt::RpSchedule sch;
	CHECK(sdt::rp_schedule(&one, 1, 1, 0, sch) == sdt::RP_PLAN_OK && sch.gens[0].size() == 3 && sch.gens[0][2].lo == 1588 && sch.max_gens == 3, "1589 keys alone");
}

static void check_limits(void)
{
	sdt::RpSchedule sch;
	// 2^32 slots hold 0.77 x 2^32 keys: a set past that cannot be scheduled (the sizes below grow additively, 2^24 at a time)
	const uint64_t huge = 3400000000ULL;
	CHECK(sdt::rp_schedule(&huge, 1, 1, 0, sch) == sdt::RP_PLAN_SLOTS, "%llu keys: no refusal", (unsigned long long)huge);
	// 2 x 30 slot bits + the depth bits pass 64: 2^29 slots and more
	const uint64_t wide = 420000000ULL;
	const sdt::RpPlanStatus st = sdt::rp_schedule(&wide, 1, 1, 0, sch);
	CHECK(st == sdt::RP_PLAN_BITS && sch.qbits == 30, "%llu keys: status %d, %d slot bits", (unsigned long long)wide, (int)st, sch.qbits);
	const uint64_t fits = 400000000ULL;
	CHECK(sdt::rp_schedule(&fits, 1, 1, 0, sch) == sdt::RP_PLAN_OK && sch.qbits == 29, "%llu keys: %d slot bits", (unsigned long long)fits, sch.qbits);
	std::vector<uint64_t> many(1024, 5);
	CHECK(sdt::rp_schedule(many.data(), 1024, 1, 0, sch) == sdt::RP_PLAN_BITS, "1024 sets: no refusal");
	CHECK(sdt::rp_schedule(many.data(), 1023, 1, 0, sch) == sdt::RP_PLAN_OK && sch.tab_total == 1023 * 1031ULL, "1023 sets");
}

static void check_list_capacity(void)
{
	// a quarter of the keys fits the closed chunks, and every wave of 8 workgroups per CU has its open chunk on top
	for (const uint64_t n : {0ULL, 1ULL, 767ULL, 768ULL, 1000000ULL, 678000000ULL})
		for (const int cu : {1, 256}) {
			const unsigned long long ch = sdt::rp_list_chunks(n, cu), open = (unsigned long long)cu * 8 * sdt::RP_PLAN_WAVES;
			CHECK(ch > open && (ch - open) * (sdt::RP_PLAN_CHUNK - 64) > n / 4, "%llu keys, %d CUs: %llu chunks", (unsigned long long)n, cu, ch);
			CHECK((ch - open - 1) * (sdt::RP_PLAN_CHUNK - 64) <= (n ? n : 1) / 4 + 1, "%llu keys, %d CUs: %llu chunks are too many", (unsigned long long)n, cu, ch);
		}
	CHECK(sdt::rp_list_chunks(0, 256) == 1 + 256 * 8 * 4, "no keys: %llu chunks", sdt::rp_list_chunks(0, 256));
}

// the lines of the reference's own run
static int check_recorded(int argc, char **argv)
{
	int n = 0;
	for (int i = 1; i < argc; n++) {
		const char *what = argv[i];
		const int nargs = !strcmp(what, "init") || !strcmp(what, "prime") ? 2 : !strcmp(what, "grow") ? 3 : -1;
		if (nargs < 0 || i + nargs >= argc) { fprintf(stderr, "layout_plan_check: bad argument %s\n", what); exit(2); }
		const uint64_t a = strtoull(argv[i + 1], nullptr, 10), b = strtoull(argv[i + 2], nullptr, 10), c = nargs == 3 ? strtoull(argv[i + 3], nullptr, 10) : 0;
		i += 1 + nargs;
		sdt::RpSchedule sch;
		if (!strcmp(what, "prime")) {
			CHECK(sdt::rp_next_prime(a) == b, "prime %llu: %llu, recorded %llu", (unsigned long long)a, (unsigned long long)sdt::rp_next_prime(a), (unsigned long long)b);
		} else if (!strcmp(what, "init")) {
			const uint64_t keys = b + 1;
			CHECK(sdt::rp_schedule(&keys, 1, 1, 0, sch) == sdt::RP_PLAN_OK && sch.gens[0].size() == 2 && sch.gens[0][0].size == a && sch.gens[0][0].hi == b,
			      "init: %u slots for %u keys, recorded %llu for %llu", sch.gens[0][0].size, sch.gens[0][0].hi, (unsigned long long)a, (unsigned long long)b);
		} else {
			const uint64_t keys = c + 1;                       // (one key more than the grown table holds: the generation ends at its max)
			bool found = false;
			CHECK(sdt::rp_schedule(&keys, 1, 1, 0, sch) == sdt::RP_PLAN_OK, "grow: %llu keys refused", (unsigned long long)keys);
			for (const sdt::RpGen &g : sch.gens[0]) found |= g.lo == a && g.size == b && g.hi == c;
			CHECK(found, "grow: no generation [%llu, %llu) in %llu slots", (unsigned long long)a, (unsigned long long)c, (unsigned long long)b);
		}
	}
	return n;
}

int main(int argc, char **argv)
{
	check_against_simulation();
	check_limits();
	check_list_capacity();
	const int recorded = check_recorded(argc, argv);
	if (failures) { fprintf(stderr, "layout_plan_check: %d checks failed\n", failures); return 1; }
	printf("layout_plan_check: ok (%d recorded lines)\n", recorded);
	return 0;
}
