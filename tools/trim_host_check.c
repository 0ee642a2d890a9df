/* trim_host_check.c -- the device-free host side of `sdt-kmers trim` (csrc/host/trimsplit.c) on synthetic records: where a read goes
 * given its own record, its mate's and the pair ranges, and what its record line looks like.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o trim_host_check \
 *       tools/trim_host_check.c soapdenovo-trans_amd/csrc/host/trimsplit.c soapdenovo-trans_amd/csrc/host/normsplit.c && ./trim_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/trimsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* what the route asks of the records' owner: is anything of read `ord` kept */
static int alive(const void *recs, uint64_t ord) { return ((const sdt_read_trim *)recs)[ord].len != 0; }

int main(void)
{
	/* ordinals: 0..2 single reads, [3, 11) four pairs of a pair of files (the range starts at an odd ordinal), 11 a single read,
	 * [12, 16) two pairs of which the last mate has no record (nrec cuts it off) */
	sdt_pair_ranges pr;
	memset(&pr, 0, sizeof pr);
	CHECK(sdt_pair_ranges_note(&pr, 0, 1, 0, 3) == 0);
	CHECK(sdt_pair_ranges_note(&pr, 3, 2, 0, 4) == 0);
	CHECK(sdt_pair_ranges_note(&pr, 4, 2, 1, 4) == 0);
	CHECK(sdt_pair_ranges_note(&pr, 11, 1, 0, 1) == 0);
	CHECK(sdt_pair_ranges_note(&pr, 12, 2, 0, 2) == 0);
	CHECK(sdt_pair_ranges_note(&pr, 13, 2, 1, 2) == 0);
	CHECK(pr.n == 2 && pr.v[0] == 3 && pr.v[1] == 11 && pr.v[2] == 12 && pr.v[3] == 16);
	const uint64_t nrec = 15;
	sdt_read_trim *t = (sdt_read_trim *)calloc(nrec, sizeof *t);          /* exactly nrec records: a look past them is a finding */
	CHECK(t != NULL);
	if (!t) return 1;
	const uint32_t len[15] = {100, 0, 40, /* pairs */ 100, 100, 0, 70, 60, 0, 0, 0, /* single */ 90, /* pairs */ 0, 50, 80};
	for (uint64_t i = 0; i < nrec; i++) {
		t[i].kmers = len[i] ? 70 : 0;
		t[i].len = len[i];
		t[i].verdict = len[i] == 100 ? 0u : (len[i] ? 2u : 3u);
	}
	const int want[15] = {SDT_TRIM_TO_SINGLE, SDT_TRIM_TO_NONE, SDT_TRIM_TO_SINGLE,
	                      SDT_TRIM_TO_PAIRS, SDT_TRIM_TO_PAIRS,              /* both mates survive */
	                      SDT_TRIM_TO_NONE, SDT_TRIM_TO_SINGLE,              /* the first mate was dropped: the second is an orphan */
	                      SDT_TRIM_TO_SINGLE, SDT_TRIM_TO_NONE,              /* ... and the other way round */
	                      SDT_TRIM_TO_NONE, SDT_TRIM_TO_NONE,
	                      SDT_TRIM_TO_SINGLE,
	                      SDT_TRIM_TO_NONE, SDT_TRIM_TO_SINGLE,
	                      SDT_TRIM_TO_SINGLE};                               /* its mate is ordinal 15: no record */
	size_t cur = 0;
	int pairs_out = 0;
	for (uint64_t ord = 0; ord < nrec; ord++) {
		const int got = sdt_trim_route(&pr, &cur, alive, t, nrec, ord);
		CHECK(got == want[ord]);
		pairs_out += got == SDT_TRIM_TO_PAIRS;
	}
	CHECK(pairs_out % 2 == 0);
	CHECK(sdt_trim_route(&pr, &cur, alive, t, nrec, nrec) == SDT_TRIM_TO_NONE); /* past the records */
	/* no ranges at all */
	sdt_pair_ranges none;
	memset(&none, 0, sizeof none);
	cur = 0;
	CHECK(sdt_trim_route(&none, &cur, alive, t, nrec, 3) == SDT_TRIM_TO_SINGLE);
	CHECK(sdt_trim_route(&none, &cur, alive, t, nrec, 5) == SDT_TRIM_TO_NONE);

	/* the record line: the widest fields fill the promised size exactly, the smallest take 12 bytes */
	char *line = (char *)malloc(SDT_TRIM_LINE_MAX);
	CHECK(line != NULL);
	if (!line) return 1;
	const sdt_read_trim widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_trim_line(line, &widest);
	CHECK(end - line == SDT_TRIM_LINE_MAX);
	CHECK(memcmp(line, "4294967295 4294967295 4294967295 4294967295 4294967295 4294967295\n", SDT_TRIM_LINE_MAX) == 0);
	const sdt_read_trim zero = {0, 0, 0, 0, 0, 0};
	end = sdt_put_trim_line(line, &zero);
	CHECK(end - line == 12 && memcmp(line, "0 0 0 0 0 0\n", 12) == 0);
	const sdt_read_trim some = {130, 21, 8, 17, 93, 2};
	end = sdt_put_trim_line(line, &some);
	CHECK(end - line == 17 && memcmp(line, "130 21 8 17 93 2\n", 17) == 0);

	/* a trimmed read's record: bases [start, start + len) of the stream, in a buffer of exactly the promised size */
	const uint32_t words[2] = {0x1B1B1B1Bu, 0xE4000000u};                 /* ACTG x 4, then GTCA */
	char *rec = (char *)malloc(6 + 23);
	CHECK(rec != NULL);
	if (!rec) return 1;
	end = sdt_put_fasta_record(rec, 41, words, 14, 6);
	CHECK(end - rec == 4 + 6 + 1 && memcmp(rec, ">42\nTGGTCA\n", 11) == 0);
	free(rec);
	free(line);
	free(t);
	sdt_pair_ranges_free(&pr);
	if (failures) { fprintf(stderr, "trim_host_check: %d checks failed\n", failures); return 1; }
	printf("trim_host_check: ok\n");
	return 0;
}
