/* select_host_check.c -- the device-free host side of `sdt-kmers normalize` (csrc/host/normsplit.c) on synthetic stream callbacks:
 * the pair ranges that come out of the batches of paired files, and where kept reads go and what their records look like.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o select_host_check \
 *       tools/select_host_check.c soapdenovo-trans_amd/csrc/host/normsplit.c && ./select_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/normsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* a pair of files of n1 / n2 reads from ordinal `at` on, in batches of `step` reads: the read-1 file first, as readstream.c does */
static uint64_t feed_pair_files(sdt_pair_ranges *pr, uint64_t at, uint64_t n1, uint64_t n2, uint64_t step)
{
	for (uint64_t i = 0; i < n1; i += step) CHECK(sdt_pair_ranges_note(pr, at + 2 * i, 2, 0, n1 - i < step ? n1 - i : step) == 0);
	for (uint64_t i = 0; i < n2; i += step) CHECK(sdt_pair_ranges_note(pr, at + 1 + 2 * i, 2, 1, n2 - i < step ? n2 - i : step) == 0);
	return at + 2 * (n1 > n2 ? n1 : n2);
}

static uint64_t feed_single_file(sdt_pair_ranges *pr, uint64_t at, uint64_t n, uint64_t step)
{
	for (uint64_t i = 0; i < n; i += step) CHECK(sdt_pair_ranges_note(pr, at + i, 1, 0, n - i < step ? n - i : step) == 0);
	return at + n;
}

static void expect_ranges(const sdt_pair_ranges *pr, const uint64_t *want, size_t n)
{
	CHECK(pr->n == n);
	for (size_t i = 0; i < 2 * n && i < 2 * pr->n; i++) CHECK(pr->v[i] == want[i]);
	for (size_t i = 0; i < pr->n; i++) {
		CHECK(pr->v[2 * i] < pr->v[2 * i + 1] && (pr->v[2 * i + 1] - pr->v[2 * i]) % 2 == 0);
		if (i) CHECK(pr->v[2 * i - 1] < pr->v[2 * i]);
	}
}

int main(void)
{
	sdt_pair_ranges pr;
	memset(&pr, 0, sizeof pr);
	/* nothing but single reads */
	uint64_t at = feed_single_file(&pr, 0, 1000, 64);
	expect_ranges(&pr, NULL, 0);
	size_t cur = 0;
	CHECK(!sdt_pair_ranges_holds(&pr, 5, &cur));
	sdt_pair_ranges_free(&pr);

	/* 7 single reads, a pair of files (the range starts at an odd ordinal), one single read, two pairs of files back to back (they
	 * merge), an empty batch, single reads */
	at = feed_single_file(&pr, 0, 7, 3);
	at = feed_pair_files(&pr, at, 100, 100, 16);
	CHECK(at == 207);
	at = feed_single_file(&pr, at, 1, 1);
	at = feed_pair_files(&pr, at, 50, 50, 50);
	CHECK(sdt_pair_ranges_note(&pr, at, 2, 0, 0) == 0);
	at = feed_pair_files(&pr, at, 33, 33, 1);
	at = feed_single_file(&pr, at, 10, 4);
	{
		const uint64_t want[] = {7, 207, 208, 208 + 100 + 66};
		expect_ranges(&pr, want, 2);
	}
	cur = 0;
	for (uint64_t o = 0; o < at + 3; o++)
		CHECK(sdt_pair_ranges_holds(&pr, o, &cur) == ((o >= 7 && o < 207) || (o >= 208 && o < 374)));
	sdt_pair_ranges_free(&pr);

	/* files of unequal length: the longer one decides where the range ends, and it holds whole pairs */
	at = feed_pair_files(&pr, 0, 10, 4, 3);
	at = feed_pair_files(&pr, at, 2, 9, 4);
	{
		const uint64_t want[] = {0, 38};
		expect_ranges(&pr, want, 1);
	}
	CHECK(at == 38);
	sdt_pair_ranges_free(&pr);

	/* a read-1 file without a read: the read-2 batches alone open the range, one ordinal before their own; and the other way round */
	at = feed_single_file(&pr, 0, 5, 5);
	at = feed_pair_files(&pr, at, 0, 6, 4);
	CHECK(at == 17);
	at = feed_single_file(&pr, at, 2, 2);
	at = feed_pair_files(&pr, at, 3, 0, 2);
	{
		const uint64_t want[] = {5, 17, 19, 25};
		expect_ranges(&pr, want, 2);
	}
	sdt_pair_ranges_free(&pr);

	/* many separate ranges: the list grows, stays sorted, and a range given twice changes nothing */
	at = 1;
	for (int i = 0; i < 100; i++) {
		at = feed_pair_files(&pr, at, 5, 5, 2);
		at = feed_single_file(&pr, at, 3, 3);
	}
	CHECK(pr.n == 100 && pr.v[0] == 1 && pr.v[1] == 11 && pr.v[198] == 1 + 99 * 13 && pr.v[199] == 1 + 99 * 13 + 10);
	CHECK(sdt_pair_ranges_note(&pr, 14, 2, 0, 5) == 0 && pr.n == 100 && pr.v[2] == 14 && pr.v[3] == 24);
	sdt_pair_ranges_free(&pr);

	/* the records: 40 bases from base 13 of a stream (across word boundaries), the last ordinal there is, an empty read */
	uint32_t words[8];
	char want[64], buf[128];
	for (int i = 0; i < 8; i++) words[i] = 0x1B1B1B1Bu * (uint32_t)(i + 1) ^ 0x9E3779B9u;
	for (int i = 0; i < 40; i++) want[i] = "ACTG"[(words[(13 + i) >> 4] >> (30 - 2 * ((13 + i) & 15))) & 3u];
	char *e = sdt_put_fasta_record(buf, 41, words, 13, 40);
	CHECK(e - buf == 4 + 41 && !memcmp(buf, ">42\n", 4) && !memcmp(buf + 4, want, 40) && e[-1] == '\n');
	e = sdt_put_fasta_record(buf, 18446744073709551614ULL, words, 0, 0);
	CHECK(e - buf == 23 && !memcmp(buf, ">18446744073709551615\n\n", 23));
	/* kept reads of a stream go to the pairs file or to the singles file by their ordinal */
	at = feed_single_file(&pr, 0, 3, 3);
	at = feed_pair_files(&pr, at, 4, 4, 4);
	at = feed_single_file(&pr, at, 2, 2);
	char pairs_txt[256] = "", single_txt[256] = "", *pp = pairs_txt, *ps = single_txt;
	cur = 0;
	for (uint64_t o = 0; o < at; o++) {
		if (o % 3 == 1) continue;                                            /* dropped */
		if (sdt_pair_ranges_holds(&pr, o, &cur)) pp = sdt_put_fasta_record(pp, o, words, 2 * o, 2);
		else ps = sdt_put_fasta_record(ps, o, words, 2 * o, 2);
	}
	*pp = *ps = 0;
	int np = 0, ns = 0;
	for (char *c = pairs_txt; *c; c++) np += *c == '>';
	for (char *c = single_txt; *c; c++) ns += *c == '>';
	CHECK(np == 5 && ns == 4);                                               /* ordinals 3 5 6 8 9 | 0 2 11 12 */
	CHECK(!strncmp(pairs_txt, ">4\n", 3) && !strncmp(single_txt, ">1\n", 3));
	sdt_pair_ranges_free(&pr);

	if (failures) { fprintf(stderr, "select_host_check: %d checks failed\n", failures); return 1; }
	printf("select_host_check: ok\n");
	return 0;
}
