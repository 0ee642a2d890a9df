/* complexity_host_check.c -- the device-free host side of `sdt-kmers complexity` (csrc/host/cxsplit.c) on synthetic input: what a read's
 * record line looks like, which records can be those of a read of a given length (the windows of every length up to 300 against a walk
 * over the window starts), and the histogram of the scores with its summary line: an empty histogram, every verdict, the scores 0 and
 * 100 at the ends of the table, and records that are refused and leave the histogram as it was.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o complexity_host_check \
 *       tools/complexity_host_check.c soapdenovo-trans_amd/csrc/host/cxsplit.c && ./complexity_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/cxsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* what sdt_score_hist_write writes, in a block of exactly its length */
static char *written(const sdt_score_hist *h)
{
	FILE *f = tmpfile();
	if (!f) return NULL;
	CHECK(sdt_score_hist_write(f, h) == 0);
	const long n = ftell(f);
	rewind(f);
	char *got = (char *)malloc((size_t)n + 1);
	CHECK(fread(got, 1, (size_t)n, f) == (size_t)n);
	got[n] = 0;
	fclose(f);
	return got;
}

int main(void)
{
	/* the record line: the widest fields fill the promised size exactly */
	char *line = (char *)malloc(SDT_CX_LINE_MAX);
	const sdt_read_complexity widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_cx_line(line, &widest);
	CHECK(end - line == SDT_CX_LINE_MAX && memcmp(line, "4294967295 4294967295 4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	const sdt_read_complexity some = {4, 2, 21, 0, 32, 2};
	end = sdt_put_cx_line(line, &some);
	CHECK(end - line == 14 && memcmp(line, "4 2 21 0 32 2\n", 14) == 0);
	const sdt_read_complexity none = {0, 0, 0, 0, 0, 3};
	end = sdt_put_cx_line(line, &none);
	CHECK(end - line == 12 && memcmp(line, "0 0 0 0 0 3\n", 12) == 0);
	free(line);

	/* records that a read of 150 bases can have, and records that it cannot */
	const sdt_read_complexity fine[] = {{4, 0, 2, 0, 150, 0}, {4, 2, 21, 0, 150, 0}, {4, 2, 21, 0, 0, 3}, {4, 2, 21, 0, 32, 2}, {4, 1, 13, 64, 86, 2},
	                                    {4, 4, 100, 0, 0, 3}, {4, 0, 0, 0, 0, 3}, {4, 1, 10, 149, 1, 2}};
	for (size_t i = 0; i < sizeof fine / sizeof fine[0]; i++) CHECK(sdt_cx_record_ok(fine + i, 150) == 1);
	const sdt_read_complexity wrong[] = {{4, 0, 2, 0, 150, 1}, {4, 0, 2, 0, 150, 4}, {4, 0, 2, 0, 150, 2}, {3, 0, 2, 0, 150, 0}, {5, 0, 2, 0, 150, 0},
	                                     {4, 5, 21, 0, 150, 0}, {4, 2, 101, 0, 150, 0}, {4, 2, 21, 0, 32, 0}, {4, 2, 21, 1, 150, 2}, {4, 2, 21, 64, 87, 2},
	                                     {4, 2, 21, 0, 5, 3}, {4, 2, 21, 5, 0, 3}, {4, 2, 21, 0, 0, 2}, {4, 0, 2, 0, 100, 2}, {4, 2, 21, 0, 151, 0}};
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_cx_record_ok(wrong + i, 150) == 0);
	/* a read of no bases has no window and is dropped */
	CHECK(sdt_cx_record_ok(&none, 0) == 1);
	const sdt_read_complexity empty_whole = {0, 0, 0, 0, 0, 0}, empty_window = {1, 0, 0, 0, 0, 3};
	CHECK(sdt_cx_record_ok(&empty_whole, 0) == 0 && sdt_cx_record_ok(&empty_window, 0) == 0);
	/* the windows of every length: one per start 0, 32, 64, ... that leaves more than 32 bases, and one at least */
	for (uint64_t L = 1; L <= 300; L++) {
		uint32_t w = 0;
		for (uint64_t b = 0; b == 0 || b + 32 < L; b += 32) w++;
		const sdt_read_complexity whole = {w, 0, 1, 0, (uint32_t)L, 0}, fewer = {w - 1, 0, 1, 0, (uint32_t)L, 0}, more = {w + 1, 0, 1, 0, (uint32_t)L, 0};
		CHECK(sdt_cx_record_ok(&whole, L) == 1 && sdt_cx_record_ok(&fewer, L) == 0 && sdt_cx_record_ok(&more, L) == 0);
	}

	/* an empty histogram: the summary line alone */
	sdt_score_hist *h = (sdt_score_hist *)calloc(1, sizeof(sdt_score_hist));
	char *got = written(h);
	CHECK(got && strcmp(got, "# reads 0 low 0 dropped 0 clipped 0\n") == 0);
	free(got);
	/* every verdict, the two ends of the table, a read of no bases */
	const sdt_read_complexity homo = {4, 4, 100, 0, 0, 3}, zero = {1, 0, 0, 0, 3, 0};
	CHECK(sdt_score_hist_note(h, fine + 0, 150) == 0 && sdt_score_hist_note(h, fine + 1, 150) == 0 && sdt_score_hist_note(h, fine + 2, 150) == 0);
	CHECK(sdt_score_hist_note(h, fine + 3, 150) == 0 && sdt_score_hist_note(h, fine + 4, 150) == 0 && sdt_score_hist_note(h, &homo, 150) == 0);
	CHECK(sdt_score_hist_note(h, &zero, 3) == 0 && sdt_score_hist_note(h, &none, 0) == 0 && sdt_score_hist_note(h, fine + 6, 150) == 0);
	CHECK(h->reads == 9 && h->low == 5 && h->dropped == 4 && h->clipped == 2);
	got = written(h);
	CHECK(got && strcmp(got, "0 3\n2 1\n13 1\n21 3\n100 1\n# reads 9 low 5 dropped 4 clipped 2\n") == 0);
	free(got);
	/* records that no read of that length has: nothing is noted */
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_score_hist_note(h, wrong + i, 150) == -2);
	CHECK(sdt_score_hist_note(h, &widest, 150) == -2 && sdt_score_hist_note(h, fine + 0, 151) == -2);
	CHECK(h->reads == 9 && h->low == 5 && h->dropped == 4 && h->clipped == 2 && h->by_score[21] == 3);
	free(h);
	if (failures) { fprintf(stderr, "complexity_host_check: %d checks failed\n", failures); return 1; }
	printf("complexity_host_check: ok\n");
	return 0;
}
