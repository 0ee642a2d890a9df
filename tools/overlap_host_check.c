/* overlap_host_check.c -- the device-free host side of `sdt-kmers overlap` (csrc/host/overlapsplit.c) on synthetic input: what a read's
 * record line looks like, which records can be those of a read of a given length and of the two mates of one pair, and the histogram
 * of the inserts with its summary line: an empty histogram, an odd and an even number of inserts (the lower median), inserts noted
 * in no order, and more of them than the first block of the list holds.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o overlap_host_check \
 *       tools/overlap_host_check.c soapdenovo-trans_amd/csrc/host/overlapsplit.c && ./overlap_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/overlapsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* what sdt_insert_hist_write writes, in a block of exactly its length */
static char *written(sdt_insert_hist *h)
{
	FILE *f = tmpfile();
	if (!f) return NULL;
	CHECK(sdt_insert_hist_write(f, h) == 0);
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
	char *line = (char *)malloc(SDT_OVERLAP_LINE_MAX);
	const sdt_read_overlap widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_overlap_line(line, &widest);
	CHECK(end - line == SDT_OVERLAP_LINE_MAX && memcmp(line, "4294967295 4294967295 4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	const sdt_read_overlap some = {100, 3, 100, 0, 100, 2};
	end = sdt_put_overlap_line(line, &some);
	CHECK(end - line == 18 && memcmp(line, "100 3 100 0 100 2\n", 18) == 0);
	const sdt_read_overlap none = {0, 0, 0, 0, 0, 3};
	end = sdt_put_overlap_line(line, &none);
	CHECK(end - line == 12 && memcmp(line, "0 0 0 0 0 3\n", 12) == 0);
	free(line);

	/* records that a read of 150 bases can have, and records that it cannot */
	const sdt_read_overlap fine[] = {{0, 0, 0, 0, 150, 0}, {100, 3, 100, 0, 100, 2}, {80, 0, 220, 0, 150, 0}, {150, 15, 150, 0, 150, 0},
	                                 {100, 0, 100, 0, 0, 3}, {0, 0, 0, 0, 0, 3}, {1, 1, 1, 0, 1, 2}};
	for (size_t i = 0; i < sizeof fine / sizeof fine[0]; i++) CHECK(sdt_overlap_record_ok(fine + i, 150) == 1);
	const sdt_read_overlap wrong[] = {{0, 0, 0, 0, 150, 1}, {0, 0, 0, 0, 150, 4}, {0, 0, 0, 0, 150, 2}, {100, 3, 100, 0, 100, 0}, {100, 3, 100, 1, 99, 2},
	                                  {100, 3, 100, 0, 150, 0}, {100, 101, 100, 0, 100, 2}, {0, 0, 100, 0, 100, 2}, {30, 0, 0, 0, 150, 0},
	                                  {80, 0, 220, 0, 151, 2}, {0, 0, 0, 0, 149, 2}, {100, 0, 100, 0, 5, 3}};
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_overlap_record_ok(wrong + i, 150) == 0);
	/* a read of no bases is dropped, whatever its mate is */
	CHECK(sdt_overlap_record_ok(&none, 0) == 1);
	const sdt_read_overlap empty_whole = {0, 0, 0, 0, 0, 0};
	CHECK(sdt_overlap_record_ok(&empty_whole, 0) == 0);

	/* an empty histogram: the summary line alone, median 0 */
	sdt_insert_hist h;
	memset(&h, 0, sizeof h);
	CHECK(sdt_insert_hist_median(&h) == 0);
	char *got = written(&h);
	CHECK(got && strcmp(got, "# pairs 0 overlapping 0 clipped 0 median 0\n") == 0);
	free(got);
	/* pairs without an overlap count as pairs only */
	const sdt_read_overlap whole150 = {0, 0, 0, 0, 150, 0}, whole90 = {0, 0, 0, 0, 90, 0};
	CHECK(sdt_insert_hist_note(&h, &whole150, &whole90, 150, 90) == 0 && h.pairs == 1 && h.n == 0 && h.clipped == 0);
	CHECK(sdt_insert_hist_note(&h, &whole150, &none, 150, 0) == 0 && h.pairs == 2 && h.n == 0);
	got = written(&h);
	CHECK(got && strcmp(got, "# pairs 2 overlapping 0 clipped 0 median 0\n") == 0);
	free(got);
	/* overlapping pairs in no order: inserts 220, 100, 100, 90 (only one mate is cut), 300: five, the median is the third */
	const sdt_read_overlap f220 = {80, 0, 220, 0, 150, 0}, f100 = {100, 3, 100, 0, 100, 2}, f90a = {60, 0, 90, 0, 90, 2}, f90b = {60, 0, 90, 0, 60, 0};
	const sdt_read_overlap f300a = {50, 5, 300, 0, 200, 0}, f300b = {50, 5, 300, 0, 150, 0}, f100drop = {100, 3, 100, 0, 0, 3};
	CHECK(sdt_insert_hist_note(&h, &f220, &f220, 150, 150) == 0 && h.clipped == 0);
	CHECK(sdt_insert_hist_note(&h, &f100, &f100, 150, 150) == 0 && h.clipped == 1);
	CHECK(sdt_insert_hist_note(&h, &f100, &f100drop, 150, 150) == 0 && h.clipped == 2);        /* (min_len dropped the second mate) */
	CHECK(sdt_insert_hist_note(&h, &f90a, &f90b, 150, 60) == 0 && h.clipped == 3);
	CHECK(sdt_insert_hist_note(&h, &f300a, &f300b, 200, 150) == 0 && h.clipped == 3);
	CHECK(h.pairs == 7 && h.n == 5 && sdt_insert_hist_median(&h) == 100);
	got = written(&h);
	CHECK(got && strcmp(got, "90 1\n100 2\n220 1\n300 1\n# pairs 7 overlapping 5 clipped 3 median 100\n") == 0);
	free(got);
	/* an even number of inserts: the lower of the two in the middle (90 100 100 | 220 300 300) */
	CHECK(sdt_insert_hist_note(&h, &f300b, &f300a, 150, 200) == 0 && h.n == 6 && sdt_insert_hist_median(&h) == 100);
	/* (90 100 100 220 | 220 300 300 300): 220 */
	CHECK(sdt_insert_hist_note(&h, &f220, &f220, 150, 150) == 0 && sdt_insert_hist_note(&h, &f300a, &f300b, 200, 150) == 0);
	CHECK(h.n == 8 && sdt_insert_hist_median(&h) == 220);
	got = written(&h);
	CHECK(got && strcmp(got, "90 1\n100 2\n220 2\n300 3\n# pairs 10 overlapping 8 clipped 3 median 220\n") == 0);
	free(got);
	/* records that are not those of one pair: nothing is noted */
	const sdt_read_overlap f100h = {100, 4, 100, 0, 100, 2}, f101 = {100, 3, 101, 0, 101, 2}, o99 = {99, 3, 100, 0, 100, 2};
	CHECK(sdt_insert_hist_note(&h, &f100, &f100h, 150, 150) == -2);
	CHECK(sdt_insert_hist_note(&h, &f100, &f101, 150, 150) == -2);
	CHECK(sdt_insert_hist_note(&h, &f100, &o99, 150, 150) == -2);
	CHECK(sdt_insert_hist_note(&h, &f100, &whole150, 150, 150) == -2);
	CHECK(sdt_insert_hist_note(&h, &f100, &f100, 150, 90) == -2);                              /* (a mate of 90 bases keeps 90, not 100) */
	CHECK(h.pairs == 10 && h.n == 8 && h.clipped == 3);
	/* more inserts than the first block of the list holds */
	for (uint32_t i = 0; i < 3000; i++) {
		const uint32_t F = 31 + (i * 7919u) % 250;
		const sdt_read_overlap r = {30, 0, F, 0, F < 150 ? F : 150, F < 150 ? 2u : 0u};
		CHECK(sdt_insert_hist_note(&h, &r, &r, 150, 150) == 0);
	}
	CHECK(h.n == 3008 && h.pairs == 3010);
	const uint32_t med = sdt_insert_hist_median(&h);
	size_t below = 0, upto = 0;
	for (size_t i = 0; i < h.n; i++) { below += h.v[i] < med; upto += h.v[i] <= med; }
	CHECK(below <= (h.n - 1) / 2 && (h.n - 1) / 2 < upto);
	for (size_t i = 1; i < h.n; i++) CHECK(h.v[i - 1] <= h.v[i]);
	sdt_insert_hist_free(&h);
	CHECK(h.v == NULL && h.n == 0 && h.pairs == 0);
	if (failures) { fprintf(stderr, "overlap_host_check: %d checks failed\n", failures); return 1; }
	printf("overlap_host_check: ok\n");
	return 0;
}
