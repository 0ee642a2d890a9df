/* dedup_host_check.c -- the device-free host side of `sdt-kmers dedup` (csrc/host/dupsplit.c) on synthetic records: what a read's
 * record line looks like, and the table of duplication levels from the records of a stream.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o dedup_host_check \
 *       tools/dedup_host_check.c soapdenovo-trans_amd/csrc/host/dupsplit.c && ./dedup_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/dupsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main(void)
{
	/* the record line: the widest fields fill the promised size exactly, the smallest take 6 bytes */
	char *line = (char *)malloc(SDT_DUP_LINE_MAX);
	CHECK(line != NULL);
	if (!line) return 1;
	const sdt_read_dup widest = {0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_dup_line(line, &widest);
	CHECK(end - line == SDT_DUP_LINE_MAX);
	CHECK(memcmp(line, "18446744073709551615 4294967295 4294967295\n", SDT_DUP_LINE_MAX) == 0);
	const sdt_read_dup zero = {0, 0, 0};
	end = sdt_put_dup_line(line, &zero);
	CHECK(end - line == 6 && memcmp(line, "0 0 0\n", 6) == 0);
	const sdt_read_dup some = {1234567, 7, 1};
	end = sdt_put_dup_line(line, &some);
	CHECK(end - line == 12 && memcmp(line, "1234567 7 1\n", 12) == 0);
	free(line);

	/* a stream of 14 reads: single reads 0 .. 5 (classes {0, 2, 5}, {1}, {3, 4}), pairs [6, 14) (classes {6, 10, 12}, {8}): the levels
	 * come out ascending whatever the order the records come in, a pair counts two reads and one class */
	const sdt_read_dup rec[14] = {{0, 3, 0}, {1, 1, 0}, {0, 3, 1}, {3, 2, 0}, {3, 2, 1}, {0, 3, 1},
	                              {6, 3, 0}, {6, 3, 0}, {8, 1, 0}, {8, 1, 0}, {6, 3, 1}, {6, 3, 1}, {6, 3, 1}, {6, 3, 1}};
	static const int orders[2][14] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13}, {13, 4, 9, 0, 7, 2, 11, 6, 1, 8, 3, 10, 5, 12}};
	for (int o = 0; o < 2; o++) {
		sdt_dup_levels lv;
		memset(&lv, 0, sizeof lv);
		for (int j = 0; j < 14; j++) {
			const int i = orders[o][j];
			CHECK(sdt_dup_levels_note(&lv, rec + i, rec[i].verdict == 0 && rec[i].first == (uint64_t)i) == 0);
		}
		CHECK(lv.n == 3);
		if (lv.n == 3) {
			CHECK(lv.v[0].copies == 1 && lv.v[0].classes == 2 && lv.v[0].reads == 3);
			CHECK(lv.v[1].copies == 2 && lv.v[1].classes == 1 && lv.v[1].reads == 2);
			CHECK(lv.v[2].copies == 3 && lv.v[2].classes == 2 && lv.v[2].reads == 9);
		}
		sdt_dup_levels_free(&lv);
		CHECK(lv.v == NULL && lv.n == 0);
	}
	/* more levels than the first allocation holds, descending: every insertion goes in front */
	sdt_dup_levels lv;
	memset(&lv, 0, sizeof lv);
	for (uint32_t c = 100; c >= 1; c--) {
		const sdt_read_dup r = {c, c, 0};
		CHECK(sdt_dup_levels_note(&lv, &r, 1) == 0);
		CHECK(sdt_dup_levels_note(&lv, &r, 0) == 0);
	}
	CHECK(lv.n == 100);
	for (size_t i = 0; i < lv.n; i++)
		CHECK(lv.v[i].copies == i + 1 && lv.v[i].classes == 1 && lv.v[i].reads == 2);
	char *ll = (char *)malloc(SDT_DUP_LEVEL_LINE_MAX);
	CHECK(ll != NULL);
	if (!ll) return 1;
	end = sdt_put_dup_level_line(ll, lv.v + 41);
	CHECK(end - ll == 7 && memcmp(ll, "42 1 2\n", 7) == 0);
	const sdt_dup_level wide = {0xFFFFFFFFu, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};
	end = sdt_put_dup_level_line(ll, &wide);
	CHECK(end - ll == SDT_DUP_LEVEL_LINE_MAX && memcmp(ll, "4294967295 18446744073709551615 18446744073709551615\n", SDT_DUP_LEVEL_LINE_MAX) == 0);
	free(ll);
	sdt_dup_levels_free(&lv);
	if (failures) { fprintf(stderr, "dedup_host_check: %d checks failed\n", failures); return 1; }
	printf("dedup_host_check: ok\n");
	return 0;
}
