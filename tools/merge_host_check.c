/* merge_host_check.c -- the device-free host side of `sdt-kmers merge` (csrc/host/mergesplit.c) on synthetic input: what a read's
 * record line looks like, which records can be those of a read with a given overlap record and of the two mates of one pair, and the
 * statistics with the summary line: no pairs, pairs without overlap, overlapping pairs that a length limit kept apart, merged pairs.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o merge_host_check \
 *       tools/merge_host_check.c soapdenovo-trans_amd/csrc/host/mergesplit.c && ./merge_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/mergesplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main(void)
{
	/* the record line: the widest fields fill the promised size exactly */
	char *line = (char *)malloc(SDT_MERGE_LINE_MAX);
	const sdt_read_merge widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_merge_line(line, &widest);
	CHECK(end - line == SDT_MERGE_LINE_MAX && memcmp(line, "4294967295 4294967295 4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	const sdt_read_merge m200 = {200, 3, 1, 0, 0, SDT_MERGE_MERGED};
	end = sdt_put_merge_line(line, &m200);
	CHECK(end - line == 14 && memcmp(line, "200 3 1 0 0 5\n", 14) == 0);
	const sdt_read_merge kept100 = {0, 0, 0, 0, 100, 2};
	end = sdt_put_merge_line(line, &kept100);
	CHECK(end - line == 14 && memcmp(line, "0 0 0 0 100 2\n", 14) == 0);
	free(line);

	/* records that a read of 150 bases with a given overlap record can have, and records that it cannot */
	const sdt_read_overlap ov200 = {100, 3, 200, 0, 150, 0}, ov100 = {100, 3, 100, 0, 100, 2}, ovnone = {0, 0, 0, 0, 150, 0}, ovdrop = {32, 0, 50, 0, 0, 3};
	const sdt_read_merge m100 = {100, 3, 0, 0, 0, SDT_MERGE_MERGED}, m50 = {50, 0, 0, 0, 0, SDT_MERGE_MERGED};
	const sdt_read_merge whole = {0, 0, 0, 0, 150, 0}, dropped = {0, 0, 0, 0, 0, 3}, all_b = {200, 3, 3, 0, 0, SDT_MERGE_MERGED};
	CHECK(sdt_merge_record_ok(&m200, &ov200, 150) == 1 && sdt_merge_record_ok(&all_b, &ov200, 150) == 1);
	CHECK(sdt_merge_record_ok(&m100, &ov100, 150) == 1 && sdt_merge_record_ok(&kept100, &ov100, 150) == 1);     /* (a length limit kept the pair apart) */
	CHECK(sdt_merge_record_ok(&whole, &ovnone, 150) == 1 && sdt_merge_record_ok(&whole, &ov200, 150) == 1);
	CHECK(sdt_merge_record_ok(&m50, &ovdrop, 32) == 1 && sdt_merge_record_ok(&dropped, &ovdrop, 32) == 1);      /* (a mate the overlap stage dropped still merges) */
	const sdt_read_merge wrong[] = {{200, 3, 4, 0, 0, 5}, {200, 3, 1, 0, 0, 0}, {200, 3, 1, 0, 0, 2}, {200, 3, 1, 1, 0, 5}, {200, 3, 1, 0, 150, 5},
	                                {199, 3, 1, 0, 0, 5}, {200, 151, 1, 0, 0, 5}, {0, 1, 0, 0, 150, 0}, {0, 0, 1, 0, 150, 0}, {0, 0, 0, 0, 150, 5},
	                                {0, 0, 0, 0, 149, 0}, {0, 0, 0, 1, 150, 0}, {0, 0, 0, 0, 150, 2}};
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_merge_record_ok(wrong + i, &ov200, 150) == 0);
	CHECK(sdt_merge_record_ok(&m100, &ovnone, 150) == 0);                                                         /* merged without an overlap */
	const sdt_read_merge one = {1, 1, 0, 0, 0, 5}, two_of_one = {1, 2, 0, 0, 0, 5};
	const sdt_read_overlap ov1 = {1, 1, 1, 0, 1, 0};
	CHECK(sdt_merge_record_ok(&one, &ov1, 1) == 1 && sdt_merge_record_ok(&two_of_one, &ov1, 150) == 0);

	/* the statistics: no pairs */
	sdt_merge_stats s;
	char buf[256];
	memset(&s, 0, sizeof s);
	sdt_merge_summary(buf, sizeof buf, &s, 0, 0, 0);
	CHECK(strcmp(buf, "merge: reads 0 pairs 0 overlapping 0 merged 0 mismatch columns 0 bases in 0 bases out 0") == 0);
	/* a pair without overlap, an overlapping pair kept apart, two merged pairs */
	CHECK(sdt_merge_stats_note(&s, &whole, &whole, &ovnone, &ovnone) == 0 && s.pairs == 1 && s.overlapping == 0 && s.merged == 0);
	CHECK(sdt_merge_stats_note(&s, &kept100, &kept100, &ov100, &ov100) == 0 && s.pairs == 2 && s.overlapping == 1 && s.merged == 0);
	CHECK(sdt_merge_stats_note(&s, &m200, &m200, &ov200, &ov200) == 0 && s.merged == 1 && s.columns == 3 && s.from_b == 1 && s.merged_bases == 200);
	CHECK(sdt_merge_stats_note(&s, &m50, &m50, &ovdrop, &ovdrop) == 0 && s.merged == 2 && s.columns == 3 && s.merged_bases == 250);
	CHECK(s.pairs == 4 && s.overlapping == 3);
	const int n = sdt_merge_summary(buf, sizeof buf, &s, 9, 1132, 500);
	CHECK(strcmp(buf, "merge: reads 9 pairs 4 overlapping 3 merged 2 mismatch columns 3 bases in 1132 bases out 750") == 0 && n == (int)strlen(buf));
	/* a buffer that is too small is not overrun */
	char *tight = (char *)malloc(10);
	CHECK(sdt_merge_summary(tight, 10, &s, 9, 1132, 500) == n && strcmp(tight, "merge: re") == 0);
	free(tight);
	/* records that are not those of one pair: nothing is noted */
	CHECK(sdt_merge_stats_note(&s, &m200, &all_b, &ov200, &ov200) == -2);
	CHECK(sdt_merge_stats_note(&s, &m200, &whole, &ov200, &ov200) == -2);
	CHECK(sdt_merge_stats_note(&s, &m200, &m100, &ov200, &ov200) == -2);
	CHECK(sdt_merge_stats_note(&s, &m200, &m200, &ov200, &ov100) == -2);
	CHECK(sdt_merge_stats_note(&s, &m100, &m100, &ov200, &ov200) == -2);
	CHECK(s.pairs == 4 && s.merged == 2 && s.merged_bases == 250);
	/* counts past 2^32 */
	s.merged_bases = 0xFFFFFFFFFFULL;
	sdt_merge_summary(buf, sizeof buf, &s, 0x1FFFFFFFFULL, 0x3FFFFFFFFFFULL, 1);
	CHECK(strstr(buf, "reads 8589934591 ") && strstr(buf, "bases in 4398046511103 bases out 1099511627776") != NULL);
	if (failures) { fprintf(stderr, "merge_host_check: %d checks failed\n", failures); return 1; }
	printf("merge_host_check: ok\n");
	return 0;
}
