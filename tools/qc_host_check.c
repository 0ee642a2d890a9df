/* qc_host_check.c -- the device-free half of `sdt-kmers qc` (csrc/host/qcsplit.c) on hand-made reports, as a stand-alone program under
 * sanitizers (tests/test_read_qc_host.py): the percentile at ties and at its ends, rows without a base, the C+ row, a class without
 * qualities, a class without reads, the summary line, and a file that cannot be written (/dev/full).  argv[1]: a directory to write in. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/qcsplit.h"

#define CHECK(cond)                                                                      \
	do {                                                                                 \
		if (!(cond)) {                                                                   \
			fprintf(stderr, "qc_host_check: %s (line %d)\n", #cond, __LINE__);           \
			exit(1);                                                                     \
		}                                                                                \
	} while (0)

enum { C = 3, R = C + 1 };

static char *slurp(const char *path)
{
	static char buf[1 << 16];
	FILE *f = fopen(path, "r");
	CHECK(f);
	const size_t n = fread(buf, 1, sizeof buf - 1, f);
	buf[n] = 0;
	fclose(f);
	return buf;
}

int main(int argc, char **argv)
{
	CHECK(argc == 2);
	CHECK(sdt_qc_words(C) == 203 + 99 * R && sdt_qc_words(1) == 401 && sdt_qc_words(4096) == 405806);
	/* the percentile: the smallest q whose cumulative count is >= ceil(p N / 100) */
	uint64_t h[SDT_QC_NQ] = {0};
	h[2] = 1; h[10] = 1; h[20] = 1; h[30] = 1;                               /* N = 4: 10 % -> 1st, 25 % -> 1st, 50 % -> 2nd, 75 % -> 3rd, 90 % -> 4th */
	CHECK(sdt_qc_percentile(h, 4, 0) == 2 && sdt_qc_percentile(h, 4, 10) == 2 && sdt_qc_percentile(h, 4, 25) == 2 && sdt_qc_percentile(h, 4, 26) == 10);
	CHECK(sdt_qc_percentile(h, 4, 50) == 10 && sdt_qc_percentile(h, 4, 51) == 20 && sdt_qc_percentile(h, 4, 75) == 20 && sdt_qc_percentile(h, 4, 90) == 30);
	CHECK(sdt_qc_percentile(h, 4, 100) == 30);
	memset(h, 0, sizeof h);
	h[7] = 5; h[93] = 5;                                                     /* a tie at the median: the cumulative count reaches 5 at q = 7 */
	CHECK(sdt_qc_percentile(h, 10, 50) == 7 && sdt_qc_percentile(h, 10, 51) == 93 && sdt_qc_percentile(h, 10, 100) == 93);
	memset(h, 0, sizeof h);
	h[0] = 1;
	CHECK(sdt_qc_percentile(h, 1, 10) == 0 && sdt_qc_percentile(h, 1, 90) == 0);
	memset(h, 0, sizeof h);
	h[40] = 0xFFFFFFFFFFull; h[41] = 1;                                      /* counts past 2^32: no product overflows */
	CHECK(sdt_qc_percentile(h, 0x10000000000ull, 90) == 40 && sdt_qc_percentile(h, 0x10000000000ull, 100) == 41);

	/* class 0: 3 reads of 1, 2 and 6 bases with qualities (row 3 = C+ holds 3 bases), one empty read; row 2 is reached by one read.
	 * class 1: no read.  class 2: 2 reads of 1 base from a FASTA file */
	static uint64_t r0[203 + 99 * R], r2[203 + 99 * R];
	uint64_t *base = r0 + 8, *qual = base + 4 * R, *len = qual + SDT_QC_NQ * R, *gc = len + R, *meanq = gc + SDT_QC_NGC;
	r0[0] = 4; r0[1] = 1; r0[2] = 9;
	base[0 * 4 + 0] = 2; base[0 * 4 + 1] = 1;                                /* row 0: A A C */
	base[1 * 4 + 3] = 2;                                                     /* row 1: G G */
	base[2 * 4 + 2] = 1;                                                     /* row 2: T */
	base[3 * 4 + 1] = 3;                                                     /* row 3+: C C C */
	qual[0 * SDT_QC_NQ + 30] = 2; qual[0 * SDT_QC_NQ + 2] = 1;
	qual[1 * SDT_QC_NQ + 20] = 1; qual[1 * SDT_QC_NQ + 21] = 1;
	qual[2 * SDT_QC_NQ + 40] = 1;
	qual[3 * SDT_QC_NQ + 0] = 1; qual[3 * SDT_QC_NQ + 93] = 2;
	len[0] = 1; len[1] = 1; len[2] = 1; len[3] = 1;
	gc[0] = 1; gc[50] = 1; gc[100] = 1;
	meanq[2] = 1; meanq[25] = 1; meanq[60] = 1;
	r2[0] = 2; r2[2] = 2;
	r2[8 + 0] = 1; r2[8 + 3] = 1;
	(r2 + 8 + 4 * R + SDT_QC_NQ * R)[1] = 2;
	(r2 + 8 + 4 * R + SDT_QC_NQ * R + R)[0] = 1;
	(r2 + 8 + 4 * R + SDT_QC_NQ * R + R)[100] = 1;
	const sdt_qc_class cls[SDT_QC_CLASSES] = {{r0, 3}, {NULL, 0}, {r2, 0}};

	char path[4200];
	snprintf(path, sizeof path, "%s/qc.bases", argv[1]);
	FILE *f = fopen(path, "w");
	CHECK(f && sdt_qc_bases_write(f, cls, C) == 0 && fclose(f) == 0);
	CHECK(strcmp(slurp(path), "# class row reads A C T G\n0 0 3 2 1 0 0\n0 1 2 0 0 0 2\n0 2 1 0 0 1 0\n0 3+ 3 0 3 0 0\n2 0 2 1 0 0 1\n") == 0);
	snprintf(path, sizeof path, "%s/qc.quals", argv[1]);
	f = fopen(path, "w");
	CHECK(f && sdt_qc_quals_write(f, cls, C) == 0 && fclose(f) == 0);
	CHECK(strcmp(slurp(path), "# class row bases mean_x100 min q10 q25 median q75 q90 max\n"
	                          "0 0 3 2066 2 2 2 30 30 30 30\n0 1 2 2050 20 20 20 20 21 21 21\n0 2 1 4000 40 40 40 40 40 40 40\n"
	                          "0 3+ 3 6200 0 0 0 93 93 93 93\n# class 2: no qualities\n") == 0);
	snprintf(path, sizeof path, "%s/qc.reads", argv[1]);
	f = fopen(path, "w");
	CHECK(f && sdt_qc_reads_write(f, cls, C) == 0 && fclose(f) == 0);
	CHECK(strcmp(slurp(path), "# hist class bin reads\nlen 0 0 1\nlen 0 1 1\nlen 0 2 1\nlen 0 3+ 1\nlen 2 1 2\n"
	                          "gc 0 0 1\ngc 0 50 1\ngc 0 100 1\ngc 2 0 1\ngc 2 100 1\n"
	                          "meanq 0 2 1\nmeanq 0 25 1\nmeanq 0 60 1\n# meanq class 2: no qualities\n") == 0);
	char line[SDT_QC_LINE_MAX];
	sdt_qc_summary(line, 0, &cls[0], C);
	CHECK(strcmp(line, "qc: class 0 reads 4 empty 1 bases 9 gc 6666 q20 7777 q30 5555\n") == 0);
	sdt_qc_summary(line, 2, &cls[2], C);
	CHECK(strcmp(line, "qc: class 2 reads 2 empty 0 bases 2 gc 5000 q20 - q30 -\n") == 0);
	/* a report without a read: headers only, and a summary that divides by nothing */
	static uint64_t none[203 + 99 * R];
	const sdt_qc_class empty[SDT_QC_CLASSES] = {{NULL, 0}, {none, 0}, {NULL, 0}};
	f = fopen(path, "w");
	CHECK(f && sdt_qc_bases_write(f, empty, C) == 0 && fclose(f) == 0);
	CHECK(strcmp(slurp(path), "# class row reads A C T G\n") == 0);
	sdt_qc_summary(line, 1, &empty[1], C);
	CHECK(strcmp(line, "qc: class 1 reads 0 empty 0 bases 0 gc 0 q20 - q30 -\n") == 0);
	/* a file that cannot be written: the writer or the close says so */
	for (int i = 0; i < 3; i++) {
		f = fopen("/dev/full", "w");
		CHECK(f);
		const int w = i == 0 ? sdt_qc_bases_write(f, cls, C) : i == 1 ? sdt_qc_quals_write(f, cls, C) : sdt_qc_reads_write(f, cls, C);
		CHECK((w != 0) | (fclose(f) != 0));
	}
	printf("qc_host_check: ok\n");
	return 0;
}
