/* support_host_check.c -- the device-free half of `sdt-kmers support` on its own (tests/test_unitig_support_host.py builds it with
 * -fsanitize=address,undefined and runs it): the lines of prefix.unitigSupport, prefix.linkSupport and prefix.junctions and the
 * summary line (supportsplit.c) from records in a file -- four uint64 (K, unitigs, links, junctions), the twelve totals, then the
 * unitig records, their tallies, the link records, their tallies and the junctions as the sdt_gpu_unitigs_* calls give them.  Writes
 * check.unitigSupport, check.linkSupport, check.junctions and check.summary into the directory given; before that a few cases by hand:
 * empty lists, a link that is left to its mirror, a list that is out of order or not in its reported form.
 *   cc -std=gnu11 -fsanitize=address,undefined -o support_host_check tools/support_host_check.c soapdenovo-trans_amd/csrc/host/supportsplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/supportsplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "support_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define LINK(u, o, v, o2, b) {u, v, (o) | (o2) << 1 | (b) << 2 | 5u << 8, 0}

static int slurp(FILE *f, char *buf, size_t cap)
{
	const long n = ftell(f);
	if (n < 0 || (size_t)n >= cap) return -1;
	rewind(f);
	if (fread(buf, 1, (size_t)n, f) != (size_t)n) return -1;
	buf[n] = 0;
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: support_host_check <records> <directory>\n"); return 2; }
	char path[4096], line[SDT_SUPPORT_SUMMARY_MAX], text[4096];
	FILE *f;
	/* by hand: two unitigs of 4 and 3 nodes; the floor of the coverage; unitig ids from `first` on */
	const sdt_unitig rec[2] = {{40, 4, 10, 10, 0}, {30, 3, 10, 10, 0}}, none = {0, 0, 0, 0, 0};
	const sdt_unitig_support us[2] = {{3, 10}, {0, 0}};
	CHECK((f = tmpfile()) && sdt_support_unitigs_write(f, rec, us, 5, 2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "6 3 10 250\n7 0 0 0\n"));
	CHECK((f = tmpfile()) && sdt_support_unitigs_write(f, &none, us, 0, 1) == -2 && sdt_support_unitigs_write(f, rec, us, 0, 0) == 0 && fclose(f) == 0);
	/* a link, its mirror (left to the first), and a self link that is its own mirror */
	const sdt_unitig_link links[3] = {LINK(0, 0, 1, 1, 2), LINK(1, 0, 0, 1, 3), LINK(1, 1, 1, 0, 0)};
	const sdt_link_support ls[3] = {{7, 2}, {2, 7}, {4, 4}};
	CHECK((f = tmpfile()) && sdt_support_links_write(f, links, ls, 3) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "1 + 2 - 7 2\n2 - 2 + 4 4\n"));
	/* junctions: in order; via with o = 1; out of order */
	const sdt_unitig_junction jn[3] = {{3, 0, 2, 0, 9}, {1, 2, 2, 0, 1}, {1, 2, 5, 0, 1ULL << 40}}, odd = {0, 1, 0, 0, 1}, back[2] = {{1, 2, 5, 0, 1}, {1, 2, 2, 0, 1}};
	CHECK((f = tmpfile()) && sdt_support_junctions_write(f, jn, 3) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "2- 1+ 2+ 9\n1- 2+ 2+ 1\n1- 2+ 3- 1099511627776\n"));
	CHECK((f = tmpfile()) && sdt_support_junctions_write(f, &odd, 1) == -2 && sdt_support_junctions_write(f, back, 2) == -2 && sdt_support_junctions_write(f, jn, 0) == 0 &&
	      fclose(f) == 0);
	const uint64_t t0[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
	sdt_support_summary(line, t0, 13);
	CHECK(!strcmp(line, "support: reads 1 placed 2 segments 3 kmers 4 traversals 5 no_record 6 passages 7 junctions 13 dropped 12\n"));

	/* the records of the file */
	uint64_t head[4], totals[12];
	FILE *in = fopen(argv[1], "rb");
	CHECK(in && fread(head, sizeof head[0], 4, in) == 4 && fread(totals, sizeof totals[0], 12, in) == 12);
	const uint64_t n = head[1], nl = head[2], nj = head[3];
	sdt_unitig *u = (sdt_unitig *)malloc((n ? n : 1) * sizeof *u);
	sdt_unitig_support *su = (sdt_unitig_support *)malloc((n ? n : 1) * sizeof *su);
	sdt_unitig_link *l = (sdt_unitig_link *)malloc((nl ? nl : 1) * sizeof *l);
	sdt_link_support *sl = (sdt_link_support *)malloc((nl ? nl : 1) * sizeof *sl);
	sdt_unitig_junction *j = (sdt_unitig_junction *)malloc((nj ? nj : 1) * sizeof *j);
	CHECK(u && su && l && sl && j);
	CHECK(fread(u, sizeof *u, n, in) == n && fread(su, sizeof *su, n, in) == n && fread(l, sizeof *l, nl, in) == nl && fread(sl, sizeof *sl, nl, in) == nl &&
	      fread(j, sizeof *j, nj, in) == nj && fgetc(in) == EOF && fclose(in) == 0);
	snprintf(path, sizeof path, "%s/check.unitigSupport", argv[2]);
	/* (in two pieces, as the tool fetches them) */
	CHECK((f = fopen(path, "w")) && sdt_support_unitigs_write(f, u, su, 0, n / 2) == 0 && sdt_support_unitigs_write(f, u + n / 2, su + n / 2, n / 2, n - n / 2) == 0 &&
	      fclose(f) == 0);
	snprintf(path, sizeof path, "%s/check.linkSupport", argv[2]);
	CHECK((f = fopen(path, "w")) && sdt_support_links_write(f, l, sl, nl) == 0 && fclose(f) == 0);
	snprintf(path, sizeof path, "%s/check.junctions", argv[2]);
	CHECK((f = fopen(path, "w")) && sdt_support_junctions_write(f, j, nj) == 0 && fclose(f) == 0);
	sdt_support_summary(line, totals, nj);
	snprintf(path, sizeof path, "%s/check.summary", argv[2]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);
	free(u); free(su); free(l); free(sl); free(j);
	printf("support_host_check: ok\n");
	return 0;
}
