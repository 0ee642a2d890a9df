/* screen_host_check.c -- the device-free host side of `sdt-kmers screen` (csrc/host/screensplit.c) on synthetic input: the FASTA reader
 * on wrapped, lower-case, N-cut, empty and malformed texts and on a file; the packed words; what a read's record line looks like;
 * which records can be those of a read of a given length; the statistics per reference with their summary line.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o screen_host_check \
 *       tools/screen_host_check.c soapdenovo-trans_amd/csrc/host/screensplit.c && ./screen_host_check [a directory for one small file] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/screensplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* the text in a block of exactly its length, so that a read past its end is seen */
static int parse(sdt_ref_set *s, const char *label, const char *text, char *err, size_t errcap)
{
	const size_t n = strlen(text);
	char *exact = (char *)malloc(n ? n : 1);
	memcpy(exact, text, n);
	const int rc = sdt_refs_parse(s, label, exact, n, err, errcap);
	free(exact);
	return rc;
}

/* segment j as letters */
static int segment_is(const sdt_ref_set *s, uint64_t j, const char *want)
{
	const uint64_t n = s->offsets[j + 1] - s->offsets[j];
	if (n != strlen(want)) return 0;
	for (uint64_t i = 0; i < n; i++) {
		const uint64_t at = s->offsets[j] + i;
		if ("ACTG"[(s->words[at >> 4] >> (30 - 2 * (at & 15))) & 3] != want[i]) return 0;
	}
	return 1;
}

static char *written(const sdt_screen_stats *st, const sdt_ref_set *refs)
{
	FILE *f = tmpfile();
	if (!f) return NULL;
	CHECK(sdt_screen_stats_write(f, st, refs) == 0);
	const long n = ftell(f);
	rewind(f);
	char *got = (char *)malloc((size_t)n + 1);
	CHECK(fread(got, 1, (size_t)n, f) == (size_t)n);
	got[n] = 0;
	fclose(f);
	return got;
}

int main(int argc, char **argv)
{
	char err[256];
	sdt_ref_set s;
	memset(&s, 0, sizeof s);
	/* wrapped lines, lower case, blank lines, '\r', a name cut at the first blank, N and other letters cutting a reference, a reference
	 * of N alone, a last line without a newline; then a second text appended */
	CHECK(parse(&s, "a.fa", ">one first reference\nACGT\nacgt\n\nAC\r\n>two\tx\nAAAANNCCCCnGGGGRTTTT\n>onlyN\nNNNN\n>last\nGATTACA", err, sizeof err) == 0);
	CHECK(parse(&s, "b.fa", ">more\nT\n", err, sizeof err) == 0);
	CHECK(sdt_refs_pack(&s) == 0);
	CHECK(s.n_refs == 5 && s.nseqs == 7 && s.ncodes == 10 + 16 + 7 + 1 && s.nwords == (s.ncodes + 15) / 16 + 4);
	CHECK(strcmp(s.names[0], "one") == 0 && strcmp(s.names[1], "two") == 0 && strcmp(s.names[2], "onlyN") == 0 && strcmp(s.names[3], "last") == 0 &&
	      strcmp(s.names[4], "more") == 0);
	CHECK(s.bases[0] == 10 && s.bases[1] == 16 && s.bases[2] == 0 && s.bases[3] == 7 && s.bases[4] == 1);
	const uint32_t want_ref[] = {0, 1, 1, 1, 1, 3, 4};
	for (int j = 0; j < 7; j++) CHECK(s.ref_of_seq[j] == want_ref[j]);
	CHECK(segment_is(&s, 0, "ACGTACGTAC") && segment_is(&s, 1, "AAAA") && segment_is(&s, 2, "CCCC") && segment_is(&s, 3, "GGGG") && segment_is(&s, 4, "TTTT"));
	CHECK(segment_is(&s, 5, "GATTACA") && segment_is(&s, 6, "T") && s.offsets[0] == 0 && s.offsets[7] == s.ncodes);
	for (uint64_t w = (s.ncodes + 15) / 16; w < s.nwords; w++) CHECK(s.words[w] == 0);                  /* the pad words */
	sdt_refs_free(&s);

	/* an empty text and a text of blank lines: no reference, and pack still gives offsets and the pad */
	CHECK(parse(&s, "e.fa", "", err, sizeof err) == 0 && parse(&s, "e.fa", "\n\n  \n", err, sizeof err) == 0);
	CHECK(sdt_refs_pack(&s) == 0 && s.n_refs == 0 && s.nseqs == 0 && s.offsets[0] == 0 && s.nwords == 4);
	sdt_refs_free(&s);

	/* many references and long ones: the arrays grow */
	{
		const size_t cap = 400000;
		char *big = (char *)malloc(cap);
		size_t n = 0;
		for (int r = 0; r < 300; r++) {
			n += (size_t)sprintf(big + n, ">r%d\n", r);
			for (int i = 0; i < 1000 + r; i++) big[n++] = (i % 97 == 96) ? 'N' : "ACGT"[(i * 7 + r) & 3];
			big[n++] = '\n';
		}
		CHECK(n < cap && sdt_refs_parse(&s, "big.fa", big, n, err, sizeof err) == 0 && sdt_refs_pack(&s) == 0);
		CHECK(s.n_refs == 300 && strcmp(s.names[299], "r299") == 0);
		uint64_t bases = 0, in_segments = 0;
		for (uint32_t r = 0; r < 300; r++) bases += s.bases[r];
		for (uint64_t j = 0; j < s.nseqs; j++) { in_segments += s.offsets[j + 1] - s.offsets[j]; CHECK(s.offsets[j + 1] - s.offsets[j] <= 96 && s.ref_of_seq[j] < 300); }
		CHECK(bases == s.ncodes && in_segments == s.ncodes && s.nseqs > 3000);
		free(big);
		sdt_refs_free(&s);
	}

	/* malformed: bases before the first header; a record without any sequence character, in the middle and at the end; what was read
	 * before stays valid and is freed */
	CHECK(parse(&s, "x.fa", "\nACGT\n>a\nAC\n", err, sizeof err) == -1 && strcmp(err, "x.fa line 2: bases before the first header") == 0);
	CHECK(parse(&s, "y.fa", ">a\nACGT\n>b\n\n>c\nAC\n", err, sizeof err) == -1 && strcmp(err, "y.fa line 3: the record has no sequence") == 0);
	CHECK(parse(&s, "z.fa", ">a\nACGT\n>b", err, sizeof err) == -1 && strcmp(err, "z.fa line 3: the record has no sequence") == 0);
	CHECK(parse(&s, "w.fa", ">\n", err, sizeof err) == -1 && strcmp(err, "w.fa line 1: the record has no sequence") == 0);
	sdt_refs_free(&s);
	CHECK(sdt_refs_load(&s, "/nonexistent/refs.fa", err, sizeof err) == -1 && strcmp(err, "cannot read /nonexistent/refs.fa") == 0);
	/* a file */
	{
		char path[4200];
		snprintf(path, sizeof path, "%s/screen_host_check.fa", argc > 1 ? argv[1] : ".");      /* (argv[1]: a directory to write it in) */
		FILE *f = fopen(path, "w");
		CHECK(f != NULL);
		if (f) {
			fputs(">f1 x\nACGTN\nACG\n", f);
			fclose(f);
			CHECK(sdt_refs_load(&s, path, err, sizeof err) == 0 && sdt_refs_pack(&s) == 0);
			CHECK(s.n_refs == 1 && s.nseqs == 2 && segment_is(&s, 0, "ACGT") && segment_is(&s, 1, "ACG") && s.bases[0] == 7);
			remove(path);
		}
	}

	/* the record line: the widest fields fill the promised size exactly; ref is 1-based, 0 for none */
	char *line = (char *)malloc(SDT_SCREEN_LINE_MAX);
	const sdt_read_screen widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_screen_line(line, &widest);
	CHECK(end - line == SDT_SCREEN_LINE_MAX && memcmp(line, "4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	const sdt_read_screen hit = {80, 37, 0, 0, 0, 1}, miss = {80, 0, SDT_SCREEN_NO_REF, 0, 100, 0};
	end = sdt_put_screen_line(line, &hit);
	CHECK(end - line == 10 && memcmp(line, "80 37 1 1\n", 10) == 0);
	end = sdt_put_screen_line(line, &miss);
	CHECK(end - line == 9 && memcmp(line, "80 0 0 0\n", 9) == 0);
	free(line);

	/* records that a read of 100 bases can have at k = 21 with 1 reference (the file above), and records that it cannot */
	const sdt_screen_params one = {1, 0, 0, 0}, strict = {40, 50, 0, 0}, bait = {1, 0, SDT_SCREEN_KEEP_MATCHED, 0};
	const sdt_read_screen kept_hit = {80, 37, 0, 0, 100, 0}, short_read = {0, 0, SDT_SCREEN_NO_REF, 0, 5, 0}, empty_read = {0, 0, SDT_SCREEN_NO_REF, 0, 0, 0};
	CHECK(sdt_screen_record_ok(&hit, 100, 21, 1) && sdt_screen_record_ok(&miss, 100, 21, 1) && sdt_screen_record_ok(&kept_hit, 100, 21, 1));
	CHECK(sdt_screen_record_ok(&short_read, 5, 21, 1) && sdt_screen_record_ok(&empty_read, 0, 21, 1) && sdt_screen_record_ok(&empty_read, 0, 11, 1));
	const sdt_read_screen wrong[] = {{79, 37, 0, 0, 0, 1}, {80, 81, 0, 0, 0, 1}, {80, 37, 1, 0, 0, 1}, {80, 37, SDT_SCREEN_NO_REF, 0, 0, 1}, {80, 0, 0, 0, 100, 0},
	                                 {80, 37, 0, 1, 100, 0}, {80, 37, 0, 0, 99, 0}, {80, 37, 0, 0, 100, 1}, {80, 37, 0, 0, 0, 0}, {80, 37, 0, 0, 0, 2}};
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_screen_record_ok(wrong + i, 100, 21, 1) == 0);
	CHECK(!sdt_screen_record_ok(&hit, 101, 21, 1) && !sdt_screen_record_ok(&hit, 100, 20, 1) && !sdt_screen_record_ok(&hit, 100, 21, 0));
	CHECK(sdt_screen_matched(&hit, &one) && !sdt_screen_matched(&miss, &one) && !sdt_screen_matched(&hit, &strict) && sdt_screen_matched(&hit, &bait));
	const sdt_read_screen forty = {80, 40, 0, 0, 0, 1}, thirty9 = {80, 39, 0, 0, 100, 0};
	CHECK(sdt_screen_matched(&forty, &strict) && !sdt_screen_matched(&thirty9, &strict));

	/* the statistics: an empty one, then reads of both verdicts; refused records leave it as it was */
	sdt_screen_stats st;
	CHECK(sdt_screen_stats_init(&st, s.n_refs) == 0);
	char *got = written(&st, &s);
	CHECK(got && strcmp(got, "1 f1 7 0 0\n# reads 0 matched 0 kept 0 dropped 0\n") == 0);
	free(got);
	CHECK(sdt_screen_stats_note(&st, &hit, 100, 21, &one) == 0 && sdt_screen_stats_note(&st, &miss, 100, 21, &one) == 0);
	CHECK(sdt_screen_stats_note(&st, &forty, 100, 21, &one) == 0 && sdt_screen_stats_note(&st, &short_read, 5, 21, &one) == 0);
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_screen_stats_note(&st, wrong + i, 100, 21, &one) == -2);
	CHECK(st.total == 4 && st.matched == 2 && st.kept == 2 && st.dropped == 2 && st.reads[0] == 2 && st.hits[0] == 77);
	got = written(&st, &s);
	CHECK(got && strcmp(got, "1 f1 7 2 77\n# reads 4 matched 2 kept 2 dropped 2\n") == 0);
	free(got);
	/* under stricter parameters the same records are matched less often: M comes from the records and the parameters */
	sdt_screen_stats_free(&st);
	CHECK(sdt_screen_stats_init(&st, s.n_refs) == 0);
	CHECK(sdt_screen_stats_note(&st, &kept_hit, 100, 21, &strict) == 0 && sdt_screen_stats_note(&st, &forty, 100, 21, &strict) == 0);
	CHECK(st.matched == 1 && st.kept == 1 && st.dropped == 1);
	sdt_screen_stats_free(&st);
	sdt_refs_free(&s);
	if (failures) { fprintf(stderr, "screen_host_check: %d checks failed\n", failures); return 1; }
	printf("screen_host_check: ok\n");
	return 0;
}
