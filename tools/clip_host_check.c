/* clip_host_check.c -- the device-free host side of `sdt-kmers clip` (csrc/host/clipsplit.c) on synthetic input: adapter FASTA texts
 * into the packed adapter set (lower case, wrapped lines, blank lines, no newline at the end; an empty record, a bad letter, bases in
 * front of the first header and a record of 129 bases are refused with the file and the line, and leave the list as it was), what a
 * read's record line looks like, and the statistics of a stream's records.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o clip_host_check \
 *       tools/clip_host_check.c soapdenovo-trans_amd/csrc/host/clipsplit.c && ./clip_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/clipsplit.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static int base_at(const sdt_adapter_list *l, uint32_t i, uint64_t k)
{
	const uint64_t at = l->offsets[i] + k;
	return (int)((l->words[at >> 4] >> (30 - 2 * (at & 15))) & 3u);
}

/* the text in a malloc'ed block of exactly its length (no terminator): a parser that reads past the end is caught */
static int parse(sdt_adapter_list *l, const char *text, int end, char *err, size_t errlen)
{
	const size_t len = strlen(text);
	char *exact = (char *)malloc(len ? len : 1);
	memcpy(exact, text, len);
	err[0] = 0;
	const int rc = sdt_adapters_parse(l, exact, len, "ad.fa", end, err, errlen);
	free(exact);
	return rc;
}

int main(void)
{
	char err[256];
	sdt_adapter_list l;
	memset(&l, 0, sizeof l);
	/* A0 C1 T2 G3; lower case; a wrapped record; blank lines; \r\n; a name cut at the first blank; no newline at the end */
	CHECK(parse(&l, ">first adapter one\nACGT\nacgt\n\n>second\r\nTTTTTGGGGGCCCCCAAAAA\r\nAC\n\n>third\ng", 0, err, sizeof err) == 0);
	CHECK(l.n == 3 && l.offsets[0] == 0 && l.offsets[1] == 8 && l.offsets[2] == 30 && l.offsets[3] == 31);
	if (l.n == 3) {
		static const int want[8] = {0, 1, 3, 2, 0, 1, 3, 2};
		for (int k = 0; k < 8; k++) CHECK(base_at(&l, 0, (uint64_t)k) == want[k]);
		CHECK(base_at(&l, 1, 0) == 2 && base_at(&l, 1, 5) == 3 && base_at(&l, 1, 10) == 1 && base_at(&l, 1, 15) == 0 && base_at(&l, 1, 21) == 1);
		CHECK(base_at(&l, 2, 0) == 3);
		CHECK(strcmp(l.names[0], "first") == 0 && strcmp(l.names[1], "second") == 0 && strcmp(l.names[2], "third") == 0);
		CHECK(l.ends[0] == 0 && l.ends[1] == 0 && l.ends[2] == 0);
		CHECK((l.words[1] & 3u) == 0 && l.words[2] == 0);                        /* zero behind the last base */
	}
	/* a second file behind the first, as 5' adapters: a record of exactly 128 bases, wrapped */
	char big[400] = ">long\n";
	size_t nb = strlen(big);
	for (int i = 0; i < 128; i++) {
		big[nb++] = "ACGT"[i & 3];
		if (i % 50 == 49) big[nb++] = '\n';                                   /* lines 2 and 3 hold 50 bases, line 4 the last 28 */
	}
	big[nb] = 0;
	CHECK(parse(&l, big, 1, err, sizeof err) == 0);
	CHECK(l.n == 4 && l.offsets[4] == 31 + 128 && l.ends[3] == 1 && base_at(&l, 3, 127) == 2);
	const sdt_adapter_set set = sdt_adapters_set(&l);
	CHECK(set.n == 4 && set.words == l.words && set.offsets == l.offsets && set.ends == l.ends && set.reserved == 0);
	/* the refusals name the file and the line, and nothing of the text is appended */
	const uint32_t w0 = l.words[9], w1 = l.words[10];
	strcat(big, "A\n");                                                          /* 129 bases */
	static const struct { const char *text, *say; } bad[] = {
		{">ok\nACGT\n>empty\n>next\nAC\n", "ad.fa line 3: the record has no bases"},
		{">ok\nACGT\n>n\nACNT\n", "ad.fa line 4: 'N' is not one of ACGT"},
		{">ok\nAC GT\n", "ad.fa line 2: ' ' is not one of ACGT"},
		{"ACGT\n>late\nAC\n", "ad.fa line 1: bases before the first '>' line"},
		{">ok\nACGT\n>last\n", "ad.fa line 3: the record has no bases"},
	};
	for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
		CHECK(parse(&l, bad[i].text, 0, err, sizeof err) == -1);
		CHECK(strcmp(err, bad[i].say) == 0);
		CHECK(l.n == 4 && l.offsets[4] == 159 && l.words[9] == w0 && l.words[10] == w1);
	}
	CHECK(parse(&l, big, 0, err, sizeof err) == -1 && strcmp(err, "ad.fa line 4: the record has more than 128 bases") == 0 && l.n == 4);
	/* the list still takes records, where the refused ones would have gone */
	CHECK(parse(&l, ">again\nTT\n", 1, err, sizeof err) == 0 && l.n == 5 && l.offsets[5] == 161 && base_at(&l, 4, 0) == 2 && base_at(&l, 4, 1) == 2);
	CHECK(base_at(&l, 3, 127) == 2);
	/* 256 adapters in all, not one more */
	sdt_adapter_list many;
	memset(&many, 0, sizeof many);
	char *text = (char *)malloc(257 * 16 + 1);
	text[0] = 0;
	for (int i = 0; i < 257; i++) sprintf(text + strlen(text), ">a%d\nACGTA\n", i);
	CHECK(parse(&many, text, 0, err, sizeof err) == -1 && strstr(err, "more than 256 adapters") != NULL && many.n == 0);
	text[strlen(text) - strlen(">a256\nACGTA\n")] = 0;
	CHECK(parse(&many, text, 0, err, sizeof err) == 0 && many.n == 256 && many.offsets[256] == 5 * 256);
	CHECK(parse(&many, ">one more\nAC\n", 1, err, sizeof err) == -1 && many.n == 256);
	free(text);
	sdt_adapters_free(&many);
	CHECK(many.words == NULL && many.n == 0);
	CHECK(sdt_adapters_load(&many, "/nonexistent/adapters.fa", 0, err, sizeof err) == -1 && strstr(err, "cannot open") != NULL);

	/* the record line: the widest fields fill the promised size exactly */
	char *line = (char *)malloc(SDT_CLIP_LINE_MAX);
	const sdt_read_clip widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_clip_line(line, &widest);
	CHECK(end - line == 2 * 6 + 5 * 11 && memcmp(line, "65535 65535 4294967295 4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	CHECK(end - line <= SDT_CLIP_LINE_MAX);
	const sdt_read_clip some = {3u | 10u << 16, 20, 9, 21, 70, 2};
	end = sdt_put_clip_line(line, &some);
	CHECK(end - line == 18 && memcmp(line, "3 10 20 9 21 70 2\n", 18) == 0);
	free(line);

	/* the statistics of six reads under the five adapters above */
	sdt_clip_stats s;
	CHECK(sdt_clip_stats_init(&s, l.n) == 0);
	const sdt_read_clip recs[6] = {{0, 0, 0, 0, 100, 0}, {1, 0, 0, 0, 60, 2}, {1u | 4u << 16, 10, 5, 17, 50, 2}, {2, 0, 0, 0, 0, 3},
	                               {0, 90, 0, 0, 0, 3}, {5u << 16, 0, 0, 2, 98, 2}};
	const uint64_t lens[6] = {100, 100, 100, 40, 90, 100};
	for (int i = 0; i < 6; i++) CHECK(sdt_clip_stats_note(&s, recs + i, lens[i]) == 0);
	CHECK(s.reads[0] == 2 && s.bases[0] == 40 + 23 && s.reads[1] == 1 && s.bases[1] == 0 && s.reads[3] == 1 && s.bases[3] == 12);
	CHECK(s.reads[4] == 1 && s.bases[4] == 2 && s.reads[2] == 0);
	CHECK(s.tail_reads[0] == 2 && s.tail_bases[0] == 100 && s.tail_reads[1] == 1 && s.tail_bases[1] == 5);
	CHECK(s.whole == 1 && s.clipped == 3 && s.dropped == 2);
	/* records that no read of that length and no set of five adapters has */
	const sdt_read_clip wrong[6] = {{6, 0, 0, 0, 50, 2}, {0, 0, 0, 0, 50, 1}, {0, 0, 0, 60, 50, 2}, {0, 0, 0, 0, 0, 2}, {0, 0, 0, 0, 99, 0}, {0, 0, 0, 1, 5, 3}};
	for (int i = 0; i < 6; i++) CHECK(sdt_clip_stats_note(&s, wrong + i, 100) == -1);
	CHECK(s.whole == 1 && s.clipped == 3 && s.dropped == 2);
	FILE *f = tmpfile();
	CHECK(f != NULL);
	if (f) {
		CHECK(sdt_clip_stats_write(f, &s, &l) == 0);
		char got[512];
		rewind(f);
		const size_t n = fread(got, 1, sizeof got - 1, f);
		got[n] = 0;
		fclose(f);
		CHECK(strcmp(got, "1 first 3 2 63\n2 second 3 1 0\n3 third 3 0 0\n4 long 5 1 12\n5 again 5 1 2\ntail3 2 100\ntail5 1 5\nwhole 1\nclipped 3\ndropped 2\n") == 0);
	}
	sdt_clip_stats_free(&s);
	sdt_adapters_free(&l);
	if (failures) { fprintf(stderr, "clip_host_check: %d checks failed\n", failures); return 1; }
	printf("clip_host_check: ok\n");
	return 0;
}
