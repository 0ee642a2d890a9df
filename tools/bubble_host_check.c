/* bubble_host_check.c -- the device-free half of `sdt-kmers bubbles` on its own (tests/test_bubbles_host.py builds it with
 * -fsanitize=address,undefined and runs it): the lines of prefix.bubbles, the records of prefix.bubbles.fa and the summary line
 * (bubblesplit.c) from arrays made by hand, for 1, 2 and 4 key words, in pieces, and for no bubble at all.  Writes hand.bubbles,
 * hand.bubbles.fa and hand.summary into the directory given, for the example that the test works by hand.
 *   cc -std=gnu11 -fsanitize=address,undefined -o bubble_host_check tools/bubble_host_check.c soapdenovo-trans_amd/csrc/host/bubblesplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/bubblesplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bubble_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

/* the whole of what was written into a temporary file, as text (at most cap - 1 bytes) */
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
	if (argc != 2) { fprintf(stderr, "usage: bubble_host_check <directory>\n"); return 2; }
	char path[4096], line[SDT_BUBBLE_SUMMARY_MAX], text[8192];
	FILE *f;
	/* the example by hand, K = 3: a substitution ACG -> (A|T) .. -> GTA with three inner nodes a side; a direct edge against two inner
	 * nodes; a large sum.  The two files are written in two pieces, as the tool does */
	const uint64_t keys[6] = {0x07, 0x38, 0x12, 0x09, 0x2A, 0x15};
	const sdt_bubble rec[3] = {{21, 9, 3, 3, 7, 2, 8, 9, 0 | 2 << 2 | 7 << 8 | 2 << 16, 0},
	                           {0, 11, 0, 2, 0, 5, 6, 6, 1 | 3 << 2 | 6 << 8 | 5 << 16, 0},
	                           {5000000000ULL, 8, 2, 2, 4000000000u, 4, 4294967295u, 1, 0 | 1 << 2 | 63 << 8 | 1 << 16, 0}};
	const uint8_t bases[] = {0, 3, 2, 0, 2, 3, 2, 0, 1, 3, 1, 2, 0, 0, 3, 1, 1, 1};
	const uint64_t offs[7] = {0, 4, 8, 9, 12, 15, 18}, offs2[3] = {0, 3, 6};
	const uint64_t info[8] = {40, 6, 13, 12, 3, 18, 3, 0};
	uint64_t kinds[3] = {0, 0, 0};
	snprintf(path, sizeof path, "%s/hand.bubbles", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_bubble_list_write(f, keys, rec, 0, 2, 1, 3, kinds) == 0 && sdt_bubble_list_write(f, keys + 4, rec + 2, 2, 1, 1, 3, kinds) == 0 &&
	      fclose(f) == 0);
	CHECK(kinds[0] == 1 && kinds[1] == 1 && kinds[2] == 1);
	snprintf(path, sizeof path, "%s/hand.bubbles.fa", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_bubble_fasta_write(f, keys, rec, bases, offs, 0, 2, 1, 3) == 0 &&
	      sdt_bubble_fasta_write(f, keys + 4, rec + 2, bases + 12, offs2, 2, 1, 1, 3) == 0 && fclose(f) == 0);
	sdt_bubble_summary(line, info, kinds);
	CHECK(!strcmp(line, "bubbles: live 40 forks 6 branches 13 reached 12 bubbles 3 kind0 1 kind1 1 kind2 1 longest 3\n"));
	snprintf(path, sizeof path, "%s/hand.summary", argv[1]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);

	/* keys of two and four words: most significant word first; K = 33: the first letter is the low pair of word 0 */
	const uint64_t k2[4] = {0, 1, 1, 0};
	const sdt_bubble r2[1] = {{66, 66, 33, 33, 2, 2, 4, 4, 1 | 2 << 2 | 2 << 8 | 2 << 16, 0}};
	uint64_t kd[3] = {0, 0, 0};
	CHECK((f = tmpfile()) && sdt_bubble_list_write(f, k2, r2, 41, 1, 2, 33, kd) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "42 AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC CAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA C T 33 33 2 2 66 66 2 2 0\n") && kd[0] == 1);
	uint64_t k4[8] = {0, 0, 0, 2, 0, 0, 0, 1};
	k4[4] = 3ULL << 60;                                      /* K = 127: the first letter is bits 61..60 of word 0 */
	CHECK((f = tmpfile()) && sdt_bubble_list_write(f, k4, r2, 0, 1, 4, 127, kd) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(text[2 + 126] == 'T' && text[2 + 127] == ' ' && text[2 + 128] == 'G' && kd[1] == 1);

	/* a path longer than the writer's buffer, every letter kept */
	enum { LONG = 10000 };
	uint8_t *lb = (uint8_t *)malloc(2 * LONG);
	CHECK(lb != NULL);
	for (int i = 0; i < 2 * LONG; i++) lb[i] = (uint8_t)(i % 3);
	const uint64_t lo[3] = {0, LONG, 2 * LONG};
	const sdt_bubble lr[1] = {{1, 1, LONG - 1, LONG - 1, 1, 1, 1, 1, 0 | 1 << 2, 0}};
	char *big = (char *)malloc(2 * LONG + 256);
	CHECK(big && (f = tmpfile()) && sdt_bubble_fasta_write(f, keys, lr, lb, lo, 0, 1, 1, 3) == 0 && slurp(f, big, 2 * LONG + 256) == 0 && fclose(f) == 0);
	const char *seq = strchr(big, '\n');
	CHECK(seq && strlen(seq + 1) > LONG && !strncmp(seq + 1, "ACGACTACT", 9) && seq[1 + 3 + LONG] == '\n' && seq[3 + LONG] == "ACT"[(LONG - 1) % 3]);
	free(lb); free(big);

	/* no bubble at all */
	const uint64_t i0[8] = {5, 0, 0, 0, 0, 0, 0, 0};
	uint64_t k0[3] = {0, 0, 0};
	CHECK((f = tmpfile()) && sdt_bubble_list_write(f, NULL, NULL, 0, 0, 1, 3, k0) == 0 && sdt_bubble_fasta_write(f, NULL, NULL, NULL, offs, 0, 0, 1, 3) == 0 &&
	      slurp(f, text, sizeof text) == 0 && fclose(f) == 0 && text[0] == 0);
	sdt_bubble_summary(line, i0, k0);
	CHECK(!strcmp(line, "bubbles: live 5 forks 0 branches 0 reached 0 bubbles 0 kind0 0 kind1 0 kind2 0 longest 0\n"));
	printf("bubble_host_check: ok\n");
	return 0;
}
