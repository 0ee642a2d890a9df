/* cmp_host_check.c -- the device-free half of `sdt-kmers compare` on its own (tests/test_table_compare_host.py builds it with
 * -fsanitize=address,undefined and runs it): the matrix file with its R+ / C+ labels, the solid counts taken from the matrix, the
 * summary line with its zero denominators, the --select text, and the k-mer list with its order, its letters and its "# N matched"
 * line (cmpsplit.c).  Writes hand.cmpMatrix, hand.cmpKmers and hand.summary into the directory given, for the example that the test
 * works by hand.
 *   cc -std=gnu11 -fsanitize=address,undefined -o cmp_host_check tools/cmp_host_check.c soapdenovo-trans_amd/csrc/host/cmpsplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/cmpsplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "cmp_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

/* the whole of what `write` puts into a temporary file, as text (at most cap - 1 bytes) */
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
	if (argc != 2) { fprintf(stderr, "usage: cmp_host_check <directory>\n"); return 2; }
	char path[4096], line[SDT_CMP_SUMMARY_MAX], text[4096];
	FILE *f;
	/* the example by hand: five k-mers in A, five in B, three shared, one node of each counted 0 times; 3 x 3 */
	const uint64_t matrix[9] = {1, 1, 1, 1, 1, 0, 1, 0, 1};
	const uint64_t totals[8] = {5, 5, 3, 9, 11, 6, 8, 8};
	sdt_cmp_solid solid;
	CHECK(sdt_cmp_solid_of(matrix, 3, 3, 3, &solid) == -1 && sdt_cmp_solid_of(matrix, 3, 9, 3, &solid) == -1 && sdt_cmp_solid_of(matrix, 9, 3, 3, &solid) == -1);
	CHECK(sdt_cmp_solid_of(matrix, 3, 3, 2, &solid) == 0 && solid.solid_a == 2 && solid.solid_b == 2 && solid.solid_shared == 1);
	CHECK(sdt_cmp_solid_of(matrix, 3, 3, 1, &solid) == 0 && solid.solid_a == 4 && solid.solid_b == 4 && solid.solid_shared == 2);
	CHECK(sdt_cmp_solid_of(matrix, 3, 3, 0, &solid) == 0 && solid.solid_a == 7 && solid.solid_b == 7 && solid.solid_shared == 7);
	CHECK(sdt_cmp_solid_of(matrix, 3, 3, 2, &solid) == 0);
	sdt_cmp_summary(line, totals, &solid);
	CHECK(!strcmp(line, "compare: nodes_a 5 nodes_b 5 shared 3 solid_a 2 solid_b 2 solid_shared 1 jaccard_x10000 4285 contain_a_x10000 6000 "
	                    "contain_b_x10000 6000 braycurtis_x10000 4000\n"));
	snprintf(path, sizeof path, "%s/hand.summary", argv[1]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);
	snprintf(path, sizeof path, "%s/hand.cmpMatrix", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_cmp_matrix_write(f, matrix, 3, 3) == 0 && fclose(f) == 0);
	/* K = 3: ACG = 0b000111, AAC = 1, TTT = 0b101010, GCA = 0b110100; given out of order, written ascending */
	const uint64_t keys[4] = {0x2A, 0x07, 0x34, 0x01};
	const uint32_t ca[4] = {1, 2, 70000, 4}, cb[4] = {0, 0, 4000000000u, 9};
	snprintf(path, sizeof path, "%s/hand.cmpKmers", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_cmp_kmers_write(f, keys, ca, cb, 4, 1, 3, 4) == 0 && fclose(f) == 0);

	/* the labels of a matrix that is not square: the last row is R+, the last column C+, and nothing else carries a + */
	const uint64_t wide[8] = {0, 1, 2, 3, 4, 5, 6, 18446744073709551615ULL};
	CHECK((f = tmpfile()) && sdt_cmp_matrix_write(f, wide, 2, 4) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "a\\b 0 1 2 3+\n0 0 1 2 3\n1+ 4 5 6 18446744073709551615\n"));

	/* more matched than were listed: the last line says how many; none listed at all: that line alone */
	CHECK((f = tmpfile()) && sdt_cmp_kmers_write(f, keys, ca, cb, 2, 1, 3, 1000000000000ULL) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "ACG 2 0\nTTT 1 0\n# 1000000000000 matched\n"));
	CHECK((f = tmpfile()) && sdt_cmp_kmers_write(f, keys, ca, cb, 0, 1, 3, 7) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "# 7 matched\n"));
	CHECK((f = tmpfile()) && sdt_cmp_kmers_write(f, NULL, NULL, NULL, 0, 1, 3, 0) == 0 && ftell(f) == 0 && fclose(f) == 0);
	/* keys of two and four words order by their most significant word first; K = 33: the first letter is the low pair of word 0 */
	const uint64_t k2[6] = {1, 0, 0, 0xFFFFFFFFFFFFFFFFULL, 0, 1};
	const uint32_t one[3] = {1, 2, 3};
	CHECK((f = tmpfile()) && sdt_cmp_kmers_write(f, k2, one, one, 3, 2, 33, 3) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC 3 3\nAGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG 2 2\nCAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA 1 1\n"));
	uint64_t k4[8] = {0, 0, 0, 2, 0, 0, 0, 1};
	k4[0] = 3ULL << 60;                                      /* K = 127: the first letter is bits 61..60 of word 0 */
	CHECK((f = tmpfile()) && sdt_cmp_kmers_write(f, k4, one, one, 2, 4, 127, 2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(strlen(text) == 2 * (127 + 5) && text[126] == 'C' && text[127] == ' ' && text[132] == 'G' && text[132 + 126] == 'T');

	/* zero denominators: nothing in either table; nothing shared; an empty B */
	const uint64_t none[8] = {0}, apart[8] = {3, 2, 0, 30, 20, 0, 0, 0}, empty_b[8] = {4, 0, 0, 12, 0, 0, 0, 0}, same[8] = {4, 4, 4, 12, 12, 12, 12, 12};
	const sdt_cmp_solid z = {0, 0, 0};
	sdt_cmp_summary(line, none, &z);
	CHECK(strstr(line, "shared 0 solid_a 0 solid_b 0 solid_shared 0 jaccard_x10000 0 contain_a_x10000 0 contain_b_x10000 0 braycurtis_x10000 0\n"));
	sdt_cmp_summary(line, apart, &z);
	CHECK(strstr(line, "jaccard_x10000 0 contain_a_x10000 0 contain_b_x10000 0 braycurtis_x10000 10000\n"));
	sdt_cmp_summary(line, empty_b, &z);
	CHECK(strstr(line, "nodes_a 4 nodes_b 0 shared 0") && strstr(line, "contain_b_x10000 0 braycurtis_x10000 10000\n"));
	sdt_cmp_summary(line, same, &z);
	CHECK(strstr(line, "jaccard_x10000 10000 contain_a_x10000 10000 contain_b_x10000 10000 braycurtis_x10000 0\n"));
	/* sums that do not fit 64 bits once multiplied by 10000 */
	const uint64_t big[8] = {1ULL << 62, 1ULL << 62, 1ULL << 61, 1ULL << 63, 1ULL << 62, 1ULL << 61, 0, 0};
	sdt_cmp_summary(line, big, &z);
	CHECK(strstr(line, "jaccard_x10000 3333 contain_a_x10000 5000 contain_b_x10000 5000 braycurtis_x10000 6666\n"));

	/* --select */
	uint32_t rg[4];
	CHECK(sdt_cmp_parse_select("2:4294967295:0:0", rg) == 0 && rg[0] == 2 && rg[1] == 4294967295u && rg[2] == 0 && rg[3] == 0);
	CHECK(sdt_cmp_parse_select("0:0:7:7", rg) == 0 && rg[2] == 7 && rg[3] == 7);
	const char *bad[] = {"", "1:2:3", "1:2:3:4:5", "1:2:3:", ":1:2:3", "1:2:3:x", "2:1:0:0", "1:2:4:3", "1:4294967296:0:0", "-1:2:0:0", "1 :2:0:0", "1:2:0:0 "};
	for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) CHECK(sdt_cmp_parse_select(bad[i], rg) == -1);
	printf("cmp_host_check: ok\n");
	return 0;
}
