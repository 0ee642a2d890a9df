/* unitig_host_check.c -- the device-free half of `sdt-kmers unitigs` on its own (tests/test_unitigs_host.py builds it with
 * -fsanitize=address,undefined and runs it): the lines of prefix.unitigs, prefix.unitigs.fa and prefix.unitigs.gfa and the summary
 * line (unitigsplit.c) from arrays made by hand, for 1, 2 and 4 key words, in pieces, for a sequence longer than the writer's buffer,
 * for no unitig at all, and the choice of the L line for a self link and a hairpin link.  Writes hand.unitigs, hand.unitigs.fa,
 * hand.unitigs.gfa and hand.summary into the directory given, for the example that the test works by hand.
 *   cc -std=gnu11 -fsanitize=address,undefined -o unitig_host_check tools/unitig_host_check.c soapdenovo-trans_amd/csrc/host/unitigsplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/unitigsplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "unitig_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define LINK(from, to, o, o2, b, link) {from, to, (o) | (o2) << 1 | (b) << 2 | (link) << 8, 0}

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
	if (argc != 2) { fprintf(stderr, "usage: unitig_host_check <directory>\n"); return 2; }
	char path[4096], line[SDT_UNITIG_SUMMARY_MAX], text[8192];
	FILE *f;
	/* the example by hand, K = 3: a fork ACG -> CGA.. / CGT; unitig 1 ACG (one node), 2 CGAT (two nodes, large counts), 3 CGT (one
	 * node, with a hairpin link), 4 a cycle TTC TCT CTT (its closing link), 5 GGG, isolated.  The files are written in two pieces,
	 * as the tool does */
	const uint64_t keys[10] = {0x07, 0x07, 0x1C, 0x32, 0x1E, 0x1E, 0x29, 0x1A, 0x3F, 0x3F};
	const sdt_unitig rec[5] = {{9, 1, 9, 9, 0 | 0 << 4 | 2 << 8}, {7000000000ULL, 2, 3000000000u, 4000000000u, 0 | 1 << 4 | 0 << 8}, {5, 1, 5, 5, 0 | 1 << 4 | 1 << 8},
	                           {12, 3, 3, 5, 1 | 1 << 4 | 1 << 8}, {2, 1, 2, 2, 0}};
	const uint8_t bases[] = {0, 1, 3, 1, 3, 0, 2, 1, 3, 2, 2, 2, 1, 2, 2, 3, 3, 3};
	const uint64_t offs[4] = {0, 3, 7, 10}, offs2[3] = {0, 5, 8};
	const sdt_unitig_link links[] = {LINK(0, 1, 0, 0, 0, 6), LINK(0, 2, 0, 0, 2, 3), LINK(1, 0, 1, 1, 2, 6), LINK(2, 2, 0, 1, 0, 63), LINK(2, 0, 1, 1, 2, 3),
	                                 LINK(3, 3, 0, 0, 2, 4), LINK(3, 3, 1, 1, 3, 4)};
	const uint64_t info[8] = {8, 8, 5, 1, 8, 18, 3, 0};
	uint32_t nodes[5];
	sdt_unitig_tally t = {0, 0, 0, 0, nodes};
	snprintf(path, sizeof path, "%s/hand.unitigs", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_unitig_list_write(f, keys, rec, 0, 3, 1, 3, &t) == 0 && sdt_unitig_list_write(f, keys + 6, rec + 3, 3, 2, 1, 3, &t) == 0 &&
	      fclose(f) == 0);
	CHECK(t.circular == 1 && t.isolated == 1 && t.dead_ends == 2 && nodes[1] == 2 && nodes[3] == 3);
	snprintf(path, sizeof path, "%s/hand.unitigs.fa", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_unitig_fasta_write(f, rec, bases, offs, 0, 3) == 0 && sdt_unitig_fasta_write(f, rec + 3, bases + 10, offs2, 3, 2) == 0 &&
	      fclose(f) == 0);
	snprintf(path, sizeof path, "%s/hand.unitigs.gfa", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_unitig_gfa_header(f) == 0 && sdt_unitig_gfa_segments(f, rec, bases, offs, 0, 3) == 0 &&
	      sdt_unitig_gfa_segments(f, rec + 3, bases + 10, offs2, 3, 2) == 0 && sdt_unitig_gfa_links(f, links, 4, 3, &t) == 0 &&
	      sdt_unitig_gfa_links(f, links + 4, 3, 3, &t) == 0 && fclose(f) == 0);
	/* the L-line choice: a link and its mirror give one line; the hairpin link (3, +) -> (3, -) is its own mirror; of the closing link
	 * of the cycle the (+, +) record is written, its mirror (-, -) is not */
	CHECK(t.links == 4);
	CHECK(sdt_unitig_link_written(links + 0) && !sdt_unitig_link_written(links + 2) && sdt_unitig_link_written(links + 3) && !sdt_unitig_link_written(links + 4) && sdt_unitig_link_written(links + 5) &&
	      !sdt_unitig_link_written(links + 6));
	const sdt_unitig_link other_hairpin = LINK(7, 7, 1, 0, 1, 2);
	CHECK(sdt_unitig_link_written(&other_hairpin));
	sdt_unitig_summary(line, info, &t, 3);
	CHECK(!strcmp(line, "unitigs: live 8 unitigs 5 circular 1 isolated 1 dead_ends 2 links 4 bases 18 longest 3 n50 4\n"));
	snprintf(path, sizeof path, "%s/hand.summary", argv[1]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);

	/* keys of two and four words: most significant word first; K = 33: the first letter is the low pair of word 0 */
	const uint64_t k2[4] = {0, 1, 1, 0};
	const sdt_unitig r2[1] = {{7, 2, 3, 4, 0 | 2 << 4 | 3 << 8}};
	sdt_unitig_tally t2 = {0, 0, 0, 0, NULL};
	CHECK((f = tmpfile()) && sdt_unitig_list_write(f, k2, r2, 41, 1, 2, 33, &t2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "42 AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC CAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA 2 34 7 350 3 4 2 3 0\n") && t2.dead_ends == 0 && t2.isolated == 0);
	uint64_t k4[8] = {0, 0, 0, 2, 0, 0, 0, 1};
	k4[4] = 3ULL << 60;                                      /* K = 127: the first letter is bits 61..60 of word 0 */
	CHECK((f = tmpfile()) && sdt_unitig_list_write(f, k4, r2, 0, 1, 4, 127, &t2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(text[2 + 126] == 'T' && text[2 + 127] == ' ' && text[2 + 128] == 'G' && strstr(text, " 2 128 7 350 3 4 2 3 0\n"));
	const uint64_t i2[8] = {2, 2, 1, 0, 2, 128, 2, 0};
	sdt_unitig_summary(line, i2, &t2, 127);                  /* (no room for the node counts: no n50) */
	CHECK(strstr(line, " longest 2 n50 0\n"));

	/* a sequence longer than the writer's buffer, every letter kept, in both files */
	enum { LONG = 10000 };
	uint8_t *lb = (uint8_t *)malloc(LONG);
	CHECK(lb != NULL);
	for (int i = 0; i < LONG; i++) lb[i] = (uint8_t)(i % 3);
	const uint64_t lo[2] = {0, LONG};
	const sdt_unitig lr[1] = {{LONG - 2, LONG - 2, 1, 1, 0}};
	char *big = (char *)malloc(2 * LONG + 512);
	CHECK(big && (f = tmpfile()) && sdt_unitig_fasta_write(f, lr, lb, lo, 0, 1) == 0 && sdt_unitig_gfa_segments(f, lr, lb, lo, 0, 1) == 0 &&
	      slurp(f, big, 2 * LONG + 512) == 0 && fclose(f) == 0);
	const char *seq = strchr(big, '\n');
	CHECK(seq && !strncmp(seq + 1, "ACTACTACT", 9) && seq[1 + LONG] == '\n' && seq[LONG] == "ACT"[(LONG - 1) % 3]);
	const char *seg = seq + 2 + LONG;
	CHECK(!strncmp(seg, "S\t1\tACTACT", 10) && !strncmp(seg + 4 + LONG, "\tLN:i:10000\tKC:i:9998\n", 22) && seg[4 + LONG + 22] == 0);
	free(lb); free(big);

	/* no unitig at all */
	const uint64_t i0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	sdt_unitig_tally t0 = {0, 0, 0, 0, NULL};
	CHECK((f = tmpfile()) && sdt_unitig_list_write(f, NULL, NULL, 0, 0, 1, 3, &t0) == 0 && sdt_unitig_fasta_write(f, NULL, NULL, offs, 0, 0) == 0 &&
	      sdt_unitig_gfa_segments(f, NULL, NULL, offs, 0, 0) == 0 && sdt_unitig_gfa_links(f, NULL, 0, 3, &t0) == 0 && slurp(f, text, sizeof text) == 0 &&
	      fclose(f) == 0 && text[0] == 0);
	sdt_unitig_summary(line, i0, &t0, 3);
	CHECK(!strcmp(line, "unitigs: live 0 unitigs 0 circular 0 isolated 0 dead_ends 0 links 0 bases 0 longest 0 n50 0\n"));
	printf("unitig_host_check: ok\n");
	return 0;
}
