/* asm_host_check.c -- the device-free half of `sdt-kmers evaluate` on its own (tests/test_asm_support_host.py builds it with
 * -fsanitize=address,undefined and runs it): the segment starts that the FASTA parser of screensplit.c records, the fold of segment
 * records into contigs, the two files and the summary line of asmsplit.c.  Writes hand.asmSupport, hand.asmSpectrum and hand.summary
 * into the directory given, for the example that the test works by hand.
 *   cc -std=gnu11 -fsanitize=address,undefined -o asm_host_check tools/asm_host_check.c soapdenovo-trans_amd/csrc/host/asmsplit.c \
 *      soapdenovo-trans_amd/csrc/host/screensplit.c -lm */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/asmsplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asm_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static int write_all(const char *dir, const char *name, const sdt_ref_set *refs, const sdt_asm_contig *ctg, const uint64_t *matrix, uint32_t rows,
                     const char *summary)
{
	char path[4096];
	FILE *f;
	snprintf(path, sizeof path, "%s/%s.asmSupport", dir, name);
	if (!(f = fopen(path, "w")) || sdt_asm_support_write(f, refs, ctg) != 0 || fclose(f) != 0) return 1;
	snprintf(path, sizeof path, "%s/%s.asmSpectrum", dir, name);
	if (!(f = fopen(path, "w")) || sdt_asm_spectrum_write(f, matrix, rows) != 0 || fclose(f) != 0) return 1;
	snprintf(path, sizeof path, "%s/%s.summary", dir, name);
	if (!(f = fopen(path, "w")) || fputs(summary, f) == EOF || fclose(f) != 0) return 1;
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: asm_host_check <directory>\n"); return 2; }
	char err[512];
	sdt_ref_set refs;
	memset(&refs, 0, sizeof refs);
	/* the example by hand: three contigs in two files, the first cut by NN, the second without a letter ACGT */
	const char *t1 = ">c1 x\nACGTA\nNNtacg\n>c2\nNN\n", *t2 = ">c3\nACGTTCGT\nAAAAA\n";
	CHECK(sdt_refs_parse(&refs, "t1", t1, strlen(t1), err, sizeof err) == 0);
	CHECK(sdt_refs_parse(&refs, "t2", t2, strlen(t2), err, sizeof err) == 0);
	CHECK(sdt_refs_pack(&refs) == 0);
	CHECK(refs.n_refs == 3 && refs.nseqs == 3 && refs.ncodes == 22);
	CHECK(refs.bases[0] == 9 && refs.bases[1] == 0 && refs.bases[2] == 13);
	CHECK(refs.ref_of_seq[0] == 0 && refs.ref_of_seq[1] == 0 && refs.ref_of_seq[2] == 2);
	CHECK(refs.seg_start[0] == 0 && refs.seg_start[1] == 7 && refs.seg_start[2] == 0);
	CHECK(refs.offsets[1] == 5 && refs.offsets[2] == 9 && refs.offsets[3] == 22);
	const sdt_seq_support seg[3] = {{4, 2, 2, 2, 0, 0, 2}, {2, 1, 1, 1, 0, 0, 1}, {8, 10, 4, 4, 2, 4, 1}};
	sdt_asm_contig ctg[3];
	sdt_asm_fold(&refs, seg, ctg);
	CHECK(ctg[0].sum == 6 && ctg[0].kmers == 3 && ctg[0].found == 3 && ctg[0].solid == 3 && ctg[0].gaps == 0 && ctg[0].longest_gap == 0 && ctg[0].longest_at == 3);
	CHECK(ctg[1].kmers == 0 && ctg[1].longest_at == 0 && ctg[1].bases == 0);
	CHECK(ctg[2].gaps == 2 && ctg[2].longest_gap == 4 && ctg[2].longest_at == 1 && ctg[2].bases == 13);
	const uint64_t matrix[3 * SDT_ASM_CN_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 1, 0, 0, 0, 0};
	sdt_asm_nodes nodes;
	CHECK(sdt_asm_nodes_of(matrix, 3, 3, &nodes) == -1 && sdt_asm_nodes_of(matrix, 3, 7, &nodes) == -1);
	CHECK(sdt_asm_nodes_of(matrix, 3, 2, &nodes) == 0 && nodes.nodes == 4 && nodes.solid_nodes == 4 && nodes.covered == 3);
	const uint64_t totals[4] = {3, 13, 7, 7};
	char line[SDT_ASM_SUMMARY_MAX];
	sdt_asm_summary(line, totals, &nodes, 4);
	CHECK(strstr(line, "evaluate: sequences 3 kmers 13 found 7 solid 7 nodes 4 solid_nodes 4 covered 3 completeness_x100 7500 qv_x100 ") == line);
	if (write_all(argv[1], "hand", &refs, ctg, matrix, 3, line) != 0) { fprintf(stderr, "asm_host_check: cannot write into %s\n", argv[1]); return 1; }

	/* a scaffold of three segments: the longest gap is the first among equals over the segments, in the scaffold's coordinates */
	sdt_ref_set sc;
	memset(&sc, 0, sizeof sc);
	const char *t3 = ">s\nACGTACGTAC\nnnnACGTACGTACGT\nNACGTACGTACGTACGT\n>t\nACGT\n";
	CHECK(sdt_refs_parse(&sc, "t3", t3, strlen(t3), err, sizeof err) == 0 && sdt_refs_pack(&sc) == 0);
	CHECK(sc.nseqs == 4 && sc.seg_start[0] == 0 && sc.seg_start[1] == 13 && sc.seg_start[2] == 26 && sc.seg_start[3] == 0);
	const sdt_seq_support s3[4] = {{10, 7, 5, 5, 1, 2, 3}, {20, 8, 6, 5, 2, 3, 1}, {30, 13, 9, 9, 2, 3, 0}, {5, 1, 1, 1, 0, 0, 1}};
	sdt_asm_contig c3[2];
	sdt_asm_fold(&sc, s3, c3);
	CHECK(c3[0].sum == 60 && c3[0].kmers == 28 && c3[0].found == 20 && c3[0].solid == 19 && c3[0].gaps == 5 && c3[0].longest_gap == 3);
	CHECK(c3[0].longest_at == 13 + 1 && c3[0].bases == 38 && c3[1].longest_at == 1 && c3[1].longest_gap == 0);

	/* the summary's special cases */
	const uint64_t none[4] = {0, 0, 0, 0}, all[4] = {2, 50, 50, 50}, some[4] = {1, 1000, 990, 985};
	const sdt_asm_nodes empty = {0, 0, 0}, n2 = {10, 3, 2};
	sdt_asm_summary(line, none, &empty, 31);
	CHECK(strstr(line, "completeness_x100 - qv_x100 -\n"));
	sdt_asm_summary(line, all, &n2, 31);
	CHECK(strstr(line, "solid_nodes 3 covered 2 completeness_x100 6666 qv_x100 inf\n"));
	sdt_asm_summary(line, some, &n2, 31);
	CHECK(strstr(line, "qv_x100 3312\n") || strstr(line, "qv_x100 3311\n") || strstr(line, "qv_x100 3313\n"));
	const uint64_t zero[4] = {1, 10, 0, 0};
	sdt_asm_summary(line, zero, &n2, 31);
	CHECK(strstr(line, "qv_x100 0\n"));
	/* a matrix without a node writes no line */
	char path[4096];
	snprintf(path, sizeof path, "%s/empty.asmSpectrum", argv[1]);
	FILE *f = fopen(path, "w+");
	const uint64_t zeros[2 * SDT_ASM_CN_COLS] = {0};
	CHECK(f && sdt_asm_spectrum_write(f, zeros, 2) == 0 && ftell(f) == 0 && fclose(f) == 0);
	sdt_refs_free(&refs);
	sdt_refs_free(&sc);
	printf("asm_host_check: ok\n");
	return 0;
}
