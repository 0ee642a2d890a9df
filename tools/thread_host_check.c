/* thread_host_check.c -- the device-free half of `sdt-kmers thread` on its own (tests/test_unitig_thread_host.py builds it with
 * -fsanitize=address,undefined and runs it): the lines of prefix.readPaths and prefix.unitigReads and the summary line
 * (threadsplit.c) from records in a file -- four uint64 (K, unitigs, reads, segments), then the read records, the reads + 1 segment
 * offsets and the segment records as sdt_gpu_unitigs_reads gives them.  Writes check.readPaths, check.unitigReads and check.summary
 * into the directory given; before that a few cases by hand: no read, a read without a segment, the separators, a record whose
 * segments do not add up.
 *   cc -std=gnu11 -fsanitize=address,undefined -o thread_host_check tools/thread_host_check.c soapdenovo-trans_amd/csrc/host/threadsplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/threadsplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "thread_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define SEG(u, o, join, rpos, upos, kmers) {u, (o) | (join) << 1, rpos, upos, kmers, 0}

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
	if (argc != 3) { fprintf(stderr, "usage: thread_host_check <records> <directory>\n"); return 2; }
	char path[4096], line[SDT_THREAD_SUMMARY_MAX], text[4096];
	FILE *f;
	/* by hand: three unitigs; a whole read over a link, a read with a gap and an unlinked step, a read that no unitig holds, a short one */
	const sdt_path_seg s0[2] = {SEG(0, 0, 0, 0, 5, 10), SEG(2, 1, 1, 10, 7, 8)};
	const sdt_path_seg s1[3] = {SEG(1, 1, 0, 3, 9, 4), SEG(1, 0, 0, 30, 0, 2), SEG(0, 0, 2, 32, 1, 1)};
	const sdt_read_path r0 = {18, 18, 2, 0, 0, 2}, r1 = {40, 7, 3, 2, 1, 0}, r2 = {12, 0, 0, 0, SDT_UNITIG_NONE, SDT_UNITIG_NONE},
	                    r3 = {0, 0, 0, 0, SDT_UNITIG_NONE, SDT_UNITIG_NONE}, bad = {18, 17, 2, 0, 0, 2};
	sdt_thread_tally t;
	CHECK(sdt_thread_tally_init(&t, 3) == 0);
	CHECK((f = tmpfile()) && sdt_thread_read_write(f, &r0, s0, &t) == 0 && sdt_thread_read_write(f, &r1, s1, &t) == 0 && sdt_thread_read_write(f, &r2, NULL, &t) == 0 &&
	      sdt_thread_read_write(f, &r3, NULL, &t) == 0);
	CHECK(sdt_thread_read_write(f, &bad, s0, &t) == -2 && t.reads == 4);
	CHECK(slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "18 18 2 0 >1:5+10-<3:7+8\n40 7 3 2 <2:9+4/>2:0+2~>1:1+1\n12 0 0 0 *\n0 0 0 0 *\n"));
	CHECK((f = tmpfile()) && sdt_thread_unitig_reads_write(f, &t) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "1 2 2 11\n2 1 2 6\n3 1 1 8\n"));
	sdt_thread_summary(line, &t);
	CHECK(!strcmp(line, "thread: reads 4 placed 2 whole 1 broken 1 unplaced 1 short 1 segments 5 linked 1 unlinked 1\n"));
	const sdt_path_seg past = SEG(3, 0, 0, 0, 0, 1);
	const sdt_read_path rp = {1, 1, 1, 0, 3, 3};
	CHECK((f = tmpfile()) && sdt_thread_read_write(f, &rp, &past, &t) == -2 && fclose(f) == 0);      /* a unitig that the list does not have */
	sdt_thread_tally_free(&t);
	/* no unitig and no read */
	CHECK(sdt_thread_tally_init(&t, 0) == 0 && (f = tmpfile()) && sdt_thread_unitig_reads_write(f, &t) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0 &&
	      text[0] == 0);
	sdt_thread_summary(line, &t);
	CHECK(!strcmp(line, "thread: reads 0 placed 0 whole 0 broken 0 unplaced 0 short 0 segments 0 linked 0 unlinked 0\n"));
	sdt_thread_tally_free(&t);

	/* the records of the file */
	uint64_t head[4];
	FILE *in = fopen(argv[1], "rb");
	CHECK(in && fread(head, sizeof head[0], 4, in) == 4);
	const uint64_t n_unitigs = head[1], reads = head[2], n_segs = head[3];
	sdt_read_path *rec = (sdt_read_path *)malloc((reads ? reads : 1) * sizeof *rec);
	uint64_t *offs = (uint64_t *)malloc((reads + 1) * sizeof *offs);
	sdt_path_seg *segs = (sdt_path_seg *)malloc((n_segs ? n_segs : 1) * sizeof *segs);
	CHECK(rec && offs && segs && fread(rec, sizeof *rec, reads, in) == reads && fread(offs, sizeof *offs, reads + 1, in) == reads + 1 &&
	      fread(segs, sizeof *segs, n_segs, in) == n_segs && fclose(in) == 0);
	CHECK(offs[0] == 0 && offs[reads] == n_segs && sdt_thread_tally_init(&t, n_unitigs) == 0);
	snprintf(path, sizeof path, "%s/check.readPaths", argv[2]);
	CHECK((f = fopen(path, "w")) != NULL);
	for (uint64_t r = 0; r < reads; r++) {
		CHECK(offs[r + 1] - offs[r] == rec[r].segs);
		CHECK(sdt_thread_read_write(f, rec + r, segs + offs[r], &t) == 0);
	}
	CHECK(fclose(f) == 0);
	snprintf(path, sizeof path, "%s/check.unitigReads", argv[2]);
	CHECK((f = fopen(path, "w")) && sdt_thread_unitig_reads_write(f, &t) == 0 && fclose(f) == 0);
	sdt_thread_summary(line, &t);
	snprintf(path, sizeof path, "%s/check.summary", argv[2]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);
	sdt_thread_tally_free(&t);
	free(rec); free(offs); free(segs);
	printf("thread_host_check: ok\n");
	return 0;
}
