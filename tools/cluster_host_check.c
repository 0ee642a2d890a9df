/* cluster_host_check.c -- the device-free half of `sdt-kmers cluster` on its own (tests/test_read_cluster_host.py builds it with
 * -fsanitize=address,undefined and runs it): the record line with its 1-based ids, the tail of a FASTA name, the --pick text and the
 * pick rule, the tally of reads and bases per cluster with its refusal of impossible records, the cluster list for 1, 2 and 4 key
 * words, and the summary line (clustersplit.c).  Writes hand.readCluster, hand.clusters and hand.summary into the directory given,
 * for the example that the test works by hand.
 *   cc -std=gnu11 -fsanitize=address,undefined -o cluster_host_check tools/cluster_host_check.c soapdenovo-trans_amd/csrc/host/clustersplit.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../soapdenovo-trans_amd/csrc/host/clustersplit.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "cluster_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)
#define NONE SDT_CLUSTER_NONE

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
	if (argc != 2) { fprintf(stderr, "usage: cluster_host_check <directory>\n"); return 2; }
	char path[4096], line[SDT_CLUSTER_SUMMARY_MAX], text[4096], buf[SDT_CLUSTER_LINE_MAX + 1];
	FILE *f;
	/* the example by hand, K = 3: three clusters AAC (2 nodes), ACG (1 node), TTT (3 nodes); eight reads, the first six in pairs:
	 * a whole pair in cluster 1; mates in clusters 1 and 3; a mate assigned through the other; then a short and an unassigned read */
	const uint64_t keys[3] = {0x01, 0x07, 0x2A};
	const sdt_cluster_comp comp[3] = {{7, 2, 0}, {70000, 1, 0}, {4000000000ULL, 3, 0}};
	const uint64_t info[8] = {6, 8, 3, 3, 2, 4, 0, 0};
	const sdt_read_cluster rec[8] = {{8, 8, 0, 0, 0, 0}, {8, 7, 0, 0, 0, 0}, {8, 8, 0, 0, 0, 1}, {8, 8, 2, 2, 0, 1}, {8, 0, 0, NONE, 1, 2}, {6, 6, 0, 1, 1, 0},
	                                 {0, 0, 0, NONE, NONE, 4}, {9, 0, 0, NONE, NONE, 3}};
	const uint64_t len[8] = {10, 10, 10, 10, 10, 8, 2, 11};
	sdt_cluster_tally t;
	CHECK(sdt_cluster_tally_init(&t, 3) == 0);
	snprintf(path, sizeof path, "%s/hand.readCluster", argv[1]);
	CHECK((f = fopen(path, "w")) != NULL);
	for (int i = 0; i < 8; i++) {
		CHECK(sdt_cluster_tally_note(&t, rec + i, len[i]) == 0);
		char *e = sdt_put_cluster_line(buf, rec + i);
		CHECK(e - buf <= SDT_CLUSTER_LINE_MAX && fwrite(buf, 1, (size_t)(e - buf), f) == (size_t)(e - buf));
	}
	CHECK(fclose(f) == 0);
	CHECK(t.all == 8 && t.assigned == 6 && t.reads[0] == 4 && t.bases[0] == 40 && t.reads[1] == 2 && t.bases[1] == 18 && t.reads[2] == 0);
	CHECK(t.by_verdict[0] == 3 && t.by_verdict[1] == 2 && t.by_verdict[2] == 1 && t.by_verdict[3] == 1 && t.by_verdict[4] == 1);
	CHECK(sdt_cluster_tally_largest_reads(&t) == 4);
	snprintf(path, sizeof path, "%s/hand.clusters", argv[1]);
	CHECK((f = fopen(path, "w")) && sdt_cluster_list_write(f, keys, comp, 1, 3, info, &t) == 0 && fclose(f) == 0);
	sdt_cluster_summary(line, info, &t);
	CHECK(!strcmp(line, "cluster: reads 8 assigned 6 whole 3 through_mate 1 unassigned 1 short 1 clusters 3 largest_nodes 3 largest_reads 4\n"));
	snprintf(path, sizeof path, "%s/hand.summary", argv[1]);
	CHECK((f = fopen(path, "w")) && fputs(line, f) != EOF && fclose(f) == 0);

	/* records that no clustering of three clusters gives: refused, nothing tallied */
	const sdt_read_cluster bad[3] = {{8, 8, 0, 3, 0, 0}, {8, 8, 0, 0, 3, 0}, {8, 8, 0, 0, 0, 5}};
	for (int i = 0; i < 3; i++) CHECK(sdt_cluster_tally_note(&t, bad + i, 10) == -1);
	CHECK(t.all == 8 && t.reads[0] == 4);

	/* the widest record line, and the tail of a name */
	const sdt_read_cluster wide = {4294967295u, 4294967295u, 4294967295u, 4294967294u, 4294967294u, 4};
	char *e = sdt_put_cluster_line(buf, &wide);
	*e = 0;
	CHECK(e - buf == SDT_CLUSTER_LINE_MAX - 9 && !strcmp(buf, "4294967295 4294967295 4294967295 4294967295 4294967295 4\n"));
	e = sdt_put_cluster_name_tail(buf, &wide);
	*e = 0;
	CHECK(e - buf == SDT_CLUSTER_NAME_MAX && !strcmp(buf, "cluster=4294967295\n"));
	e = sdt_put_cluster_name_tail(buf, rec + 7);
	*e = 0;
	CHECK(!strcmp(buf, "cluster=0\n"));

	/* --pick: 1-based in the text, 0-based for the library; NONE is never picked */
	uint32_t pick[2];
	CHECK(sdt_cluster_parse_pick("1:1", pick) == 0 && pick[0] == 0 && pick[1] == 0);
	CHECK(sdt_cluster_parse_pick("2:4294967295", pick) == 0 && pick[0] == 1 && pick[1] == 4294967294u);
	CHECK(!sdt_cluster_picked(rec + 0, pick) && sdt_cluster_picked(rec + 4, pick) && !sdt_cluster_picked(rec + 6, pick));
	const char *refused[] = {"", "1", "1:", ":1", "0:3", "3:2", "1:4294967296", "1:2:3", "-1:2", "1 :2", "1:2 ", "a:b", "1:x"};
	for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) CHECK(sdt_cluster_parse_pick(refused[i], pick) == -1);

	/* keys of two and four words: most significant word first; K = 33: the first letter is the low pair of word 0 */
	sdt_cluster_tally t2;
	CHECK(sdt_cluster_tally_init(&t2, 2) == 0);
	const uint64_t k2[4] = {0, 1, 1, 0};
	const sdt_cluster_comp c2[2] = {{1, 1, 0}, {2, 2, 0}};
	const uint64_t i2[8] = {3, 0, 2, 2, 1, 0, 0, 0};
	CHECK((f = tmpfile()) && sdt_cluster_list_write(f, k2, c2, 2, 33, i2, &t2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "1 AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC 1 1 0 0\n2 CAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA 2 2 0 0\n"
	                    "# live 3 link_ends 0 clusters 2 largest 2 unassigned 0\n"));
	uint64_t k4[8] = {0, 0, 0, 2, 0, 0, 0, 1};
	k4[4] = 3ULL << 60;                                      /* K = 127: the first letter is bits 61..60 of word 0 */
	CHECK((f = tmpfile()) && sdt_cluster_list_write(f, k4, c2, 4, 127, i2, &t2) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(text[2 + 126] == 'T' && text[2 + 127] == ' ' && strstr(text, "\n2 G") != NULL);
	sdt_cluster_tally_free(&t2);

	/* no cluster at all */
	sdt_cluster_tally t0;
	const uint64_t i0[8] = {0};
	CHECK(sdt_cluster_tally_init(&t0, 0) == 0 && sdt_cluster_tally_note(&t0, rec + 6, 2) == 0 && sdt_cluster_tally_note(&t0, rec + 0, 10) == -1);
	CHECK((f = tmpfile()) && sdt_cluster_list_write(f, NULL, NULL, 1, 3, i0, &t0) == 0 && slurp(f, text, sizeof text) == 0 && fclose(f) == 0);
	CHECK(!strcmp(text, "# live 0 link_ends 0 clusters 0 largest 0 unassigned 1\n"));
	sdt_cluster_summary(line, i0, &t0);
	CHECK(!strcmp(line, "cluster: reads 1 assigned 0 whole 0 through_mate 0 unassigned 0 short 1 clusters 0 largest_nodes 0 largest_reads 0\n"));
	sdt_cluster_tally_free(&t0);
	sdt_cluster_tally_free(&t);
	printf("cluster_host_check: ok\n");
	return 0;
}
