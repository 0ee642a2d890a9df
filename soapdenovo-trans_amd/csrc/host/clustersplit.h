/* clustersplit.h -- the host side of `sdt-kmers cluster` that needs no device: what a read's record line and the tail of its FASTA
 * name look like, the --pick text, the reads and bases of every cluster tallied from the records, the lines of prefix.clusters and
 * the summary line.  Ids are 1-based in every text and 0 means none, as `screen` writes references; the library's are 0-based with
 * SDT_CLUSTER_NONE.  Plain C, no GPU library (include/sdt_gpu.h only for the records' types): tools/cluster_host_check.c links it on
 * its own. */
#ifndef SDT_CLUSTERSPLIT_H
#define SDT_CLUSTERSPLIT_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* the id as the texts print it */
static inline uint64_t sdt_cluster_text_id(uint32_t id) { return id == SDT_CLUSTER_NONE ? 0 : (uint64_t)id + 1; }

/* "kmers live split cluster unit verdict\n"; returns the end of what it wrote (at most SDT_CLUSTER_LINE_MAX bytes) */
enum { SDT_CLUSTER_LINE_MAX = 6 * 11 };
char *sdt_put_cluster_line(char *p, const sdt_read_cluster *r);

/* "cluster=<unit>\n", what follows "><read number> " in the FASTA name of a read; at most SDT_CLUSTER_NAME_MAX bytes */
enum { SDT_CLUSTER_NAME_MAX = 8 + 11 };
char *sdt_put_cluster_name_tail(char *p, const sdt_read_cluster *r);

/* "LO:HI", two ids as the texts print them, 1 <= LO <= HI < 2^32, and nothing else: the library's pick_lo and pick_hi, or -1 */
int sdt_cluster_parse_pick(const char *text, uint32_t pick[2]);

/* is the unit of this record picked (the library's rule for keep[]) */
static inline int sdt_cluster_picked(const sdt_read_cluster *r, const uint32_t pick[2])
{
	return r->unit != SDT_CLUSTER_NONE && pick[0] <= r->unit && r->unit <= pick[1];
}

/* what the records of a stream add up to: per cluster the reads and bases of the units assigned to it, and the reads by verdict */
typedef struct {
	uint64_t *reads, *bases;                /* by cluster id, n_clusters entries each */
	uint64_t n_clusters;
	unsigned long long all, assigned, by_verdict[5];
} sdt_cluster_tally;
int sdt_cluster_tally_init(sdt_cluster_tally *t, uint64_t n_clusters);      /* 0, or -1 when memory runs out */
/* one read of read_len bases; 0, or -1 for an impossible record (a unit or a cluster that does not exist, a verdict above 4) */
int sdt_cluster_tally_note(sdt_cluster_tally *t, const sdt_read_cluster *r, uint64_t read_len);
uint64_t sdt_cluster_tally_largest_reads(const sdt_cluster_tally *t);
void sdt_cluster_tally_free(sdt_cluster_tally *t);

/* prefix.clusters: per cluster in id order "id kmer nodes count_sum reads bases" with the k-mer in letters (keys: nw words per
 * cluster, most significant first; A0 C1 T2 G3), then "# live L link_ends E clusters C largest N unassigned U" from the info[8] of
 * sdt_gpu_cluster_begin and the tally.  0, or -1 when a write failed */
int sdt_cluster_list_write(FILE *f, const uint64_t *keys, const sdt_cluster_comp *comp, int nw, int K, const uint64_t info[8],
                           const sdt_cluster_tally *t);

/* "cluster: reads R assigned A whole W through_mate M unassigned U short S clusters C largest_nodes N largest_reads X\n" */
enum { SDT_CLUSTER_SUMMARY_MAX = 384 };
void sdt_cluster_summary(char line[SDT_CLUSTER_SUMMARY_MAX], const uint64_t info[8], const sdt_cluster_tally *t);

#endif
