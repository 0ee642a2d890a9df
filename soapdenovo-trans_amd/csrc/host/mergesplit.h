/* mergesplit.h -- the host side of `sdt-kmers merge` that needs no device: what a read's record line looks like, whether a record can
 * be that of a read with a given overlap record, and the statistics of the pairs with the summary line.  Where a read of a pair that
 * did not merge goes is trimsplit.h's sdt_trim_route; the histogram of the inserts is overlapsplit.h's.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/merge_host_check.c links it on its own. */
#ifndef SDT_MERGESPLIT_H
#define SDT_MERGESPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* "merged mismatches from_b start len verdict\n"; returns the end of what it wrote (at most SDT_MERGE_LINE_MAX bytes) */
enum { SDT_MERGE_LINE_MAX = 6 * 11 };
char *sdt_put_merge_line(char *p, const sdt_read_merge *r);

/* 1 iff r can be the merge record of a read of read_len bases whose overlap record is ov, under the rule of include/sdt_gpu.h: merged:
 * the overlap's insert, at least 1; no more mismatch columns than the read has bases or the fragment has positions, no more of them
 * decided for mate 2 than there are; start = len = 0 and verdict SDT_MERGE_MERGED.  Not merged: the first three fields 0 and start,
 * len and verdict those of ov */
int sdt_merge_record_ok(const sdt_read_merge *r, const sdt_read_overlap *ov, uint64_t read_len);

/* the pairs counted */
typedef struct {
	uint64_t pairs, overlapping, merged;    /* pairs noted; those with an overlap; those merged */
	uint64_t columns, from_b;               /* mismatch columns of the merged pairs; those decided for mate 2 */
	uint64_t merged_bases;                  /* bases of the merged reads */
} sdt_merge_stats;
/* one pair: the merge records and the overlap records of its mates.  0; -2 (nothing noted): the records are not those of one pair (the
 * mates disagree in merged, mismatches or from_b, or only one of them is merged) */
int sdt_merge_stats_note(sdt_merge_stats *s, const sdt_read_merge *a, const sdt_read_merge *b, const sdt_read_overlap *oa, const sdt_read_overlap *ob);
/* "merge: reads R pairs P overlapping V merged M mismatch columns C bases in I bases out O" (no newline) into buf[n]; bases_out: the
 * bases of the reads that did not merge as they are written; the merged bases are added here.  Returns snprintf's count */
int sdt_merge_summary(char *buf, size_t n, const sdt_merge_stats *s, uint64_t reads, uint64_t bases_in, uint64_t bases_out);

#endif
