/* overlapsplit.h -- the host side of `sdt-kmers overlap` that needs no device: what a read's record line looks like, whether a record
 * can be that of a read of a given length, and the histogram of the fragment lengths (inserts) of the overlapping pairs with its
 * summary line.  Where a read goes is trimsplit.h's sdt_trim_route.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/overlap_host_check.c links it on its own. */
#ifndef SDT_OVERLAPSPLIT_H
#define SDT_OVERLAPSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* "overlap mismatches insert start len verdict\n"; returns the end of what it wrote (at most SDT_OVERLAP_LINE_MAX bytes) */
enum { SDT_OVERLAP_LINE_MAX = 6 * 11 };
char *sdt_put_overlap_line(char *p, const sdt_read_overlap *r);

/* 1 iff r can be the record of a read of read_len bases under the rule of include/sdt_gpu.h: verdict 0, 2 or 3, start 0, the kept
 * bases min(read_len, insert) (read_len without an overlap) unless dropped, whole iff nothing was cut, no insert without an overlap
 * and no more mismatches than columns */
int sdt_overlap_record_ok(const sdt_read_overlap *r, uint64_t read_len);

/* the inserts of the overlapping pairs, and the pairs counted */
typedef struct {
	uint32_t *v;                /* one insert per overlapping pair, in the order noted; sorted by sdt_insert_hist_write */
	size_t n, cap;
	uint64_t pairs, clipped;    /* pairs noted; overlapping pairs whose insert is shorter than one of the mates: bases were cut */
} sdt_insert_hist;
/* one pair: the records of its mates and their lengths.  0; -1: out of memory; -2 (nothing noted): the records are not those of one
 * pair (sdt_overlap_record_ok fails, or overlap, mismatches and insert differ between the mates) */
int sdt_insert_hist_note(sdt_insert_hist *h, const sdt_read_overlap *a, const sdt_read_overlap *b, uint64_t len_a, uint64_t len_b);
/* the lower median of the inserts noted, 0 if there are none (sorts them) */
uint32_t sdt_insert_hist_median(sdt_insert_hist *h);
/* "insert pairs" per insert that occurs, ascending, then "# pairs P overlapping V clipped C median M"; 0, or -1 when a write failed */
int sdt_insert_hist_write(FILE *f, sdt_insert_hist *h);
void sdt_insert_hist_free(sdt_insert_hist *h);

#endif
