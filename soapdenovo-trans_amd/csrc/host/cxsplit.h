/* cxsplit.h -- the host side of `sdt-kmers complexity` that needs no device: what a read's record line looks like, whether a record
 * can be that of a read of a given length, and the histogram of the reads' scores with its summary line.  Where a read goes is
 * trimsplit.h's sdt_trim_route.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/complexity_host_check.c links it on its own. */
#ifndef SDT_CXSPLIT_H
#define SDT_CXSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* "windows low score start len verdict\n"; returns the end of what it wrote (at most SDT_CX_LINE_MAX bytes) */
enum { SDT_CX_LINE_MAX = 6 * 11 };
char *sdt_put_cx_line(char *p, const sdt_read_complexity *r);

/* 1 iff r can be the record of a read of read_len bases under the rule of include/sdt_gpu.h: verdict 0, 2 or 3; the windows of a read
 * of that length, no more LOW windows than windows, a score of 100 at most; a dropped read keeps nothing and starts at 0; a kept
 * range lies in the read, is whole iff it is the read, and a read without a LOW window loses no base unless it is dropped */
int sdt_cx_record_ok(const sdt_read_complexity *r, uint64_t read_len);

/* the reads by score (a percentage), and the reads counted */
typedef struct {
	uint64_t by_score[101];
	uint64_t reads, low, dropped, clipped;      /* reads noted; those with a LOW window; by verdict */
} sdt_score_hist;
/* one read: 0, or -2 (nothing noted) when sdt_cx_record_ok fails */
int sdt_score_hist_note(sdt_score_hist *h, const sdt_read_complexity *r, uint64_t read_len);
/* "score reads" per score that occurs, ascending, then "# reads R low V dropped D clipped C"; 0, or -1 when a write failed */
int sdt_score_hist_write(FILE *f, const sdt_score_hist *h);

#endif
