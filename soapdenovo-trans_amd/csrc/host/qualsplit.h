/* qualsplit.h -- the host side of `sdt-kmers qtrim` that needs no device: what a read's record line looks like, whether a record can
 * be that of a read of a given length under given parameters, which line of the verdict dropped a read, and the histogram of the kept
 * lengths with its summary line.  Where a read goes is trimsplit.h's sdt_trim_route.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/quality_host_check.c links it on its own. */
#ifndef SDT_QUALSPLIT_H
#define SDT_QUALSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* "span low ee_ppm start len verdict\n"; returns the end of what it wrote (at most SDT_QUAL_LINE_MAX bytes) */
enum { SDT_QUAL_LINE_MAX = 6 * 11 };
char *sdt_put_qual_line(char *p, const sdt_read_quality *r);

/* the first line of the verdict (include/sdt_gpu.h) that drops a segment with these measures, recomputed from the record */
enum { SDT_QUAL_KEPT = 0, SDT_QUAL_SHORT = 1, SDT_QUAL_LOW = 2, SDT_QUAL_ERRORS = 3 };
int sdt_qual_drop_cause(const sdt_read_quality *r, const sdt_quality_params *p);

/* 1 iff r can be the record of a read of read_len bases under p: verdict 0, 2 or 3; a segment within the read with no more low bases
 * than bases and 10^6 expected errors per million at most, nothing measured on an empty one; dropped iff a line of the verdict drops
 * it, and then start = len = 0; kept: len = span, the range lies in the read, whole iff it is the read and then start = 0 */
int sdt_qual_record_ok(const sdt_read_quality *r, uint64_t read_len, const sdt_quality_params *p);

/* the kept reads by length, and the reads counted */
typedef struct {
	uint64_t *by_len, cap;                          /* by_len[0, cap) */
	uint64_t reads, whole, clipped, dropped;        /* reads noted; by verdict */
	uint64_t n_short, n_low, n_errors;              /* the dropped reads by the line that dropped them */
	uint64_t bases_in, bases_out;
} sdt_len_hist;
/* one read: 0, -2 (nothing noted) when sdt_qual_record_ok fails, -1 (nothing noted) when memory runs out */
int sdt_len_hist_note(sdt_len_hist *h, const sdt_read_quality *r, uint64_t read_len, const sdt_quality_params *p);
/* "len reads" per kept length that occurs, ascending, then
 * "# reads R whole W clipped C dropped D short S low V errors X bases_in I bases_out O"; 0, or -1 when a write failed */
int sdt_len_hist_write(FILE *f, const sdt_len_hist *h);
void sdt_len_hist_free(sdt_len_hist *h);

#endif
