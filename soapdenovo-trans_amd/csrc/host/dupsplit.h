/* dupsplit.h -- the host side of `sdt-kmers dedup` that needs no device: what a read's record line looks like, and the table of
 * duplication levels (how many classes have how many copies) from the records.  Plain C, no GPU library (include/sdt_gpu.h only for
 * the record's type): tools/dedup_host_check.c links it on its own. */
#ifndef SDT_DUPSPLIT_H
#define SDT_DUPSPLIT_H
#include <stdint.h>
#include <stddef.h>
#include "../../../include/sdt_gpu.h"

/* "first copies verdict\n"; returns the end of what it wrote (at most SDT_DUP_LINE_MAX bytes) */
enum { SDT_DUP_LINE_MAX = 21 + 11 + 11 };
char *sdt_put_dup_line(char *p, const sdt_read_dup *d);

/* one level: `classes` classes of `copies` units each, `reads` reads in them (a pair counts two) */
typedef struct { uint32_t copies; uint64_t classes, reads; } sdt_dup_level;
typedef struct { sdt_dup_level *v; size_t n, cap; } sdt_dup_levels;                 /* v[0 .. n) ascending by copies */

/* the record of one read, in any order: it adds to the reads of its level.  leads != 0: it is the first read of the unit that its
 * class keeps -- every class has exactly one such read -- and the class is counted.  Returns 0, or -1 when memory runs out. */
int sdt_dup_levels_note(sdt_dup_levels *lv, const sdt_read_dup *d, int leads);
void sdt_dup_levels_free(sdt_dup_levels *lv);
/* "copies classes reads\n"; returns the end of what it wrote (at most SDT_DUP_LEVEL_LINE_MAX bytes) */
enum { SDT_DUP_LEVEL_LINE_MAX = 11 + 21 + 21 };
char *sdt_put_dup_level_line(char *p, const sdt_dup_level *l);

#endif
