/* trimsplit.h -- the host side of `sdt-kmers trim` that needs no device: where a read goes given its own record, its mate's record
 * and the pair ranges (normsplit.h), and what its record line looks like.  Plain C, no GPU library (include/sdt_gpu.h only for the
 * record's type): tools/trim_host_check.c links it on its own. */
#ifndef SDT_TRIMSPLIT_H
#define SDT_TRIMSPLIT_H
#include "normsplit.h"
#include "../../../include/sdt_gpu.h"

enum { SDT_TRIM_TO_NONE = 0, SDT_TRIM_TO_PAIRS = 1, SDT_TRIM_TO_SINGLE = 2 };

/* 1 iff the record of ordinal `ord` keeps something of its read; recs is the caller's, who owns the record type */
typedef int (*sdt_alive_fn)(const void *recs, uint64_t ord);

/* Read `ord` of nrec records by ordinal.  Nothing of it is kept (!alive): SDT_TRIM_TO_NONE.  It lies in a pair range and its mate --
 * the other ordinal of its pair, counted from the range's first -- has a record that is alive: SDT_TRIM_TO_PAIRS, and so says the
 * mate's call, so the two come out next to each other in ordinal order.  Otherwise (a single read, a mate that was dropped, a mate
 * past nrec): SDT_TRIM_TO_SINGLE.  *cursor as for sdt_pair_ranges_holds: ord must not descend between calls. */
int sdt_trim_route(const sdt_pair_ranges *pr, size_t *cursor, sdt_alive_fn alive, const void *recs, uint64_t nrec, uint64_t ord);

/* "kmers weak median start len verdict\n"; returns the end of what it wrote (at most SDT_TRIM_LINE_MAX bytes) */
enum { SDT_TRIM_LINE_MAX = 6 * 11 };
char *sdt_put_trim_line(char *p, const sdt_read_trim *t);

#endif
