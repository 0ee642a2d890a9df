/* supportsplit.h -- the host side of `sdt-kmers support` that needs no device: the lines of prefix.unitigSupport, prefix.linkSupport
 * and prefix.junctions and the summary line, as pure functions of the arrays that the sdt_gpu_unitigs_support_*
 * fetches give.  Ids are 1-based in every text; an oriented unitig is written <id><+|->.  Plain C, no GPU library (include/sdt_gpu.h
 * only for the records' types): tools/support_host_check.c links it on its own. */
#ifndef SDT_SUPPORTSPLIT_H
#define SDT_SUPPORTSPLIT_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* unitigs first .. first + n - 1: "id segments kmers cov_x100", cov_x100 = 100 x kmers / nodes, a floor (the mean number of segments
 * that cover a node of the unitig, in hundredths).  0; -1 when a write failed; -2 for a unitig without a node */
int sdt_support_unitigs_write(FILE *f, const sdt_unitig *rec, const sdt_unitig_support *sup, uint64_t first, uint64_t n);

/* the link records that the GFA writes (unitigsplit.h: sdt_unitig_link_written), in their order: "from o to o' along against" -- along:
 * the reads that traverse the link as written, against: those that traverse its mirror.  0, or -1 when a write failed */
int sdt_support_links_write(FILE *f, const sdt_unitig_link *links, const sdt_link_support *sup, uint64_t n_links);

/* "from via to count" per junction.  0; -1 when a write failed; -2 when via has o = 1 or the list does not ascend by (via, from, to) */
int sdt_support_junctions_write(FILE *f, const sdt_unitig_junction *j, uint64_t n);

/* "support: reads R placed P segments G kmers L traversals T no_record N passages X junctions J dropped Z\n" from the twelve totals and
 * the length of the junction list (the tool adds single reads: the totals over pairs are not written) */
enum { SDT_SUPPORT_SUMMARY_MAX = 320 };
void sdt_support_summary(char line[SDT_SUPPORT_SUMMARY_MAX], const uint64_t totals[12], uint64_t n_junctions);

#endif
