/* unitigsplit.h -- the host side of `sdt-kmers unitigs` that needs no device: the lines of prefix.unitigs, the records of
 * prefix.unitigs.fa, the lines of prefix.unitigs.gfa (GFA 1) and the summary line, as pure functions of the arrays that
 * sdt_gpu_unitigs_fetch, sdt_gpu_unitigs_seqs and sdt_gpu_unitigs_links give.  Ids are 1-based in every text; k-mers and bases are
 * letters (A0 C1 T2 G3).  Plain C, no GPU library (include/sdt_gpu.h only for the records' types): tools/unitig_host_check.c links
 * it on its own. */
#ifndef SDT_UNITIGSPLIT_H
#define SDT_UNITIGSPLIT_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* what the summary line says beyond the info[8] of sdt_gpu_unitigs_begin.  nodes: room for every unitig's node count by 0-based id
 * (the N50 needs them all), or NULL: then n50 is 0 */
typedef struct { uint64_t circular, isolated, dead_ends, links; uint32_t *nodes; } sdt_unitig_tally;

/* n unitigs whose first has the 0-based id `first`: per unitig "id first last nodes bases sum mean_x100 min max in out circular" (keys:
 * 2 nw words per unitig, first word then last, most significant word first; bases = nodes + K - 1; the mean is a floor); the tally
 * grows by them (isolated: in = out = 0; dead_ends: exactly one of them is 0).  0, or -1 when a write failed */
int sdt_unitig_list_write(FILE *f, const uint64_t *keys, const sdt_unitig *rec, uint64_t first, uint64_t n, int nw, int K, sdt_unitig_tally *t);

/* the same n unitigs as FASTA: ">id nodes=N sum=S min=A max=B circular=C" and the sequence on one line (bases / offsets as
 * sdt_gpu_unitigs_seqs gives them for these n).  0, or -1 when a write failed */
int sdt_unitig_fasta_write(FILE *f, const sdt_unitig *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n);

/* GFA 1: the header line; the S lines of n unitigs "S id seq LN:i:bases KC:i:sum"; the L lines of n_links link records "L from +/- to
 * +/- <K-1>M lc:i:link", tab-separated.  A link is written once: the directed record (from, o, to, o') that is <= its mirror
 * (to, not o', from, not o) as a tuple, + before -; t->links grows by the lines written.  0, or -1 when a write failed */
int sdt_unitig_gfa_header(FILE *f);
int sdt_unitig_gfa_segments(FILE *f, const sdt_unitig *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n);
int sdt_unitig_gfa_links(FILE *f, const sdt_unitig_link *links, uint64_t n_links, int K, sdt_unitig_tally *t);

/* 1 when the GFA writes this link record, 0 when it leaves it to its mirror */
static inline int sdt_unitig_link_written(const sdt_unitig_link *l)
{
	const uint32_t o = l->info & 1u, o2 = l->info >> 1 & 1u;
	if (l->from != l->to) return l->from < l->to;
	return o != o2 || o == 0;                                               /* (u, o, u, o') against (u, not o', u, not o) */
}

/* "unitigs: live L unitigs N circular C isolated I dead_ends D links E bases B longest M n50 X\n" from the info[8] of
 * sdt_gpu_unitigs_begin and the tally; n50 is over bases; sorts t->nodes */
enum { SDT_UNITIG_SUMMARY_MAX = 320 };
void sdt_unitig_summary(char line[SDT_UNITIG_SUMMARY_MAX], const uint64_t info[8], sdt_unitig_tally *t, int K);

#endif
