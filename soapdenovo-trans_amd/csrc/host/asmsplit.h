/* asmsplit.h -- the host side of `sdt-kmers evaluate` that needs no device: the support records of the segments of an assembly
 * (screensplit.h: every letter outside ACGT cuts a contig into segments) folded into one record per contig, in the contig's own
 * coordinates; the lines of prefix.asmSupport and prefix.asmSpectrum; the node counts and the summary line.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/asm_host_check.c links it on its own. */
#ifndef SDT_ASMSPLIT_H
#define SDT_ASMSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "screensplit.h"

/* One contig: the fields of sdt_seq_support over all its segments, in 64 bits.  sum, kmers, found, solid and gaps add up; longest_gap
 * is the maximum over the segments, the first among equals, and longest_at the first base of that gap's first k-mer counted from the
 * contig's first letter (0-based, the cut letters counted): seg_start + the segment's longest_at.  Without a gap longest_gap is 0 and
 * longest_at = kmers, as in a record.  bases: the letters ACGT of the contig. */
typedef struct { uint64_t sum, bases, kmers, found, solid, gaps, longest_gap, longest_at; } sdt_asm_contig;

/* seg[refs->nseqs] -> out[refs->n_refs]; a contig without a segment is all 0 */
void sdt_asm_fold(const sdt_ref_set *refs, const sdt_seq_support *seg, sdt_asm_contig *out);

/* "index name bases kmers found solid sum gaps longest_gap longest_at" per contig, index 1-based; 0, or -1 when a write failed */
int sdt_asm_support_write(FILE *f, const sdt_ref_set *refs, const sdt_asm_contig *ctg);
/* "row c0 c1 c2 c3 c4 c5 c6 c7" for every row of the matrix (rows x SDT_ASM_CN_COLS) with a non-zero entry; 0, or -1 */
int sdt_asm_spectrum_write(FILE *f, const uint64_t *matrix, uint32_t rows);

/* from the matrix: the nodes of the table, those counted min_count times or more, and those of them that the assembly holds (copy
 * number 1 or more).  rows must exceed min_count, so that the last row, which takes every larger count, lies at or above it:
 * 0, or -1 when it does not (nothing written) */
typedef struct { uint64_t nodes, solid_nodes, covered; } sdt_asm_nodes;
int sdt_asm_nodes_of(const uint64_t *matrix, uint32_t rows, uint32_t min_count, sdt_asm_nodes *out);

/* "evaluate: sequences S kmers N found F solid V nodes D solid_nodes E covered C completeness_x100 P qv_x100 Q\n" into line.
 * totals: sequences, k-mers, found, solid (sdt_gpu_asm_spectrum).  P = floor(10000 C / E), "-" when E = 0.
 * Q = round(100 * -10 log10(1 - (V / N)^(1 / K))): the consensus quality if every k-mer without support holds one wrong base
 * (Merqury's rule); "inf" when V = N, "-" when N = 0. */
enum { SDT_ASM_SUMMARY_MAX = 400 };
void sdt_asm_summary(char line[SDT_ASM_SUMMARY_MAX], const uint64_t totals[4], const sdt_asm_nodes *nodes, int K);

#endif
