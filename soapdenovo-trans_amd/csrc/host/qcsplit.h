/* qcsplit.h -- the device-free half of `sdt-kmers qc`: the three text files and the summary lines from the reports that
 * sdt_gpu_qc_reads filled, one per class of reads (0 single reads, 1 first mates, 2 second mates).  Integers only.  Plain C, no GPU
 * library: tools/qc_host_check.c links it on its own.
 *
 * A report is the flat array of include/sdt_gpu.h for C cycles, R = C + 1 rows: totals[8], base[R][4], qual[R][94], len[R], gc[101],
 * meanq[94].  A row is written by its number from 0; row C, which holds everything past the C-th cycle, as "C+".
 *   prefix.qcBases    # class row reads A C T G
 *                     per class and row that has a base: reads = A + C + T + G, the reads that reach the row (row C+: the bases in it)
 *   prefix.qcQuals    # class row bases mean_x100 min q10 q25 median q75 q90 max
 *                     per class and row that has a base with a quality: mean_x100 = floor(100 * sum of q / bases); the percentile at
 *                     p is the smallest q whose cumulative count is >= ceil(p * bases / 100).  A class of which no read came with
 *                     qualities (FASTA files) has the one line  # class K: no qualities
 *   prefix.qcReads    # hist class bin reads
 *                     three sparse histograms, the bins that hold a read: len (min(bases, C), bin C as C+), gc (floor of the percentage
 *                     of C and G), meanq (floor of the mean quality; a class without qualities:  # meanq class K: no qualities)
 * and per class one line for stdout:
 *   qc: class K reads R empty E bases B gc G q20 X q30 Y      G, X, Y in hundredths of a percent, floor; X and Y "-" without qualities */
#ifndef SDT_QCSPLIT_H
#define SDT_QCSPLIT_H
#include <stdint.h>
#include <stdio.h>

enum { SDT_QC_CLASSES = 3, SDT_QC_NQ = 94, SDT_QC_NGC = 101, SDT_QC_LINE_MAX = 256 };

typedef struct {
	const uint64_t *report;     /* NULL: no read of the class was seen, nothing is written for it */
	uint64_t with_quals;        /* the reads of the class that came with qualities */
} sdt_qc_class;

/* the words of a report for C cycles: 203 + 99 (C + 1) */
uint64_t sdt_qc_words(uint32_t cycles);
/* the smallest q whose cumulative count is >= ceil(p * n / 100); n = the sum of hist, n >= 1, 0 <= p <= 100 */
uint32_t sdt_qc_percentile(const uint64_t hist[SDT_QC_NQ], uint64_t n, uint32_t p);
/* 0, or -1 when a write failed */
int sdt_qc_bases_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles);
int sdt_qc_quals_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles);
int sdt_qc_reads_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles);
/* the summary line of class k into line[SDT_QC_LINE_MAX], with its newline */
void sdt_qc_summary(char *line, int k, const sdt_qc_class *c, uint32_t cycles);

#endif
