/* cmpsplit.h -- the host side of `sdt-kmers compare` that needs no device: the lines of prefix.cmpMatrix and prefix.cmpKmers, the solid
 * counts taken from the matrix, and the summary line with its four ratios.  All figures are floors of integer arithmetic; none is
 * floating point.  Plain C, no GPU library: tools/cmp_host_check.c links it on its own. */
#ifndef SDT_CMPSPLIT_H
#define SDT_CMPSPLIT_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

/* prefix.cmpMatrix.  The header line names the columns, "a\b 0 1 .. C+" with C = cols - 1: the last column takes every larger count
 * in B.  Then one line per row r, "r m[r][0] .. m[r][cols-1]", the last row written "R+" with R = rows - 1.  0, or -1 when a write
 * failed */
int sdt_cmp_matrix_write(FILE *f, const uint64_t *matrix, uint32_t rows, uint32_t cols);

/* from the matrix: the k-mers counted min_count times or more in A, in B, and in both.  rows and cols must exceed min_count, so that
 * the last row and column, which take every larger count, lie at or above it: 0, or -1 when they do not (nothing written) */
typedef struct { uint64_t solid_a, solid_b, solid_shared; } sdt_cmp_solid;
int sdt_cmp_solid_of(const uint64_t *matrix, uint32_t rows, uint32_t cols, uint32_t min_count, sdt_cmp_solid *out);

/* "compare: nodes_a X nodes_b Y shared S solid_a P solid_b Q solid_shared T jaccard_x10000 J contain_a_x10000 U contain_b_x10000 V
 * braycurtis_x10000 W\n" into line.  totals: the eight of sdt_gpu_compare_tables.  J = floor(10000 S / (X + Y - S)),
 * U = floor(10000 S / X), V = floor(10000 S / Y), W = floor(10000 (sum cA + sum cB - 2 sum min) / (sum cA + sum cB)); a ratio with a
 * zero denominator prints 0 */
enum { SDT_CMP_SUMMARY_MAX = 512 };
void sdt_cmp_summary(char line[SDT_CMP_SUMMARY_MAX], const uint64_t totals[8], const sdt_cmp_solid *solid);

/* "min_a:max_a:min_b:max_b", four whole numbers of 32 bits with min <= max in both pairs, and nothing else: 0, or -1 */
int sdt_cmp_parse_select(const char *text, uint32_t range[4]);

/* prefix.cmpKmers.  n k-mers of K letters in the layout of sdt_gpu_export_nodes (nw words each, most significant first; A0 C1 T2 G3)
 * with their counts: one line "kmer cA cB" each, ascending by key, so the file does not depend on the order the device gave them in.
 * matched > n: a last line "# N matched" with N = matched.  0, or -1 (a write failed, or no memory for the order) */
int sdt_cmp_kmers_write(FILE *f, const uint64_t *keys, const uint32_t *count_a, const uint32_t *count_b, uint64_t n, int nw, int K,
                        uint64_t matched);

#endif
