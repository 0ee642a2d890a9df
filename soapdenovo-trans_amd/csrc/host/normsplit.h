/* normsplit.h -- the host side of `sdt-kmers normalize` that needs no device: which ordinals of the read stream hold interleaved
 * pairs (from the batches the stream callback sees), and where a kept read goes and what its record looks like.  Plain C, no GPU
 * library: tools/select_host_check.c links it on its own. */
#ifndef SDT_NORMSPLIT_H
#define SDT_NORMSPLIT_H
#include <stdint.h>
#include <stddef.h>

/* v[2i], v[2i + 1] = [first, end) of ordinals that hold interleaved pairs: ascending, disjoint, of even length, neighbours merged --
 * the form sdt_gpu_select_kept_reads takes */
typedef struct {
	uint64_t *v;
	size_t n, cap;
} sdt_pair_ranges;

/* one batch of the stream: nreads reads with the ordinals ord_base + i * ord_stride.  Batches with ord_stride != 2 hold single reads
 * and change nothing.  parity is the batch's stream_parity (seqio.h): 0 = the read-1 file of a pair of files, whose reads take the
 * first ordinal of every pair, 1 = the read-2 file, so the range starts one ordinal before ord_base -- also where the read-1 file had
 * no read at all.  Returns 0, or -1 when memory runs out. */
int sdt_pair_ranges_note(sdt_pair_ranges *pr, uint64_t ord_base, uint64_t ord_stride, int parity, uint64_t nreads);
void sdt_pair_ranges_free(sdt_pair_ranges *pr);
/* 1 iff ordinal ord lies in a pair range.  *cursor (0 at first) walks the ranges: ord must not descend between calls. */
int sdt_pair_ranges_holds(const sdt_pair_ranges *pr, uint64_t ord, size_t *cursor);

/* ">ordinal + 1\n" and the len bases from base `start` of a 2-bit stream as letters on one line; returns the end of what it wrote
 * (at most len + 23 bytes) */
char *sdt_put_fasta_record(char *p, uint64_t ord, const uint32_t *words, uint64_t start, uint64_t len);
/* the sequence line alone: len bases from `start` of words and a newline (len + 1 bytes) */
char *sdt_put_fasta_bases(char *p, const uint32_t *words, uint64_t start, uint64_t len);

#endif
