/* bubblesplit.h -- the host side of `sdt-kmers bubbles` that needs no device: the lines of prefix.bubbles, the records of
 * prefix.bubbles.fa and the summary line, as pure functions of the arrays that sdt_gpu_bubbles_fetch and sdt_gpu_bubbles_paths give.
 * Ids are 1-based in every text; k-mers and bases are letters (A0 C1 T2 G3).  Plain C, no GPU library (include/sdt_gpu.h only for
 * the record's type): tools/bubble_host_check.c links it on its own. */
#ifndef SDT_BUBBLESPLIT_H
#define SDT_BUBBLESPLIT_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* 0: len_a == len_b == K (substitution-like); 1: other equal lengths; 2: unequal */
static inline int sdt_bubble_kind(const sdt_bubble *r, int K)
{
	return r->len_a != r->len_b ? 2 : r->len_a == (uint32_t)K ? 0 : 1;
}

/* n bubbles whose first has the 0-based id `first`: per bubble "id source sink base_a base_b len_a len_b min_a min_b sum_a sum_b
 * link_a link_b kind" (keys: 2 nw words per bubble, source then sink, most significant word first); kinds[3] grow by the bubbles of
 * each kind.  0, or -1 when a write failed */
int sdt_bubble_list_write(FILE *f, const uint64_t *keys, const sdt_bubble *rec, uint64_t first, uint64_t n, int nw, int K, uint64_t kinds[3]);

/* the same n bubbles as FASTA, two records each: ">id_a len=L min=M sum=S" and the allele -- the source followed by the branch's
 * bases (bases / offsets as sdt_gpu_bubbles_paths gives them for these n) -- then the same for b.  0, or -1 when a write failed */
int sdt_bubble_fasta_write(FILE *f, const uint64_t *keys, const sdt_bubble *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n,
                           int nw, int K);

/* "bubbles: live L forks F branches B reached R bubbles N kind0 X kind1 Y kind2 Z longest M\n" from the info[8] of sdt_gpu_bubbles_begin */
enum { SDT_BUBBLE_SUMMARY_MAX = 320 };
void sdt_bubble_summary(char line[SDT_BUBBLE_SUMMARY_MAX], const uint64_t info[8], const uint64_t kinds[3]);

#endif
