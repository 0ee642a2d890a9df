/* bubblesplit.c -- see bubblesplit.h */
#include <stdlib.h>
#include <string.h>
#include "bubblesplit.h"
#include "putdec.h"

static const char letters[4] = {'A', 'C', 'T', 'G'};
enum { MAX_K = 127 };                                                        /* four key words */

/* the K letters of a key of nw words, most significant word first */
static char *put_kmer(char *p, const uint64_t *key, int nw, int K)
{
	for (int j = 0; j < K; j++) {
		const int bit = 2 * (K - 1 - j);                                        /* of the whole key; word nw - 1 holds the lowest 64 */
		*p++ = letters[(key[nw - 1 - (bit >> 6)] >> (bit & 63)) & 3u];
	}
	return p;
}

int sdt_bubble_list_write(FILE *f, const uint64_t *keys, const sdt_bubble *rec, uint64_t first, uint64_t n, int nw, int K, uint64_t kinds[3])
{
	char line[21 + 2 * (MAX_K + 1) + 4 + 4 * 11 + 2 * 21 + 2 * 3 + 2];
	for (uint64_t i = 0; i < n; i++) {
		const sdt_bubble *r = rec + i;
		const int kind = sdt_bubble_kind(r, K);
		char *p = sdt_put_dec(line, first + i + 1, ' ');
		p = put_kmer(p, keys + i * 2 * (uint64_t)nw, nw, K);
		*p++ = ' ';
		p = put_kmer(p, keys + (i * 2 + 1) * (uint64_t)nw, nw, K);
		*p++ = ' ';
		*p++ = letters[r->info & 3u];
		*p++ = ' ';
		*p++ = letters[r->info >> 2 & 3u];
		*p++ = ' ';
		p = sdt_put_dec(p, r->len_a, ' ');
		p = sdt_put_dec(p, r->len_b, ' ');
		p = sdt_put_dec(p, r->min_a, ' ');
		p = sdt_put_dec(p, r->min_b, ' ');
		p = sdt_put_dec(p, r->sum_a, ' ');
		p = sdt_put_dec(p, r->sum_b, ' ');
		p = sdt_put_dec(p, r->info >> 8 & 63u, ' ');
		p = sdt_put_dec(p, r->info >> 16 & 63u, ' ');
		p = sdt_put_dec(p, (uint64_t)kind, '\n');
		kinds[kind]++;
		if (fwrite(line, 1, (size_t)(p - line), f) != (size_t)(p - line)) return -1;
	}
	return 0;
}

int sdt_bubble_fasta_write(FILE *f, const uint64_t *keys, const sdt_bubble *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n,
                           int nw, int K)
{
	char head[1 + 21 + 2 + 5 + 11 + 5 + 11 + 5 + 21], kmer[MAX_K + 1], chunk[4096];
	for (uint64_t j = 0; j < 2 * n; j++) {
		const sdt_bubble *r = rec + (j >> 1);
		const int b = (int)(j & 1);
		char *p = head;
		*p++ = '>';
		p = sdt_put_dec(p, first + (j >> 1) + 1, '_');
		*p++ = b ? 'b' : 'a';
		memcpy(p, " len=", 5);
		p = sdt_put_dec(p + 5, b ? r->len_b : r->len_a, ' ');
		memcpy(p, "min=", 4);
		p = sdt_put_dec(p + 4, b ? r->min_b : r->min_a, ' ');
		memcpy(p, "sum=", 4);
		p = sdt_put_dec(p + 4, b ? r->sum_b : r->sum_a, '\n');
		if (fwrite(head, 1, (size_t)(p - head), f) != (size_t)(p - head)) return -1;
		put_kmer(kmer, keys + (j >> 1) * 2 * (uint64_t)nw, nw, K);
		if (fwrite(kmer, 1, (size_t)K, f) != (size_t)K) return -1;
		for (uint64_t at = offsets[j]; at < offsets[j + 1];) {
			size_t k = 0;
			for (; k < sizeof chunk && at < offsets[j + 1]; k++, at++) chunk[k] = letters[bases[at] & 3u];
			if (fwrite(chunk, 1, k, f) != k) return -1;
		}
		if (fputc('\n', f) == EOF) return -1;
	}
	return 0;
}

void sdt_bubble_summary(char line[SDT_BUBBLE_SUMMARY_MAX], const uint64_t info[8], const uint64_t kinds[3])
{
	snprintf(line, SDT_BUBBLE_SUMMARY_MAX, "bubbles: live %llu forks %llu branches %llu reached %llu bubbles %llu kind0 %llu kind1 %llu kind2 %llu longest %llu\n",
	         (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)info[4],
	         (unsigned long long)kinds[0], (unsigned long long)kinds[1], (unsigned long long)kinds[2], (unsigned long long)info[6]);
}
