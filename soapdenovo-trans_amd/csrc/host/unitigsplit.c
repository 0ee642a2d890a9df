/* unitigsplit.c -- see unitigsplit.h */
#include <stdlib.h>
#include <string.h>
#include "unitigsplit.h"
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

static char *put_text(char *p, const char *text)
{
	const size_t n = strlen(text);
	memcpy(p, text, n);
	return p + n;
}

static int put_line(FILE *f, const char *line, const char *end) { return fwrite(line, 1, (size_t)(end - line), f) == (size_t)(end - line) ? 0 : -1; }

/* bases[from .. to) in letters, a buffer at a time */
static int put_bases(FILE *f, const uint8_t *bases, uint64_t from, uint64_t to)
{
	char chunk[4096];
	for (uint64_t at = from; at < to;) {
		size_t k = 0;
		for (; k < sizeof chunk && at < to; k++, at++) chunk[k] = letters[bases[at] & 3u];
		if (fwrite(chunk, 1, k, f) != k) return -1;
	}
	return 0;
}

int sdt_unitig_list_write(FILE *f, const uint64_t *keys, const sdt_unitig *rec, uint64_t first, uint64_t n, int nw, int K, sdt_unitig_tally *t)
{
	char line[21 + 2 * (MAX_K + 1) + 2 * 11 + 3 * 21 + 2 * 11 + 3 * 2 + 2];
	for (uint64_t i = 0; i < n; i++) {
		const sdt_unitig *r = rec + i;
		const uint32_t in = r->info >> 4 & 15u, out = r->info >> 8 & 15u, circular = r->info & 1u;
		char *p = sdt_put_dec(line, first + i + 1, ' ');
		p = put_kmer(p, keys + i * 2 * (uint64_t)nw, nw, K);
		*p++ = ' ';
		p = put_kmer(p, keys + (i * 2 + 1) * (uint64_t)nw, nw, K);
		*p++ = ' ';
		p = sdt_put_dec(p, r->nodes, ' ');
		p = sdt_put_dec(p, (uint64_t)r->nodes + (uint64_t)(K - 1), ' ');
		p = sdt_put_dec(p, r->sum, ' ');
		p = sdt_put_dec(p, (uint64_t)((unsigned __int128)r->sum * 100u / r->nodes), ' ');
		p = sdt_put_dec(p, r->min, ' ');
		p = sdt_put_dec(p, r->max, ' ');
		p = sdt_put_dec(p, in, ' ');
		p = sdt_put_dec(p, out, ' ');
		p = sdt_put_dec(p, circular, '\n');
		t->circular += circular;
		t->isolated += in == 0 && out == 0;
		t->dead_ends += (in == 0) != (out == 0);
		if (t->nodes) t->nodes[first + i] = r->nodes;
		if (put_line(f, line, p) != 0) return -1;
	}
	return 0;
}

int sdt_unitig_fasta_write(FILE *f, const sdt_unitig *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n)
{
	char head[1 + 21 + 7 + 11 + 5 + 21 + 5 + 11 + 5 + 11 + 10 + 2 + 2];
	for (uint64_t i = 0; i < n; i++) {
		const sdt_unitig *r = rec + i;
		char *p = head;
		*p++ = '>';
		p = sdt_put_dec(p, first + i + 1, ' ');
		p = sdt_put_dec(put_text(p, "nodes="), r->nodes, ' ');
		p = sdt_put_dec(put_text(p, "sum="), r->sum, ' ');
		p = sdt_put_dec(put_text(p, "min="), r->min, ' ');
		p = sdt_put_dec(put_text(p, "max="), r->max, ' ');
		p = sdt_put_dec(put_text(p, "circular="), r->info & 1u, '\n');
		if (put_line(f, head, p) != 0 || put_bases(f, bases, offsets[i], offsets[i + 1]) != 0 || fputc('\n', f) == EOF) return -1;
	}
	return 0;
}

int sdt_unitig_gfa_header(FILE *f) { return fputs("H\tVN:Z:1.0\n", f) == EOF ? -1 : 0; }

int sdt_unitig_gfa_segments(FILE *f, const sdt_unitig *rec, const uint8_t *bases, const uint64_t *offsets, uint64_t first, uint64_t n)
{
	char text[8 + 21 + 8 + 21 + 2];
	for (uint64_t i = 0; i < n; i++) {
		char *p = text;
		*p++ = 'S';
		*p++ = '\t';
		p = sdt_put_dec(p, first + i + 1, '\t');
		if (put_line(f, text, p) != 0 || put_bases(f, bases, offsets[i], offsets[i + 1]) != 0) return -1;
		p = sdt_put_dec(put_text(text, "\tLN:i:"), offsets[i + 1] - offsets[i], '\t');
		p = sdt_put_dec(put_text(p, "KC:i:"), rec[i].sum, '\n');
		if (put_line(f, text, p) != 0) return -1;
	}
	return 0;
}

int sdt_unitig_gfa_links(FILE *f, const sdt_unitig_link *links, uint64_t n_links, int K, sdt_unitig_tally *t)
{
	char line[2 + 2 * (11 + 2) + 11 + 2 + 5 + 3 + 2];
	for (uint64_t j = 0; j < n_links; j++) {
		const sdt_unitig_link *l = links + j;
		if (!sdt_unitig_link_written(l)) continue;
		char *p = line;
		*p++ = 'L';
		*p++ = '\t';
		p = sdt_put_dec(p, (uint64_t)l->from + 1, '\t');
		*p++ = l->info & 1u ? '-' : '+';
		*p++ = '\t';
		p = sdt_put_dec(p, (uint64_t)l->to + 1, '\t');
		*p++ = l->info >> 1 & 1u ? '-' : '+';
		*p++ = '\t';
		p = sdt_put_dec(p, (uint64_t)(K - 1), 'M');
		p = sdt_put_dec(put_text(p, "\tlc:i:"), l->info >> 8 & 63u, '\n');
		t->links++;
		if (put_line(f, line, p) != 0) return -1;
	}
	return 0;
}

static int by_nodes_descending(const void *a, const void *b)
{
	const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
	return x < y ? 1 : x > y ? -1 : 0;
}

void sdt_unitig_summary(char line[SDT_UNITIG_SUMMARY_MAX], const uint64_t info[8], sdt_unitig_tally *t, int K)
{
	uint64_t n50 = 0, acc = 0;
	if (t->nodes && info[2]) {
		qsort(t->nodes, (size_t)info[2], sizeof *t->nodes, by_nodes_descending);
		for (uint64_t i = 0; i < info[2]; i++) {
			acc += (uint64_t)t->nodes[i] + (uint64_t)(K - 1);
			if (acc >= info[5] - acc) { n50 = (uint64_t)t->nodes[i] + (uint64_t)(K - 1); break; }
		}
	}
	snprintf(line, SDT_UNITIG_SUMMARY_MAX, "unitigs: live %llu unitigs %llu circular %llu isolated %llu dead_ends %llu links %llu bases %llu longest %llu n50 %llu\n",
	         (unsigned long long)info[0], (unsigned long long)info[2], (unsigned long long)t->circular, (unsigned long long)t->isolated,
	         (unsigned long long)t->dead_ends, (unsigned long long)t->links, (unsigned long long)info[5], (unsigned long long)info[6], (unsigned long long)n50);
}
