/* overlapsplit.c -- see overlapsplit.h */
#include <stdlib.h>
#include <string.h>
#include "overlapsplit.h"
#include "putdec.h"

char *sdt_put_overlap_line(char *p, const sdt_read_overlap *r)
{
	p = sdt_put_dec(p, r->overlap, ' ');
	p = sdt_put_dec(p, r->mismatches, ' ');
	p = sdt_put_dec(p, r->insert, ' ');
	p = sdt_put_dec(p, r->start, ' ');
	p = sdt_put_dec(p, r->len, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

int sdt_overlap_record_ok(const sdt_read_overlap *r, uint64_t read_len)
{
	if (r->verdict != 0 && r->verdict != 2 && r->verdict != 3) return 0;
	if (r->start != 0 || r->mismatches > r->overlap) return 0;
	if ((r->insert == 0) != (r->overlap == 0)) return 0;
	const uint64_t kept = r->insert && r->insert < read_len ? r->insert : read_len;
	if (r->verdict == 3) return r->len == 0;
	if (r->len != kept || kept == 0) return 0;
	return (r->verdict == 0) == (kept == read_len);
}

int sdt_insert_hist_note(sdt_insert_hist *h, const sdt_read_overlap *a, const sdt_read_overlap *b, uint64_t len_a, uint64_t len_b)
{
	if (!sdt_overlap_record_ok(a, len_a) || !sdt_overlap_record_ok(b, len_b)) return -2;
	if (a->overlap != b->overlap || a->mismatches != b->mismatches || a->insert != b->insert) return -2;
	if (a->insert) {
		if (h->n == h->cap) {
			const size_t cap = h->cap ? 2 * h->cap : 1024;
			uint32_t *v = (uint32_t *)realloc(h->v, cap * sizeof(uint32_t));
			if (!v) return -1;
			h->v = v;
			h->cap = cap;
		}
		h->v[h->n++] = a->insert;
		h->clipped += a->insert < len_a || a->insert < len_b;
	}
	h->pairs++;
	return 0;
}

static int by_value(const void *x, const void *y)
{
	const uint32_t a = *(const uint32_t *)x, b = *(const uint32_t *)y;
	return a < b ? -1 : a > b;
}

uint32_t sdt_insert_hist_median(sdt_insert_hist *h)
{
	if (!h->n) return 0;
	qsort(h->v, h->n, sizeof(uint32_t), by_value);
	return h->v[(h->n - 1) / 2];
}

int sdt_insert_hist_write(FILE *f, sdt_insert_hist *h)
{
	const uint32_t median = sdt_insert_hist_median(h);
	for (size_t i = 0; i < h->n;) {
		size_t j = i;
		while (j < h->n && h->v[j] == h->v[i]) j++;
		if (fprintf(f, "%u %zu\n", h->v[i], j - i) < 0) return -1;
		i = j;
	}
	return fprintf(f, "# pairs %llu overlapping %zu clipped %llu median %u\n", (unsigned long long)h->pairs, h->n, (unsigned long long)h->clipped, median) < 0 ? -1 : 0;
}

void sdt_insert_hist_free(sdt_insert_hist *h)
{
	free(h->v);
	memset(h, 0, sizeof *h);
}
