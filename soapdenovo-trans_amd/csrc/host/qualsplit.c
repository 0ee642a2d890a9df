/* qualsplit.c -- see qualsplit.h */
#include <stdlib.h>
#include <string.h>
#include "qualsplit.h"
#include "putdec.h"

char *sdt_put_qual_line(char *p, const sdt_read_quality *r)
{
	p = sdt_put_dec(p, r->span, ' ');
	p = sdt_put_dec(p, r->low, ' ');
	p = sdt_put_dec(p, r->ee_ppm, ' ');
	p = sdt_put_dec(p, r->start, ' ');
	p = sdt_put_dec(p, r->len, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

int sdt_qual_drop_cause(const sdt_read_quality *r, const sdt_quality_params *p)
{
	if (r->span < (p->min_len > 1 ? p->min_len : 1u)) return SDT_QUAL_SHORT;
	if (100 * (uint64_t)r->low > (uint64_t)p->max_low_pct * r->span) return SDT_QUAL_LOW;
	if (p->max_ee_ppm != 0 && r->ee_ppm > p->max_ee_ppm) return SDT_QUAL_ERRORS;
	return SDT_QUAL_KEPT;
}

int sdt_qual_record_ok(const sdt_read_quality *r, uint64_t read_len, const sdt_quality_params *p)
{
	if (r->verdict != 0 && r->verdict != 2 && r->verdict != 3) return 0;
	if (r->span > read_len || r->low > r->span || r->ee_ppm > 1000000u) return 0;
	if (r->span == 0 && r->ee_ppm != 0) return 0;
	const int dropped = sdt_qual_drop_cause(r, p) != SDT_QUAL_KEPT;
	if (dropped != (r->verdict == 3)) return 0;
	if (dropped) return r->start == 0 && r->len == 0;
	if (r->len != r->span || (uint64_t)r->start + r->len > read_len) return 0;
	if (r->verdict == 0) return r->start == 0 && r->len == read_len;
	return r->len != read_len;
}

int sdt_len_hist_note(sdt_len_hist *h, const sdt_read_quality *r, uint64_t read_len, const sdt_quality_params *p)
{
	if (!sdt_qual_record_ok(r, read_len, p)) return -2;
	if (r->len && r->len >= h->cap) {
		uint64_t ncap = h->cap ? h->cap : 256;
		while (ncap <= r->len) ncap *= 2;
		uint64_t *nb = (uint64_t *)realloc(h->by_len, ncap * sizeof(uint64_t));
		if (!nb) return -1;
		memset(nb + h->cap, 0, (ncap - h->cap) * sizeof(uint64_t));
		h->by_len = nb;
		h->cap = ncap;
	}
	if (r->len) h->by_len[r->len]++;
	h->reads++;
	h->whole += r->verdict == 0;
	h->clipped += r->verdict == 2;
	h->dropped += r->verdict == 3;
	const int why = r->verdict == 3 ? sdt_qual_drop_cause(r, p) : SDT_QUAL_KEPT;
	h->n_short += why == SDT_QUAL_SHORT;
	h->n_low += why == SDT_QUAL_LOW;
	h->n_errors += why == SDT_QUAL_ERRORS;
	h->bases_in += read_len;
	h->bases_out += r->len;
	return 0;
}

int sdt_len_hist_write(FILE *f, const sdt_len_hist *h)
{
	for (uint64_t n = 1; n < h->cap; n++)
		if (h->by_len[n] && fprintf(f, "%llu %llu\n", (unsigned long long)n, (unsigned long long)h->by_len[n]) < 0) return -1;
	return fprintf(f, "# reads %llu whole %llu clipped %llu dropped %llu short %llu low %llu errors %llu bases_in %llu bases_out %llu\n",
	               (unsigned long long)h->reads, (unsigned long long)h->whole, (unsigned long long)h->clipped, (unsigned long long)h->dropped,
	               (unsigned long long)h->n_short, (unsigned long long)h->n_low, (unsigned long long)h->n_errors, (unsigned long long)h->bases_in,
	               (unsigned long long)h->bases_out) < 0 ? -1 : 0;
}

void sdt_len_hist_free(sdt_len_hist *h)
{
	free(h->by_len);
	memset(h, 0, sizeof *h);
}
