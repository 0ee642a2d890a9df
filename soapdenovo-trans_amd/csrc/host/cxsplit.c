/* cxsplit.c -- see cxsplit.h */
#include "cxsplit.h"
#include "putdec.h"

char *sdt_put_cx_line(char *p, const sdt_read_complexity *r)
{
	p = sdt_put_dec(p, r->windows, ' ');
	p = sdt_put_dec(p, r->low, ' ');
	p = sdt_put_dec(p, r->score, ' ');
	p = sdt_put_dec(p, r->start, ' ');
	p = sdt_put_dec(p, r->len, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

int sdt_cx_record_ok(const sdt_read_complexity *r, uint64_t read_len)
{
	const uint64_t windows = read_len == 0 ? 0 : (read_len <= 64 ? 1 : (read_len + 31) / 32 - 1);
	if (r->verdict != 0 && r->verdict != 2 && r->verdict != 3) return 0;
	if (r->windows != windows || r->low > r->windows || r->score > 100) return 0;
	if (r->verdict == 3) return r->start == 0 && r->len == 0;
	if (r->len == 0 || (uint64_t)r->start + r->len > read_len) return 0;
	if (r->low == 0 && r->len != read_len) return 0;
	return (r->verdict == 0) == (r->len == read_len);
}

int sdt_score_hist_note(sdt_score_hist *h, const sdt_read_complexity *r, uint64_t read_len)
{
	if (!sdt_cx_record_ok(r, read_len)) return -2;
	h->by_score[r->score]++;
	h->reads++;
	h->low += r->low != 0;
	h->dropped += r->verdict == 3;
	h->clipped += r->verdict == 2;
	return 0;
}

int sdt_score_hist_write(FILE *f, const sdt_score_hist *h)
{
	for (unsigned s = 0; s <= 100; s++)
		if (h->by_score[s] && fprintf(f, "%u %llu\n", s, (unsigned long long)h->by_score[s]) < 0) return -1;
	return fprintf(f, "# reads %llu low %llu dropped %llu clipped %llu\n", (unsigned long long)h->reads, (unsigned long long)h->low,
	               (unsigned long long)h->dropped, (unsigned long long)h->clipped) < 0 ? -1 : 0;
}
