/* trimsplit.c -- see trimsplit.h */
#include "trimsplit.h"
#include "putdec.h"

int sdt_trim_route(const sdt_pair_ranges *pr, size_t *cursor, sdt_alive_fn alive, const void *recs, uint64_t nrec, uint64_t ord)
{
	if (ord >= nrec || !alive(recs, ord)) return SDT_TRIM_TO_NONE;
	if (!sdt_pair_ranges_holds(pr, ord, cursor)) return SDT_TRIM_TO_SINGLE;
	const uint64_t first = pr->v[2 * *cursor];
	const uint64_t mate = first + ((ord - first) ^ 1u);
	return mate < nrec && alive(recs, mate) ? SDT_TRIM_TO_PAIRS : SDT_TRIM_TO_SINGLE;
}

char *sdt_put_trim_line(char *p, const sdt_read_trim *t)
{
	p = sdt_put_dec(p, t->kmers, ' ');
	p = sdt_put_dec(p, t->weak, ' ');
	p = sdt_put_dec(p, t->median, ' ');
	p = sdt_put_dec(p, t->start, ' ');
	p = sdt_put_dec(p, t->len, ' ');
	return sdt_put_dec(p, t->verdict, '\n');
}
