/* trimsplit.c -- see trimsplit.h */
#include "trimsplit.h"

int sdt_trim_route(const sdt_pair_ranges *pr, size_t *cursor, const sdt_read_trim *trim, uint64_t nrec, uint64_t ord)
{
	if (ord >= nrec || trim[ord].len == 0) return SDT_TRIM_TO_NONE;
	if (!sdt_pair_ranges_holds(pr, ord, cursor)) return SDT_TRIM_TO_SINGLE;
	const uint64_t first = pr->v[2 * *cursor];
	const uint64_t mate = first + ((ord - first) ^ 1u);
	return mate < nrec && trim[mate].len != 0 ? SDT_TRIM_TO_PAIRS : SDT_TRIM_TO_SINGLE;
}

static char *put_field(char *p, uint32_t v, char sep)
{
	char t[10];
	int n = 0;
	do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (n) *p++ = t[--n];
	*p++ = sep;
	return p;
}

char *sdt_put_trim_line(char *p, const sdt_read_trim *t)
{
	p = put_field(p, t->kmers, ' ');
	p = put_field(p, t->weak, ' ');
	p = put_field(p, t->median, ' ');
	p = put_field(p, t->start, ' ');
	p = put_field(p, t->len, ' ');
	return put_field(p, t->verdict, '\n');
}
