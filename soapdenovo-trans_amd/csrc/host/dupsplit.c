/* dupsplit.c -- see dupsplit.h */
#include <stdlib.h>
#include <string.h>
#include "dupsplit.h"
#include "putdec.h"

char *sdt_put_dup_line(char *p, const sdt_read_dup *d)
{
	p = sdt_put_dec(p, d->first, ' ');
	p = sdt_put_dec(p, d->copies, ' ');
	return sdt_put_dec(p, d->verdict, '\n');
}

char *sdt_put_dup_level_line(char *p, const sdt_dup_level *l)
{
	p = sdt_put_dec(p, l->copies, ' ');
	p = sdt_put_dec(p, l->classes, ' ');
	return sdt_put_dec(p, l->reads, '\n');
}

int sdt_dup_levels_note(sdt_dup_levels *lv, const sdt_read_dup *d, int leads)
{
	size_t lo = 0, hi = lv->n;                                               /* the first level with copies >= d->copies */
	while (lo < hi) {
		const size_t mid = lo + (hi - lo) / 2;
		if (lv->v[mid].copies < d->copies) lo = mid + 1; else hi = mid;
	}
	if (lo == lv->n || lv->v[lo].copies != d->copies) {
		if (lv->n == lv->cap) {
			const size_t cap = lv->cap ? 2 * lv->cap : 16;
			sdt_dup_level *v = (sdt_dup_level *)realloc(lv->v, cap * sizeof *v);
			if (!v) return -1;
			lv->v = v;
			lv->cap = cap;
		}
		memmove(lv->v + lo + 1, lv->v + lo, (lv->n - lo) * sizeof *lv->v);
		lv->v[lo].copies = d->copies;
		lv->v[lo].classes = lv->v[lo].reads = 0;
		lv->n++;
	}
	lv->v[lo].reads++;
	if (leads) lv->v[lo].classes++;
	return 0;
}

void sdt_dup_levels_free(sdt_dup_levels *lv)
{
	free(lv->v);
	memset(lv, 0, sizeof *lv);
}
