/* normsplit.c -- see normsplit.h */
#include <stdlib.h>
#include <string.h>
#include "normsplit.h"
#include "putdec.h"

/* [first, end) into the sorted list; ranges that overlap or touch become one (all of them have even length and the ranges of one
 * pair of files start an even number of ordinals apart, so a merged range pairs the same ordinals) */
static int ranges_add(sdt_pair_ranges *pr, uint64_t first, uint64_t end)
{
	size_t at = pr->n;
	while (at > 0 && pr->v[2 * (at - 1)] > first) at--;                  /* batches come nearly in order: from the back */
	if (at > 0 && pr->v[2 * (at - 1) + 1] >= first) {                    /* runs into its left neighbour */
		at--;
		if (pr->v[2 * at + 1] < end) pr->v[2 * at + 1] = end;
	} else {
		if (pr->n == pr->cap) {
			const size_t cap = pr->cap ? 2 * pr->cap : 16;
			uint64_t *v = (uint64_t *)realloc(pr->v, 2 * cap * sizeof(uint64_t));
			if (!v) return -1;
			pr->v = v;
			pr->cap = cap;
		}
		memmove(pr->v + 2 * (at + 1), pr->v + 2 * at, 2 * (pr->n - at) * sizeof(uint64_t));
		pr->v[2 * at] = first;
		pr->v[2 * at + 1] = end;
		pr->n++;
	}
	size_t last = at;                                                    /* ... and its right neighbours into it */
	while (last + 1 < pr->n && pr->v[2 * (last + 1)] <= pr->v[2 * at + 1]) {
		last++;
		if (pr->v[2 * last + 1] > pr->v[2 * at + 1]) pr->v[2 * at + 1] = pr->v[2 * last + 1];
	}
	if (last > at) {
		memmove(pr->v + 2 * (at + 1), pr->v + 2 * (last + 1), 2 * (pr->n - last - 1) * sizeof(uint64_t));
		pr->n -= last - at;
	}
	return 0;
}

int sdt_pair_ranges_note(sdt_pair_ranges *pr, uint64_t ord_base, uint64_t ord_stride, int parity, uint64_t nreads)
{
	if (nreads == 0 || ord_stride != 2) return 0;
	const uint64_t first = ord_base - (uint64_t)(parity != 0);
	return ranges_add(pr, first, first + 2 * nreads);
}

void sdt_pair_ranges_free(sdt_pair_ranges *pr)
{
	free(pr->v);
	memset(pr, 0, sizeof *pr);
}

int sdt_pair_ranges_holds(const sdt_pair_ranges *pr, uint64_t ord, size_t *cursor)
{
	while (*cursor < pr->n && pr->v[2 * *cursor + 1] <= ord) ++*cursor;
	return *cursor < pr->n && pr->v[2 * *cursor] <= ord;
}

char *sdt_put_fasta_record(char *p, uint64_t ord, const uint32_t *words, uint64_t start, uint64_t len)
{
	*p++ = '>';
	p = sdt_put_dec(p, ord + 1, '\n');
	return sdt_put_fasta_bases(p, words, start, len);
}

char *sdt_put_fasta_bases(char *p, const uint32_t *words, uint64_t start, uint64_t len)
{
	static const char letters[4] = {'A', 'C', 'T', 'G'};
	/* base by base up to a word boundary, then whole words without a branch per base, then the rest.  (The bases are most of what the
	 * read stages' host side does; how fast a loop of one base per round ran depended on where the linker had put it.) */
	uint64_t g = start;
	const uint64_t end = start + len;
	for (; g < end && (g & 15); g++) *p++ = letters[(words[g >> 4] >> (30 - 2 * (int)(g & 15))) & 3u];
	for (; g + 16 <= end; g += 16, p += 16) {
		const uint32_t w = words[g >> 4];
		for (int j = 0; j < 16; j += 4) {
			p[j] = letters[(w >> (30 - 2 * j)) & 3u];
			p[j + 1] = letters[(w >> (28 - 2 * j)) & 3u];
			p[j + 2] = letters[(w >> (26 - 2 * j)) & 3u];
			p[j + 3] = letters[(w >> (24 - 2 * j)) & 3u];
		}
	}
	for (; g < end; g++) *p++ = letters[(words[g >> 4] >> (30 - 2 * (int)(g & 15))) & 3u];
	*p++ = '\n';
	return p;
}
