/* screensplit.c -- see screensplit.h */
#include <stdlib.h>
#include <string.h>
#include "screensplit.h"
#include "putdec.h"

static int grow(void **p, uint64_t *cap, uint64_t need, size_t elem)
{
	if (need <= *cap) return 0;
	uint64_t c = *cap ? *cap : 64;
	while (c < need) c *= 2;
	void *q = realloc(*p, (size_t)c * elem);
	if (!q) return -1;
	*p = q;
	*cap = c;
	return 0;
}

/* the open segment [from, s->ncodes) of reference ref, which starts at letter `at` of its record, becomes a sequence, unless it is empty */
static int close_segment(sdt_ref_set *s, uint64_t from, uint32_t ref, uint64_t at)
{
	if (from == s->ncodes) return 0;
	uint64_t cap = s->seqs_cap;
	/* offsets holds one more than ref_of_seq: both grow to the same capacity + 1 */
	if (s->nseqs + 1 > s->seqs_cap) {
		uint64_t ocap = s->seqs_cap ? s->seqs_cap + 1 : 0, scap = s->seqs_cap;
		if (grow((void **)&s->ref_of_seq, &cap, s->nseqs + 1, sizeof(uint32_t)) != 0) return -1;
		if (grow((void **)&s->seg_start, &scap, cap, sizeof(uint64_t)) != 0) return -1;
		if (grow((void **)&s->offsets, &ocap, cap + 1, sizeof(uint64_t)) != 0) return -1;
		s->seqs_cap = cap;
	}
	s->offsets[s->nseqs] = from;
	s->offsets[s->nseqs + 1] = s->ncodes;
	s->seg_start[s->nseqs] = at;
	s->ref_of_seq[s->nseqs++] = ref;
	return 0;
}

int sdt_refs_parse(sdt_ref_set *s, const char *label, const char *text, size_t n, char *err, size_t errcap)
{
	unsigned long long line = 1, header_line = 0;
	int in_record = 0, seen = 0;                             /* a header was read; its record has a sequence character */
	uint64_t from = s->ncodes, letters = 0, from_at = 0;     /* letters of the record so far; the open segment starts at from_at */
	size_t i = 0;
	while (i < n) {
		if (text[i] == '>') {
			if (in_record && !seen) { snprintf(err, errcap, "%s line %llu: the record has no sequence", label, header_line); return -1; }
			if (in_record && close_segment(s, from, s->n_refs - 1, from_at) != 0) goto nomem;
			size_t e = i + 1, b = i + 1;
			while (e < n && text[e] != '\n') e++;
			size_t ne = b;
			while (ne < e && text[ne] != ' ' && text[ne] != '\t' && text[ne] != '\r') ne++;
			uint64_t cap = s->refs_cap, cap2 = s->refs_cap;
			if (grow((void **)&s->names, &cap, (uint64_t)s->n_refs + 1, sizeof(char *)) != 0) goto nomem;
			if (grow((void **)&s->bases, &cap2, (uint64_t)s->n_refs + 1, sizeof(uint64_t)) != 0) goto nomem;
			s->refs_cap = (uint32_t)(cap < cap2 ? cap : cap2);
			char *name = (char *)malloc(ne - b + 1);
			if (!name) goto nomem;
			memcpy(name, text + b, ne - b);
			name[ne - b] = 0;
			s->names[s->n_refs] = name;
			s->bases[s->n_refs++] = 0;
			in_record = 1;
			seen = 0;
			header_line = line;
			from = s->ncodes;
			letters = from_at = 0;
			i = e;                                               /* (at the newline, or at the end) */
			continue;
		}
		const char ch = text[i++];
		if (ch == '\n') { line++; continue; }
		if (ch == ' ' || ch == '\t' || ch == '\r') continue;
		if (!in_record) { snprintf(err, errcap, "%s line %llu: bases before the first header", label, line); return -1; }
		seen = 1;
		int code;
		switch (ch) {
		case 'A': case 'a': code = 0; break;
		case 'C': case 'c': code = 1; break;
		case 'T': case 't': code = 2; break;
		case 'G': case 'g': code = 3; break;
		default: code = -1; break;
		}
		letters++;
		if (code < 0) {                                          /* any other letter cuts the reference */
			if (close_segment(s, from, s->n_refs - 1, from_at) != 0) goto nomem;
			from = s->ncodes;
			from_at = letters;
			continue;
		}
		if (grow((void **)&s->codes, &s->codes_cap, s->ncodes + 1, 1) != 0) goto nomem;
		s->codes[s->ncodes++] = (uint8_t)code;
		s->bases[s->n_refs - 1]++;
	}
	if (in_record && !seen) { snprintf(err, errcap, "%s line %llu: the record has no sequence", label, header_line); return -1; }
	if (in_record && close_segment(s, from, s->n_refs - 1, from_at) != 0) goto nomem;
	return 0;
nomem:
	snprintf(err, errcap, "%s: out of memory", label);
	return -1;
}

int sdt_refs_load(sdt_ref_set *s, const char *path, char *err, size_t errcap)
{
	FILE *f = fopen(path, "rb");
	if (!f) { snprintf(err, errcap, "cannot read %s", path); return -1; }
	char *text = NULL;
	uint64_t n = 0, cap = 0;
	for (;;) {
		if (grow((void **)&text, &cap, n + 65536, 1) != 0) { fclose(f); free(text); snprintf(err, errcap, "%s: out of memory", path); return -1; }
		const size_t got = fread(text + n, 1, 65536, f);
		n += got;
		if (got < 65536) break;
	}
	const int bad = ferror(f);
	fclose(f);
	if (bad) { free(text); snprintf(err, errcap, "cannot read %s", path); return -1; }
	const int rc = sdt_refs_parse(s, path, text, (size_t)n, err, errcap);
	free(text);
	return rc;
}

int sdt_refs_pack(sdt_ref_set *s)
{
	if (!s->offsets) {
		s->offsets = (uint64_t *)calloc(1, sizeof(uint64_t));
		if (!s->offsets) return -1;
	}
	free(s->words);
	s->nwords = (s->ncodes + 15) / 16 + 4;
	s->words = (uint32_t *)calloc((size_t)s->nwords, sizeof(uint32_t));
	if (!s->words) return -1;
	for (uint64_t i = 0; i < s->ncodes; i++)
		s->words[i >> 4] |= (uint32_t)s->codes[i] << (30 - 2 * (i & 15));
	return 0;
}

void sdt_refs_free(sdt_ref_set *s)
{
	for (uint32_t i = 0; i < s->n_refs; i++) free(s->names[i]);
	free(s->names); free(s->bases); free(s->codes); free(s->offsets); free(s->ref_of_seq); free(s->words); free(s->seg_start);
	memset(s, 0, sizeof *s);
}

char *sdt_put_screen_line(char *p, const sdt_read_screen *r)
{
	p = sdt_put_dec(p, r->kmers, ' ');
	p = sdt_put_dec(p, r->hits, ' ');
	p = sdt_put_dec(p, r->ref == SDT_SCREEN_NO_REF ? 0u : r->ref + 1, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

int sdt_screen_matched(const sdt_read_screen *r, const sdt_screen_params *prm)
{
	return r->hits >= (prm->min_hits > 1 ? prm->min_hits : 1u) && 100 * (uint64_t)r->hits >= (uint64_t)prm->min_hit_pct * r->kmers;
}

int sdt_screen_record_ok(const sdt_read_screen *r, uint64_t read_len, uint32_t k, uint32_t n_refs)
{
	const uint64_t kmers = read_len >= k ? read_len - k + 1 : 0;
	if (r->kmers != kmers || r->hits > r->kmers || r->start != 0) return 0;
	if (r->hits ? r->ref >= n_refs : r->ref != SDT_SCREEN_NO_REF) return 0;
	if (r->verdict == 0) return r->len == read_len;
	return r->verdict == 1 && r->len == 0;
}

int sdt_screen_stats_init(sdt_screen_stats *st, uint32_t n_refs)
{
	memset(st, 0, sizeof *st);
	st->reads = (uint64_t *)calloc(n_refs ? n_refs : 1, sizeof(uint64_t));
	st->hits = (uint64_t *)calloc(n_refs ? n_refs : 1, sizeof(uint64_t));
	if (!st->reads || !st->hits) { sdt_screen_stats_free(st); return -1; }
	st->n_refs = n_refs;
	return 0;
}

int sdt_screen_stats_note(sdt_screen_stats *st, const sdt_read_screen *r, uint64_t read_len, uint32_t k, const sdt_screen_params *prm)
{
	if (!sdt_screen_record_ok(r, read_len, k, st->n_refs)) return -2;
	if (r->hits) {
		st->reads[r->ref]++;
		st->hits[r->ref] += r->hits;
	}
	st->total++;
	st->matched += sdt_screen_matched(r, prm) != 0;
	if (r->verdict == 0) st->kept++; else st->dropped++;
	return 0;
}

int sdt_screen_stats_write(FILE *f, const sdt_screen_stats *st, const sdt_ref_set *refs)
{
	for (uint32_t i = 0; i < st->n_refs; i++)
		if (fprintf(f, "%u %s %llu %llu %llu\n", i + 1, refs->names[i], (unsigned long long)refs->bases[i], (unsigned long long)st->reads[i],
		            (unsigned long long)st->hits[i]) < 0) return -1;
	return fprintf(f, "# reads %llu matched %llu kept %llu dropped %llu\n", (unsigned long long)st->total, (unsigned long long)st->matched,
	               (unsigned long long)st->kept, (unsigned long long)st->dropped) < 0 ? -1 : 0;
}

void sdt_screen_stats_free(sdt_screen_stats *st)
{
	free(st->reads); free(st->hits);
	memset(st, 0, sizeof *st);
}
