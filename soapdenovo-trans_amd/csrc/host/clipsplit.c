/* clipsplit.c -- see clipsplit.h */
#include <stdlib.h>
#include <string.h>
#include "clipsplit.h"
#include "putdec.h"

/* one finished record behind the others; 0, or -1: out of memory */
static int append(sdt_adapter_list *l, const uint8_t *codes, uint32_t m, const char *name, size_t name_len, int end)
{
	if (l->n == l->cap) {
		const size_t cap = l->cap ? 2 * l->cap : 8;
		uint64_t *o = (uint64_t *)realloc(l->offsets, (cap + 1) * sizeof *o);
		if (o) l->offsets = o;
		uint8_t *e = (uint8_t *)realloc(l->ends, cap);
		if (e) l->ends = e;
		char **nm = (char **)realloc(l->names, cap * sizeof *nm);
		if (nm) l->names = nm;
		if (!o || !e || !nm) return -1;
		if (!l->cap) l->offsets[0] = 0;
		l->cap = cap;
	}
	const uint64_t at = l->offsets[l->n], need = ((at + m + 15) >> 4) + 1;
	if (need > l->wcap) {
		const size_t wcap = need > 2 * l->wcap ? need : 2 * l->wcap;
		uint32_t *w = (uint32_t *)realloc(l->words, wcap * sizeof *w);
		if (!w) return -1;
		memset(w + l->wcap, 0, (wcap - l->wcap) * sizeof *w);
		l->words = w;
		l->wcap = wcap;
	}
	char *copy = (char *)malloc(name_len + 1);
	if (!copy) return -1;
	memcpy(copy, name, name_len);
	copy[name_len] = 0;
	for (uint32_t k = 0; k < m; k++)
		l->words[(at + k) >> 4] |= (uint32_t)codes[k] << (30 - 2 * ((at + k) & 15));
	l->names[l->n] = copy;
	l->ends[l->n] = (uint8_t)end;
	l->offsets[++l->n] = at + m;
	return 0;
}

/* back to n0 adapters: the names go, the words behind the last base are zero again */
static void roll_back(sdt_adapter_list *l, uint32_t n0)
{
	while (l->n > n0) free(l->names[--l->n]);
	if (!l->words) return;
	const uint64_t at = l->n ? l->offsets[l->n] : 0;
	const size_t w = (size_t)(at >> 4);
	if (at & 15) l->words[w] &= ~(0xFFFFFFFFu >> (2 * (at & 15)));
	const size_t from = (at & 15) ? w + 1 : w;
	if (from < l->wcap) memset(l->words + from, 0, (l->wcap - from) * sizeof *l->words);
}

/* the open record (name != NULL) is complete: checked and appended */
static int close_record(sdt_adapter_list *l, const uint8_t *codes, uint32_t m, const char *name, size_t name_len, int end, const char *label,
                        unsigned long long header_line, char *err, size_t errlen)
{
	if (!name) return 0;
	if (m == 0) { snprintf(err, errlen, "%s line %llu: the record has no bases", label, header_line); return -1; }
	if (l->n >= SDT_CLIP_MAX_ADAPTERS) { snprintf(err, errlen, "%s line %llu: more than %d adapters", label, header_line, SDT_CLIP_MAX_ADAPTERS); return -1; }
	if (append(l, codes, m, name, name_len, end) != 0) { snprintf(err, errlen, "%s: out of memory", label); return -1; }
	return 0;
}

int sdt_adapters_parse(sdt_adapter_list *l, const char *text, size_t len, const char *label, int end, char *err, size_t errlen)
{
	const uint32_t n0 = l->n;
	uint8_t codes[SDT_CLIP_MAX_ADAPTER_LEN];
	uint32_t m = 0;
	const char *name = NULL;
	size_t name_len = 0;
	unsigned long long lineno = 0, header_line = 0;
	int bad = 0;
	for (size_t at = 0; at < len && !bad;) {
		size_t eol = at;
		while (eol < len && text[eol] != '\n') eol++;
		lineno++;
		size_t a = at, b = eol;
		while (b > a && (text[b - 1] == '\r' || text[b - 1] == ' ' || text[b - 1] == '\t')) b--;
		while (a < b && (text[a] == ' ' || text[a] == '\t')) a++;
		at = eol + 1;
		if (a < b && text[a] == '>') {
			bad = close_record(l, codes, m, name, name_len, end, label, header_line, err, errlen) != 0;
			name = text + a + 1;
			name_len = 0;
			while (name + name_len < text + b && name[name_len] != ' ' && name[name_len] != '\t') name_len++;
			header_line = lineno;
			m = 0;
			continue;
		}
		for (size_t i = a; i < b && !bad; i++) {
			const char c = text[i];
			bad = 1;
			if (!name) snprintf(err, errlen, "%s line %llu: bases before the first '>' line", label, lineno);
			else if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'a' && c != 'c' && c != 'g' && c != 't')
				snprintf(err, errlen, "%s line %llu: '%c' is not one of ACGT", label, lineno, c);
			else if (m == SDT_CLIP_MAX_ADAPTER_LEN)
				snprintf(err, errlen, "%s line %llu: the record has more than %d bases", label, lineno, SDT_CLIP_MAX_ADAPTER_LEN);
			else {
				codes[m++] = (uint8_t)((c & 6) >> 1);           /* seqio.c: A0 C1 T2 G3, either case */
				bad = 0;
			}
		}
	}
	if (!bad) bad = close_record(l, codes, m, name, name_len, end, label, header_line, err, errlen) != 0;
	if (bad) { roll_back(l, n0); return -1; }
	return 0;
}

int sdt_adapters_load(sdt_adapter_list *l, const char *path, int end, char *err, size_t errlen)
{
	FILE *f = fopen(path, "rb");
	if (!f) { snprintf(err, errlen, "%s: cannot open", path); return -1; }
	char *text = NULL;
	size_t len = 0, cap = 0;
	for (;;) {
		if (len == cap) {
			cap = cap ? 2 * cap : 4096;
			char *t = (char *)realloc(text, cap);
			if (!t) { free(text); fclose(f); snprintf(err, errlen, "%s: out of memory", path); return -1; }
			text = t;
		}
		const size_t got = fread(text + len, 1, cap - len, f);
		if (!got) break;
		len += got;
	}
	const int failed = ferror(f);
	fclose(f);
	if (failed) { free(text); snprintf(err, errlen, "%s: read error", path); return -1; }
	const int rc = sdt_adapters_parse(l, text, len, path, end, err, errlen);
	free(text);
	return rc;
}

void sdt_adapters_free(sdt_adapter_list *l)
{
	roll_back(l, 0);
	free(l->words); free(l->offsets); free(l->ends); free(l->names);
	memset(l, 0, sizeof *l);
}

sdt_adapter_set sdt_adapters_set(const sdt_adapter_list *l)
{
	const sdt_adapter_set s = {l->words, l->offsets, l->ends, l->n, 0};
	return s;
}

char *sdt_put_clip_line(char *p, const sdt_read_clip *c)
{
	p = sdt_put_dec(p, c->adapters & 0xFFFFu, ' ');
	p = sdt_put_dec(p, c->adapters >> 16, ' ');
	p = sdt_put_dec(p, c->tail3, ' ');
	p = sdt_put_dec(p, c->tail5, ' ');
	p = sdt_put_dec(p, c->start, ' ');
	p = sdt_put_dec(p, c->len, ' ');
	return sdt_put_dec(p, c->verdict, '\n');
}

int sdt_clip_stats_init(sdt_clip_stats *s, uint32_t n_adapters)
{
	memset(s, 0, sizeof *s);
	s->reads = (uint64_t *)calloc(n_adapters ? n_adapters : 1, sizeof *s->reads);
	s->bases = (uint64_t *)calloc(n_adapters ? n_adapters : 1, sizeof *s->bases);
	if (!s->reads || !s->bases) { sdt_clip_stats_free(s); return -1; }
	s->n = n_adapters;
	return 0;
}

int sdt_clip_stats_note(sdt_clip_stats *s, const sdt_read_clip *c, uint64_t read_len)
{
	const uint32_t a3 = c->adapters & 0xFFFFu, a5 = c->adapters >> 16;
	const int live = c->verdict != 3;
	if (a3 > s->n || a5 > s->n || (c->verdict != 0 && c->verdict != 2 && c->verdict != 3)) return -1;
	if ((uint64_t)c->tail3 + c->tail5 > read_len) return -1;
	if (live ? c->len == 0 || c->start < c->tail5 || (uint64_t)c->start + c->len + c->tail3 > read_len : (c->start | c->len) != 0) return -1;
	if (c->verdict == 0 && (c->len != read_len || c->adapters || c->tail3 || c->tail5)) return -1;
	/* what the adapters left is [s0, e0) */
	const uint64_t e0 = live ? (uint64_t)c->start + c->len + c->tail3 : read_len, s0 = live ? c->start - c->tail5 : 0;
	if (a3) { s->reads[a3 - 1]++; s->bases[a3 - 1] += read_len - e0; }
	if (a5) { s->reads[a5 - 1]++; s->bases[a5 - 1] += s0; }
	if (c->tail3) { s->tail_reads[0]++; s->tail_bases[0] += c->tail3; }
	if (c->tail5) { s->tail_reads[1]++; s->tail_bases[1] += c->tail5; }
	if (c->verdict == 0) s->whole++;
	else if (c->verdict == 2) s->clipped++;
	else s->dropped++;
	return 0;
}

int sdt_clip_stats_write(FILE *f, const sdt_clip_stats *s, const sdt_adapter_list *l)
{
	int ok = 1;
	for (uint32_t i = 0; i < s->n; i++)
		ok &= fprintf(f, "%u %s %d %llu %llu\n", i + 1, l->names[i], l->ends[i] ? 5 : 3, (unsigned long long)s->reads[i], (unsigned long long)s->bases[i]) > 0;
	for (int t = 0; t < 2; t++)
		ok &= fprintf(f, "tail%d %llu %llu\n", t ? 5 : 3, (unsigned long long)s->tail_reads[t], (unsigned long long)s->tail_bases[t]) > 0;
	ok &= fprintf(f, "whole %llu\nclipped %llu\ndropped %llu\n", (unsigned long long)s->whole, (unsigned long long)s->clipped,
	              (unsigned long long)s->dropped) > 0;
	return ok ? 0 : -1;
}

void sdt_clip_stats_free(sdt_clip_stats *s)
{
	free(s->reads); free(s->bases);
	memset(s, 0, sizeof *s);
}
