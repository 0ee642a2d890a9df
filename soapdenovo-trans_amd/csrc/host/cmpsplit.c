/* cmpsplit.c -- see cmpsplit.h */
#define _GNU_SOURCE
#include <errno.h>
#include <inttypes.h>
#include <stdlib.h>
#include <string.h>
#include "cmpsplit.h"

int sdt_cmp_matrix_write(FILE *f, const uint64_t *matrix, uint32_t rows, uint32_t cols)
{
	if (fputs("a\\b", f) == EOF) return -1;
	for (uint32_t c = 0; c < cols; c++)
		if (fprintf(f, c + 1 == cols ? " %u+" : " %u", c) < 0) return -1;
	if (fputc('\n', f) == EOF) return -1;
	for (uint32_t r = 0; r < rows; r++) {
		if (fprintf(f, r + 1 == rows ? "%u+" : "%u", r) < 0) return -1;
		for (uint32_t c = 0; c < cols; c++)
			if (fprintf(f, " %" PRIu64, matrix[(size_t)r * cols + c]) < 0) return -1;
		if (fputc('\n', f) == EOF) return -1;
	}
	return 0;
}

int sdt_cmp_solid_of(const uint64_t *matrix, uint32_t rows, uint32_t cols, uint32_t min_count, sdt_cmp_solid *out)
{
	if (rows <= min_count || cols <= min_count) return -1;
	memset(out, 0, sizeof *out);
	for (uint32_t r = 0; r < rows; r++)
		for (uint32_t c = 0; c < cols; c++) {
			const uint64_t v = matrix[(size_t)r * cols + c];
			if (r >= min_count) out->solid_a += v;
			if (c >= min_count) out->solid_b += v;
			if (r >= min_count && c >= min_count) out->solid_shared += v;
		}
	return 0;
}

/* floor(10000 num / den), 0 for den = 0 */
static uint64_t x10000(uint64_t num, uint64_t den)
{
	return den ? (uint64_t)(((unsigned __int128)num * 10000u) / den) : 0;
}

void sdt_cmp_summary(char line[SDT_CMP_SUMMARY_MAX], const uint64_t totals[8], const sdt_cmp_solid *solid)
{
	const uint64_t X = totals[0], Y = totals[1], S = totals[2], sum = totals[3] + totals[4];
	snprintf(line, SDT_CMP_SUMMARY_MAX,
	         "compare: nodes_a %" PRIu64 " nodes_b %" PRIu64 " shared %" PRIu64 " solid_a %" PRIu64 " solid_b %" PRIu64 " solid_shared %" PRIu64
	         " jaccard_x10000 %" PRIu64 " contain_a_x10000 %" PRIu64 " contain_b_x10000 %" PRIu64 " braycurtis_x10000 %" PRIu64 "\n",
	         X, Y, S, solid->solid_a, solid->solid_b, solid->solid_shared, x10000(S, X + Y - S), x10000(S, X), x10000(S, Y),
	         x10000(sum - 2 * totals[5], sum));
}

int sdt_cmp_parse_select(const char *text, uint32_t range[4])
{
	const char *p = text;
	for (int i = 0; i < 4; i++) {
		char *end = NULL;
		if (*p < '0' || *p > '9') return -1;
		errno = 0;
		const unsigned long long v = strtoull(p, &end, 10);
		if (errno || v > UINT32_MAX || *end != (i < 3 ? ':' : '\0')) return -1;
		range[i] = (uint32_t)v;
		p = end + 1;
	}
	return range[0] <= range[1] && range[2] <= range[3] ? 0 : -1;
}

typedef struct { const uint64_t *keys; int nw; } key_order;

static int by_key(const void *a, const void *b, void *arg)
{
	const key_order *o = (const key_order *)arg;
	const uint64_t *x = o->keys + *(const uint64_t *)a * (size_t)o->nw, *y = o->keys + *(const uint64_t *)b * (size_t)o->nw;
	for (int w = 0; w < o->nw; w++)
		if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
	return 0;
}

int sdt_cmp_kmers_write(FILE *f, const uint64_t *keys, const uint32_t *count_a, const uint32_t *count_b, uint64_t n, int nw, int K,
                        uint64_t matched)
{
	uint64_t *order = (uint64_t *)malloc((n ? n : 1) * sizeof *order);
	if (!order) return -1;
	for (uint64_t i = 0; i < n; i++) order[i] = i;
	key_order o = {keys, nw};
	qsort_r(order, n, sizeof *order, by_key, &o);
	char text[4 * 64 + 1];
	int rc = 0;
	for (uint64_t i = 0; i < n && rc == 0; i++) {
		const uint64_t *key = keys + order[i] * (size_t)nw;
		for (int j = 0; j < K; j++) {
			const int bit = 2 * (K - 1 - j);                     /* first base in the most significant pair, words most significant first */
			text[j] = "ACTG"[(key[nw - 1 - bit / 64] >> (bit % 64)) & 3u];
		}
		text[K] = 0;
		if (fprintf(f, "%s %u %u\n", text, count_a[order[i]], count_b[order[i]]) < 0) rc = -1;
	}
	if (rc == 0 && matched > n && fprintf(f, "# %" PRIu64 " matched\n", matched) < 0) rc = -1;
	free(order);
	return rc;
}
