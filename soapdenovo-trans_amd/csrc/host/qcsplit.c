/* qcsplit.c -- see qcsplit.h */
#include <string.h>
#include "qcsplit.h"

typedef struct { const uint64_t *totals, *base, *qual, *len, *gc, *meanq; uint64_t rows; } qc_view;

uint64_t sdt_qc_words(uint32_t cycles) { return 203 + 99 * ((uint64_t)cycles + 1); }

static qc_view view_of(const uint64_t *report, uint32_t cycles)
{
	qc_view v;
	v.rows = (uint64_t)cycles + 1;
	v.totals = report;
	v.base = v.totals + 8;
	v.qual = v.base + 4 * v.rows;
	v.len = v.qual + SDT_QC_NQ * v.rows;
	v.gc = v.len + v.rows;
	v.meanq = v.gc + SDT_QC_NGC;
	return v;
}

uint32_t sdt_qc_percentile(const uint64_t hist[SDT_QC_NQ], uint64_t n, uint32_t p)
{
	/* ceil(p n / 100) without the product: n = 100 a + b */
	const uint64_t a = n / 100, b = n % 100;
	uint64_t need = p * a + (p * b + 99) / 100, cum = 0;
	if (need == 0) need = 1;                                                 /* (p = 0: the smallest q that occurs) */
	for (uint32_t q = 0; q < SDT_QC_NQ; q++) {
		cum += hist[q];
		if (cum >= need) return q;
	}
	return SDT_QC_NQ - 1;
}

/* "12" or "150+" */
static void row_name(char name[16], uint64_t row, uint32_t cycles) { snprintf(name, 16, row == cycles ? "%llu+" : "%llu", (unsigned long long)row); }

int sdt_qc_bases_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles)
{
	if (fprintf(f, "# class row reads A C T G\n") < 0) return -1;
	for (int k = 0; k < SDT_QC_CLASSES; k++) {
		if (!cls[k].report) continue;
		const qc_view v = view_of(cls[k].report, cycles);
		for (uint64_t r = 0; r < v.rows; r++) {
			const uint64_t *b = v.base + 4 * r, n = b[0] + b[1] + b[2] + b[3];
			char name[16];
			if (!n) continue;
			row_name(name, r, cycles);
			if (fprintf(f, "%d %s %llu %llu %llu %llu %llu\n", k, name, (unsigned long long)n, (unsigned long long)b[0], (unsigned long long)b[1],
			            (unsigned long long)b[2], (unsigned long long)b[3]) < 0) return -1;
		}
	}
	return 0;
}

int sdt_qc_quals_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles)
{
	if (fprintf(f, "# class row bases mean_x100 min q10 q25 median q75 q90 max\n") < 0) return -1;
	for (int k = 0; k < SDT_QC_CLASSES; k++) {
		if (!cls[k].report) continue;
		if (!cls[k].with_quals) {
			if (fprintf(f, "# class %d: no qualities\n", k) < 0) return -1;
			continue;
		}
		const qc_view v = view_of(cls[k].report, cycles);
		for (uint64_t r = 0; r < v.rows; r++) {
			const uint64_t *h = v.qual + SDT_QC_NQ * r;
			uint64_t n = 0, sum = 0;
			uint32_t lo = SDT_QC_NQ, hi = 0;
			char name[16];
			for (uint32_t q = 0; q < SDT_QC_NQ; q++) {
				if (!h[q]) continue;
				n += h[q];
				sum += q * h[q];
				if (lo == SDT_QC_NQ) lo = q;
				hi = q;
			}
			if (!n) continue;
			row_name(name, r, cycles);
			if (fprintf(f, "%d %s %llu %llu %u %u %u %u %u %u %u\n", k, name, (unsigned long long)n,
			            (unsigned long long)((unsigned __int128)100 * sum / n), lo, sdt_qc_percentile(h, n, 10), sdt_qc_percentile(h, n, 25),
			            sdt_qc_percentile(h, n, 50), sdt_qc_percentile(h, n, 75), sdt_qc_percentile(h, n, 90), hi) < 0) return -1;
		}
	}
	return 0;
}

static int hist_write(FILE *f, const char *what, int k, const uint64_t *h, uint64_t bins, uint64_t plus)
{
	for (uint64_t i = 0; i < bins; i++)
		if (h[i] && fprintf(f, i == plus ? "%s %d %llu+ %llu\n" : "%s %d %llu %llu\n", what, k, (unsigned long long)i, (unsigned long long)h[i]) < 0) return -1;
	return 0;
}

int sdt_qc_reads_write(FILE *f, const sdt_qc_class cls[SDT_QC_CLASSES], uint32_t cycles)
{
	if (fprintf(f, "# hist class bin reads\n") < 0) return -1;
	for (int pass = 0; pass < 3; pass++)
		for (int k = 0; k < SDT_QC_CLASSES; k++) {
			if (!cls[k].report) continue;
			const qc_view v = view_of(cls[k].report, cycles);
			int rc = 0;
			if (pass == 0) rc = hist_write(f, "len", k, v.len, v.rows, cycles);
			else if (pass == 1) rc = hist_write(f, "gc", k, v.gc, SDT_QC_NGC, UINT64_MAX);
			else if (cls[k].with_quals) rc = hist_write(f, "meanq", k, v.meanq, SDT_QC_NQ, UINT64_MAX);
			else rc = fprintf(f, "# meanq class %d: no qualities\n", k) < 0 ? -1 : 0;
			if (rc != 0) return -1;
		}
	return 0;
}

/* floor(10000 part / whole), the product in 128 bits */
static uint64_t share_x100(uint64_t part, uint64_t whole) { return whole ? (uint64_t)((unsigned __int128)10000 * part / whole) : 0; }

void sdt_qc_summary(char *line, int k, const sdt_qc_class *c, uint32_t cycles)
{
	const qc_view v = view_of(c->report, cycles);
	uint64_t cg = 0, nq = 0, q20 = 0, q30 = 0;
	for (uint64_t r = 0; r < v.rows; r++) {
		cg += v.base[4 * r + 1] + v.base[4 * r + 3];
		for (uint32_t q = 0; q < SDT_QC_NQ; q++) {
			const uint64_t x = v.qual[SDT_QC_NQ * r + q];
			nq += x;
			if (q >= 20) q20 += x;
			if (q >= 30) q30 += x;
		}
	}
	int at = snprintf(line, SDT_QC_LINE_MAX, "qc: class %d reads %llu empty %llu bases %llu gc %llu", k, (unsigned long long)v.totals[0],
	                  (unsigned long long)v.totals[1], (unsigned long long)v.totals[2], (unsigned long long)share_x100(cg, v.totals[2]));
	if (c->with_quals && nq)
		snprintf(line + at, SDT_QC_LINE_MAX - at, " q20 %llu q30 %llu\n", (unsigned long long)share_x100(q20, nq), (unsigned long long)share_x100(q30, nq));
	else
		snprintf(line + at, SDT_QC_LINE_MAX - at, " q20 - q30 -\n");
}
