/* asmsplit.c -- see asmsplit.h */
#include <inttypes.h>
#include <math.h>
#include <string.h>
#include "asmsplit.h"

void sdt_asm_fold(const sdt_ref_set *refs, const sdt_seq_support *seg, sdt_asm_contig *out)
{
	memset(out, 0, (size_t)refs->n_refs * sizeof *out);
	for (uint32_t i = 0; i < refs->n_refs; i++) out[i].bases = refs->bases[i];
	for (uint64_t j = 0; j < refs->nseqs; j++) {
		sdt_asm_contig *c = out + refs->ref_of_seq[j];
		const sdt_seq_support *s = seg + j;
		c->sum += s->sum;
		c->kmers += s->kmers;
		c->found += s->found;
		c->solid += s->solid;
		c->gaps += s->gaps;
		if (s->longest_gap > c->longest_gap) {                   /* (the segments of a contig come in its order: the first among equals stays) */
			c->longest_gap = s->longest_gap;
			c->longest_at = refs->seg_start[j] + s->longest_at;
		}
	}
	for (uint32_t i = 0; i < refs->n_refs; i++)
		if (!out[i].longest_gap) out[i].longest_at = out[i].kmers;
}

int sdt_asm_support_write(FILE *f, const sdt_ref_set *refs, const sdt_asm_contig *ctg)
{
	for (uint32_t i = 0; i < refs->n_refs; i++) {
		const sdt_asm_contig *c = ctg + i;
		if (fprintf(f, "%u %s %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", i + 1, refs->names[i],
		            c->bases, c->kmers, c->found, c->solid, c->sum, c->gaps, c->longest_gap, c->longest_at) < 0)
			return -1;
	}
	return 0;
}

int sdt_asm_spectrum_write(FILE *f, const uint64_t *matrix, uint32_t rows)
{
	for (uint32_t r = 0; r < rows; r++) {
		const uint64_t *m = matrix + (size_t)r * SDT_ASM_CN_COLS;
		uint64_t any = 0;
		for (int c = 0; c < SDT_ASM_CN_COLS; c++) any |= m[c];
		if (!any) continue;
		if (fprintf(f, "%u", r) < 0) return -1;
		for (int c = 0; c < SDT_ASM_CN_COLS; c++)
			if (fprintf(f, " %" PRIu64, m[c]) < 0) return -1;
		if (fputc('\n', f) == EOF) return -1;
	}
	return 0;
}

int sdt_asm_nodes_of(const uint64_t *matrix, uint32_t rows, uint32_t min_count, sdt_asm_nodes *out)
{
	if (rows <= min_count) return -1;
	memset(out, 0, sizeof *out);
	for (uint32_t r = 0; r < rows; r++)
		for (int c = 0; c < SDT_ASM_CN_COLS; c++) {
			const uint64_t v = matrix[(size_t)r * SDT_ASM_CN_COLS + c];
			out->nodes += v;
			if (r >= min_count) {
				out->solid_nodes += v;
				if (c >= 1) out->covered += v;
			}
		}
	return 0;
}

void sdt_asm_summary(char line[SDT_ASM_SUMMARY_MAX], const uint64_t totals[4], const sdt_asm_nodes *nodes, int K)
{
	char p[32], q[32];
	const uint64_t N = totals[1], V = totals[3];
	if (nodes->solid_nodes == 0) strcpy(p, "-");
	else snprintf(p, sizeof p, "%" PRIu64, (uint64_t)(((unsigned __int128)nodes->covered * 10000u) / nodes->solid_nodes));
	if (N == 0) strcpy(q, "-");
	else if (V == N) strcpy(q, "inf");
	else snprintf(q, sizeof q, "%ld", lround(100.0 * -10.0 * log10(1.0 - pow((double)V / (double)N, 1.0 / (double)K))));
	snprintf(line, SDT_ASM_SUMMARY_MAX,
	         "evaluate: sequences %" PRIu64 " kmers %" PRIu64 " found %" PRIu64 " solid %" PRIu64 " nodes %" PRIu64 " solid_nodes %" PRIu64 " covered %" PRIu64
	         " completeness_x100 %s qv_x100 %s\n",
	         totals[0], N, totals[2], V, nodes->nodes, nodes->solid_nodes, nodes->covered, p, q);
}
