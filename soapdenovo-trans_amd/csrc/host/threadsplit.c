/* threadsplit.c -- see threadsplit.h */
#include "threadsplit.h"
#include <stdlib.h>
#include <string.h>

int sdt_thread_tally_init(sdt_thread_tally *t, uint64_t n_unitigs)
{
	memset(t, 0, sizeof *t);
	const size_t n = n_unitigs ? (size_t)n_unitigs : 1;
	t->n_unitigs = n_unitigs;
	t->u_reads = (uint64_t *)calloc(n, sizeof(uint64_t));
	t->u_segs = (uint64_t *)calloc(n, sizeof(uint64_t));
	t->u_kmers = (uint64_t *)calloc(n, sizeof(uint64_t));
	t->mark = (uint64_t *)calloc(n, sizeof(uint64_t));
	if (t->u_reads && t->u_segs && t->u_kmers && t->mark) return 0;
	sdt_thread_tally_free(t);
	return -1;
}

void sdt_thread_tally_free(sdt_thread_tally *t)
{
	free(t->u_reads); free(t->u_segs); free(t->u_kmers); free(t->mark);
	t->u_reads = t->u_segs = t->u_kmers = t->mark = NULL;
}

int sdt_thread_path_write(FILE *f, const sdt_path_seg *segs, uint64_t n)
{
	if (n == 0) return fputc('*', f) == EOF ? -1 : 0;
	for (uint64_t j = 0; j < n; j++) {
		const uint32_t o = segs[j].info & 1u, join = segs[j].info >> 1;
		char sep[2] = {join == 1 ? '-' : join == 2 ? '~' : '/', 0};
		if (j == 0) sep[0] = 0;
		if (fprintf(f, "%s%c%llu:%u+%u", sep, o ? '<' : '>', (unsigned long long)segs[j].unitig + 1, segs[j].unitig_pos, segs[j].kmers) < 0) return -1;
	}
	return 0;
}

int sdt_thread_read_write(FILE *f, const sdt_read_path *rec, const sdt_path_seg *segs, sdt_thread_tally *t)
{
	uint64_t kmers = 0;
	for (uint32_t j = 0; j < rec->segs; j++) {
		if (segs[j].unitig >= t->n_unitigs) return -2;
		kmers += segs[j].kmers;
	}
	if (kmers != rec->live) return -2;
	if (fprintf(f, "%u %u %u %u ", rec->kmers, rec->live, rec->segs, rec->breaks) < 0 || sdt_thread_path_write(f, segs, rec->segs) != 0 || fputc('\n', f) == EOF) return -1;
	t->reads++;
	const int whole = rec->segs && rec->live == rec->kmers && rec->breaks == 0;
	if (rec->segs) { t->placed++; if (whole) t->whole++; else t->broken++; }
	else if (rec->kmers) t->unplaced++;
	else t->too_short++;
	t->segments += rec->segs;
	for (uint32_t j = 0; j < rec->segs; j++) {
		const uint32_t u = segs[j].unitig, join = segs[j].info >> 1;
		t->linked += join == 1;
		t->unlinked += join == 2;
		t->u_segs[u]++;
		t->u_kmers[u] += segs[j].kmers;
		if (t->mark[u] != t->reads) { t->mark[u] = t->reads; t->u_reads[u]++; }      /* (reads was just raised: this read's number from 1) */
	}
	return 0;
}

int sdt_thread_unitig_reads_write(FILE *f, const sdt_thread_tally *t)
{
	for (uint64_t u = 0; u < t->n_unitigs; u++)
		if (fprintf(f, "%llu %llu %llu %llu\n", (unsigned long long)u + 1, (unsigned long long)t->u_reads[u], (unsigned long long)t->u_segs[u],
		            (unsigned long long)t->u_kmers[u]) < 0)
			return -1;
	return 0;
}

void sdt_thread_summary(char line[SDT_THREAD_SUMMARY_MAX], const sdt_thread_tally *t)
{
	snprintf(line, SDT_THREAD_SUMMARY_MAX, "thread: reads %llu placed %llu whole %llu broken %llu unplaced %llu short %llu segments %llu linked %llu unlinked %llu\n",
	         (unsigned long long)t->reads, (unsigned long long)t->placed, (unsigned long long)t->whole, (unsigned long long)t->broken,
	         (unsigned long long)t->unplaced, (unsigned long long)t->too_short, (unsigned long long)t->segments, (unsigned long long)t->linked,
	         (unsigned long long)t->unlinked);
}
