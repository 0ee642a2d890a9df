/* supportsplit.c -- see supportsplit.h */
#include "supportsplit.h"
#include "unitigsplit.h"

#define OU(x) (unsigned long long)((x) >> 1) + 1, ((x) & 1u) ? '-' : '+'

int sdt_support_unitigs_write(FILE *f, const sdt_unitig *rec, const sdt_unitig_support *sup, uint64_t first, uint64_t n)
{
	for (uint64_t i = 0; i < n; i++) {
		if (rec[i].nodes == 0) return -2;
		/* (kmers is below 2^57 for any tally that a device holds: the product fits) */
		if (fprintf(f, "%llu %llu %llu %llu\n", (unsigned long long)(first + i) + 1, (unsigned long long)sup[i].segs, (unsigned long long)sup[i].kmers,
		            (unsigned long long)(sup[i].kmers * 100 / rec[i].nodes)) < 0)
			return -1;
	}
	return 0;
}

int sdt_support_links_write(FILE *f, const sdt_unitig_link *links, const sdt_link_support *sup, uint64_t n_links)
{
	for (uint64_t j = 0; j < n_links; j++) {
		const sdt_unitig_link *l = links + j;
		if (!sdt_unitig_link_written(l)) continue;
		if (fprintf(f, "%llu %c %llu %c %llu %llu\n", (unsigned long long)l->from + 1, l->info & 1u ? '-' : '+', (unsigned long long)l->to + 1,
		            l->info >> 1 & 1u ? '-' : '+', (unsigned long long)sup[j].along, (unsigned long long)sup[j].against) < 0)
			return -1;
	}
	return 0;
}

int sdt_support_junctions_write(FILE *f, const sdt_unitig_junction *j, uint64_t n)
{
	for (uint64_t i = 0; i < n; i++) {
		if (j[i].via & 1u) return -2;
		if (i && !(j[i - 1].via < j[i].via || (j[i - 1].via == j[i].via && (j[i - 1].from < j[i].from || (j[i - 1].from == j[i].from && j[i - 1].to < j[i].to)))))
			return -2;
		if (fprintf(f, "%llu%c %llu%c %llu%c %llu\n", OU(j[i].from), OU(j[i].via), OU(j[i].to), (unsigned long long)j[i].count) < 0) return -1;
	}
	return 0;
}

void sdt_support_summary(char line[SDT_SUPPORT_SUMMARY_MAX], const uint64_t totals[12], uint64_t n_junctions)
{
	const unsigned long long *t = (const unsigned long long *)totals;
	snprintf(line, SDT_SUPPORT_SUMMARY_MAX, "support: reads %llu placed %llu segments %llu kmers %llu traversals %llu no_record %llu passages %llu junctions %llu dropped %llu\n",
	         t[0], t[1], t[2], t[3], t[4], t[5], t[6], (unsigned long long)n_junctions, t[11]);
}
