/* clustersplit.c -- see clustersplit.h */
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include "clustersplit.h"
#include "putdec.h"

char *sdt_put_cluster_line(char *p, const sdt_read_cluster *r)
{
	p = sdt_put_dec(p, r->kmers, ' ');
	p = sdt_put_dec(p, r->live, ' ');
	p = sdt_put_dec(p, r->split, ' ');
	p = sdt_put_dec(p, sdt_cluster_text_id(r->cluster), ' ');
	p = sdt_put_dec(p, sdt_cluster_text_id(r->unit), ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

char *sdt_put_cluster_name_tail(char *p, const sdt_read_cluster *r)
{
	memcpy(p, "cluster=", 8);
	return sdt_put_dec(p + 8, sdt_cluster_text_id(r->unit), '\n');
}

int sdt_cluster_parse_pick(const char *text, uint32_t pick[2])
{
	unsigned long long v[2];
	const char *s = text;
	for (int i = 0; i < 2; i++) {
		char *end = NULL;
		if (*s < '0' || *s > '9') return -1;
		errno = 0;
		v[i] = strtoull(s, &end, 10);
		if (errno || v[i] < 1 || v[i] > 0xFFFFFFFFULL || *end != (i == 0 ? ':' : '\0')) return -1;
		s = end + 1;
	}
	if (v[0] > v[1]) return -1;
	pick[0] = (uint32_t)(v[0] - 1);
	pick[1] = (uint32_t)(v[1] - 1);
	return 0;
}

int sdt_cluster_tally_init(sdt_cluster_tally *t, uint64_t n_clusters)
{
	memset(t, 0, sizeof *t);
	t->n_clusters = n_clusters;
	t->reads = (uint64_t *)calloc(n_clusters ? n_clusters : 1, sizeof(uint64_t));
	t->bases = (uint64_t *)calloc(n_clusters ? n_clusters : 1, sizeof(uint64_t));
	if (!t->reads || !t->bases) { sdt_cluster_tally_free(t); return -1; }
	return 0;
}

int sdt_cluster_tally_note(sdt_cluster_tally *t, const sdt_read_cluster *r, uint64_t read_len)
{
	if (r->verdict > 4 || (r->unit != SDT_CLUSTER_NONE && r->unit >= t->n_clusters) || (r->cluster != SDT_CLUSTER_NONE && r->cluster >= t->n_clusters)) return -1;
	t->all++;
	t->by_verdict[r->verdict]++;
	if (r->unit == SDT_CLUSTER_NONE) return 0;
	t->assigned++;
	t->reads[r->unit]++;
	t->bases[r->unit] += read_len;
	return 0;
}

uint64_t sdt_cluster_tally_largest_reads(const sdt_cluster_tally *t)
{
	uint64_t most = 0;
	for (uint64_t i = 0; i < t->n_clusters; i++)
		if (t->reads[i] > most) most = t->reads[i];
	return most;
}

void sdt_cluster_tally_free(sdt_cluster_tally *t)
{
	free(t->reads);
	free(t->bases);
	memset(t, 0, sizeof *t);
}

int sdt_cluster_list_write(FILE *f, const uint64_t *keys, const sdt_cluster_comp *comp, int nw, int K, const uint64_t info[8],
                           const sdt_cluster_tally *t)
{
	static const char letters[4] = {'A', 'C', 'T', 'G'};
	char line[21 + 128 + 11 + 3 * 21 + 8];
	for (uint64_t i = 0; i < t->n_clusters; i++) {
		char *p = sdt_put_dec(line, i + 1, ' ');
		for (int j = 0; j < K; j++) {
			const int bit = 2 * (K - 1 - j);                                    /* of the whole key; word nw - 1 holds the lowest 64 */
			*p++ = letters[(keys[i * (uint64_t)nw + (uint64_t)(nw - 1 - (bit >> 6))] >> (bit & 63)) & 3u];
		}
		*p++ = ' ';
		p = sdt_put_dec(p, comp[i].nodes, ' ');
		p = sdt_put_dec(p, comp[i].count_sum, ' ');
		p = sdt_put_dec(p, t->reads[i], ' ');
		p = sdt_put_dec(p, t->bases[i], '\n');
		if (fwrite(line, 1, (size_t)(p - line), f) != (size_t)(p - line)) return -1;
	}
	return fprintf(f, "# live %llu link_ends %llu clusters %llu largest %llu unassigned %llu\n", (unsigned long long)info[0], (unsigned long long)info[1],
	               (unsigned long long)info[2], (unsigned long long)info[3], t->all - t->assigned) < 0 ? -1 : 0;
}

void sdt_cluster_summary(char line[SDT_CLUSTER_SUMMARY_MAX], const uint64_t info[8], const sdt_cluster_tally *t)
{
	snprintf(line, SDT_CLUSTER_SUMMARY_MAX,
	         "cluster: reads %llu assigned %llu whole %llu through_mate %llu unassigned %llu short %llu clusters %llu largest_nodes %llu largest_reads %llu\n",
	         t->all, t->assigned, t->by_verdict[0], t->by_verdict[2], t->by_verdict[3], t->by_verdict[4], (unsigned long long)info[2],
	         (unsigned long long)info[3], (unsigned long long)sdt_cluster_tally_largest_reads(t));
}
