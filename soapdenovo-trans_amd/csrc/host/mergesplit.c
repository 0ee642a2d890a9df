/* mergesplit.c -- see mergesplit.h */
#include <string.h>
#include "mergesplit.h"
#include "putdec.h"

char *sdt_put_merge_line(char *p, const sdt_read_merge *r)
{
	p = sdt_put_dec(p, r->merged, ' ');
	p = sdt_put_dec(p, r->mismatches, ' ');
	p = sdt_put_dec(p, r->from_b, ' ');
	p = sdt_put_dec(p, r->start, ' ');
	p = sdt_put_dec(p, r->len, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

int sdt_merge_record_ok(const sdt_read_merge *r, const sdt_read_overlap *ov, uint64_t read_len)
{
	if (r->merged == 0)
		return r->mismatches == 0 && r->from_b == 0 && r->start == ov->start && r->len == ov->len && r->verdict == ov->verdict;
	if (r->merged != ov->insert || r->verdict != SDT_MERGE_MERGED || r->start != 0 || r->len != 0) return 0;
	if (r->mismatches > read_len || r->mismatches > r->merged) return 0;
	return r->from_b <= r->mismatches;
}

int sdt_merge_stats_note(sdt_merge_stats *s, const sdt_read_merge *a, const sdt_read_merge *b, const sdt_read_overlap *oa, const sdt_read_overlap *ob)
{
	if (a->merged != b->merged || a->mismatches != b->mismatches || a->from_b != b->from_b) return -2;
	if ((a->verdict == SDT_MERGE_MERGED) != (b->verdict == SDT_MERGE_MERGED) || (a->verdict == SDT_MERGE_MERGED) != (a->merged != 0)) return -2;
	if (oa->insert != ob->insert || (a->merged && a->merged != oa->insert)) return -2;
	s->pairs++;
	s->overlapping += oa->insert != 0;
	if (a->merged) {
		s->merged++;
		s->columns += a->mismatches;
		s->from_b += a->from_b;
		s->merged_bases += a->merged;
	}
	return 0;
}

int sdt_merge_summary(char *buf, size_t n, const sdt_merge_stats *s, uint64_t reads, uint64_t bases_in, uint64_t bases_out)
{
	return snprintf(buf, n, "merge: reads %llu pairs %llu overlapping %llu merged %llu mismatch columns %llu bases in %llu bases out %llu",
	                (unsigned long long)reads, (unsigned long long)s->pairs, (unsigned long long)s->overlapping, (unsigned long long)s->merged,
	                (unsigned long long)s->columns, (unsigned long long)bases_in, (unsigned long long)(bases_out + s->merged_bases));
}
