/* readwalk.c -- see readwalk.h */
#include <stdlib.h>
#include <string.h>
#include "readwalk.h"
#include "trimsplit.h"
#include "putdec.h"

int ob_open(outbuf *o, const char *path)
{
	o->path = path;
	o->f = fopen(path, "w");
	if (!o->f) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path); return -1; }
	o->buf = o->p = (char *)malloc(OB_BLOCK);
	o->ok = 1;
	if (!o->buf) { fprintf(stderr, "sdt-kmers: out of memory\n"); fclose(o->f); o->f = NULL; return -1; }
	return 0;
}

void ob_room(outbuf *o, size_t need)
{
	if ((size_t)(o->p - o->buf) + need > OB_BLOCK) {
		if (o->ok) o->ok = fwrite(o->buf, 1, (size_t)(o->p - o->buf), o->f) == (size_t)(o->p - o->buf);
		o->p = o->buf;
	}
}

int ob_close(outbuf *o)
{
	if (o->ok && o->p != o->buf) o->ok = fwrite(o->buf, 1, (size_t)(o->p - o->buf), o->f) == (size_t)(o->p - o->buf);
	free(o->buf);
	if (fclose(o->f) != 0) o->ok = 0;
	if (!o->ok) fprintf(stderr, "sdt-kmers: write to %s failed\n", o->path);
	return o->ok ? 0 : -1;
}

int kept_init(kept_reads *k, uint64_t nb, uint64_t reads)
{
	const uint64_t m = reads ? reads : 1;
	memset(k, 0, sizeof *k);
	k->nb = nb;
	k->reads = reads;
	k->bw = (uint32_t **)calloc(nb ? nb : 1, sizeof(uint32_t *));
	k->bo = (uint64_t **)calloc(nb ? nb : 1, sizeof(uint64_t *));
	k->at_batch = (uint32_t *)malloc(m * sizeof(uint32_t));
	k->at_read = (uint32_t *)malloc(m * sizeof(uint32_t));
	if (!k->bw || !k->bo || !k->at_batch || !k->at_read) { fprintf(stderr, "sdt-kmers: out of memory\n"); return 1; }
	memset(k->at_batch, 0xFF, m * sizeof(uint32_t));
	return 0;
}

int kept_add(kept_reads *k, uint64_t b, uint32_t *words, uint64_t *offsets, uint64_t nreads, uint64_t ord_base, uint64_t ord_stride)
{
	k->bw[b] = words;
	k->bo[b] = offsets;
	for (uint64_t i = 0; i < nreads; i++) {
		const uint64_t ord = ord_base + i * ord_stride;
		if (ord >= k->reads) { fprintf(stderr, "sdt-kmers: a kept read has ordinal %llu of %llu\n", (unsigned long long)ord, (unsigned long long)k->reads); return 1; }
		k->at_batch[ord] = (uint32_t)b;
		k->at_read[ord] = (uint32_t)i;
		if (offsets[i + 1] - offsets[i] > k->longest) k->longest = offsets[i + 1] - offsets[i];
	}
	return 0;
}

void kept_free(kept_reads *k)
{
	for (uint64_t b = 0; b < k->nb; b++) { free(k->bw[b]); free(k->bo[b]); }
	free(k->bw); free(k->bo); free(k->at_batch); free(k->at_read);
	memset(k, 0, sizeof *k);
}

int sdt_walk_reads(const kept_reads *k, const sdt_pair_ranges *pairs, const char *prefix, const sdt_walk_stage *stage, void *state,
                   uint64_t n_kept, sdt_walk_tally *tally)
{
	static const sdt_pair_ranges no_pairs = {NULL, 0, 0};
	if (!pairs) pairs = &no_pairs;
	memset(tally, 0, sizeof *tally);
	if (k->longest + 64 > OB_BLOCK) { fprintf(stderr, "sdt-kmers: a read of %llu bases\n", (unsigned long long)k->longest); return 1; }
	char path[3][4200];
	outbuf out[3];                                                           /* the record lines, the pairs, the singles */
	for (int i = 0; i < 3; i++) {
		if (!stage->suffix[i]) { out[i].f = NULL; continue; }
		snprintf(path[i], sizeof path[i], "%s%s", prefix, stage->suffix[i]);
		if (ob_open(&out[i], path[i]) != 0) {
			while (i--) if (out[i].f) ob_close(&out[i]);
			return 1;
		}
	}
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < k->reads; ord++) {
		if (!out[0].ok || (out[1].f && !out[1].ok) || !out[2].ok) break;    /* a write failed: ob_close says which */
		if (k->at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		uint32_t *w = k->bw[k->at_batch[ord]];
		const uint64_t at = k->bo[k->at_batch[ord]][k->at_read[ord]], read_len = k->bo[k->at_batch[ord]][k->at_read[ord] + 1] - at;
		uint64_t start = 0, len = read_len;
		if (stage->note(state, ord, read_len, &start, &len) != 0) { bad = 1; break; }
		ob_room(&out[0], stage->line_max);
		out[0].p = stage->put_line(state, out[0].p, ord);
		tally->bases_in += read_len;
		if (stage->edit && stage->edit(state, ord, w, at, read_len) != 0) { bad = 1; break; }
		const int to = stage->unit ? (!stage->alive(state, ord) ? SDT_TRIM_TO_NONE : (sdt_pair_ranges_holds(pairs, ord, &cursor) ? SDT_TRIM_TO_PAIRS : SDT_TRIM_TO_SINGLE))
		                           : sdt_trim_route(pairs, &cursor, stage->alive, state, k->reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		tally->kept++;
		tally->bases_out += len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS && out[1].f ? &out[1] : &out[2];
		ob_room(o, (size_t)len + 24 + SDT_WALK_NAME_TAIL_MAX);
		if (stage->name_tail) {
			*o->p++ = '>';
			o->p = stage->name_tail(state, sdt_put_dec(o->p, ord + 1, ' '), ord);
			o->p = sdt_put_fasta_bases(o->p, w, at + start, len);
		} else {
			o->p = sdt_put_fasta_record(o->p, ord, w, at + start, len);
		}
	}
	const int all_written = out[0].ok && (!out[1].f || out[1].ok) && out[2].ok;
	if ((ob_close(&out[0]) != 0) | (out[1].f && ob_close(&out[1]) != 0) | (ob_close(&out[2]) != 0) || bad) return 1;
	if (all_written && tally->kept != n_kept) {
		fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, tally->kept);
		return 1;
	}
	return 0;
}
