/* screensplit.h -- the host side of `sdt-kmers screen` that needs no device: the reference files (FASTA) as the packed segments that
 * sdt_gpu_screen_load takes, what a read's record line looks like, whether a record can be that of a read of a given length, and the
 * statistics per reference with their summary line.  Where a read goes is trimsplit.h's sdt_trim_route.
 * Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/screen_host_check.c links it on its own. */
#ifndef SDT_SCREENSPLIT_H
#define SDT_SCREENSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* The references of one or more FASTA files, in the order they were read: reference i has names[i] (the header up to the first blank)
 * and bases[i] letters A, C, G, T.  Every other letter cuts the reference: the stretches between are the segments, packed like reads
 * (16 bases per word, the first in the most significant pair), segment j = bases [offsets[j], offsets[j + 1]) of reference
 * ref_of_seq[j].  A reference may have no segment at all (only N). */
typedef struct {
	uint8_t *codes;                 /* one base per byte while the files are read */
	uint64_t ncodes, codes_cap;
	uint64_t *offsets;              /* nseqs + 1 once a segment exists */
	uint32_t *ref_of_seq;
	uint64_t nseqs, seqs_cap;
	char **names;
	uint64_t *bases;
	uint32_t n_refs, refs_cap;
	uint32_t *words;                /* sdt_refs_pack */
	uint64_t nwords;
	uint64_t *seg_start;            /* per segment: where it starts inside its reference, counting every letter of the record (0-based) */
} sdt_ref_set;

/* One FASTA text of n bytes appended to the set.  Letters in either case; wrapped lines are joined; blank lines, blanks and '\r' are
 * skipped.  0, or -1 with "label line N: ..." in err: bases before the first header (N: their line), a record without any sequence
 * character (N: its header's line); "label: out of memory". */
int sdt_refs_parse(sdt_ref_set *s, const char *label, const char *text, size_t n, char *err, size_t errcap);
/* the file at path, label = path; also -1 with "cannot read path" */
int sdt_refs_load(sdt_ref_set *s, const char *path, char *err, size_t errcap);
/* codes -> words with the four pad words of sdt_gpu_push_reads; offsets is then valid even without a segment.  0, or -1: out of memory */
int sdt_refs_pack(sdt_ref_set *s);
void sdt_refs_free(sdt_ref_set *s);

/* "kmers hits ref verdict\n", ref 1-based and 0 for none; returns the end of what it wrote (at most SDT_SCREEN_LINE_MAX bytes) */
enum { SDT_SCREEN_LINE_MAX = 4 * 11 };
char *sdt_put_screen_line(char *p, const sdt_read_screen *r);

/* is a read with this record MATCHED under the rule of include/sdt_gpu.h */
int sdt_screen_matched(const sdt_read_screen *r, const sdt_screen_params *prm);

/* 1 iff r can be the record of a read of read_len bases screened with k-mers of k bases against n_refs references: the k-mers of a read
 * of that length, no more hits than k-mers, a reference iff there is a hit, start 0, verdict 0 with len = read_len or 1 with len 0 */
int sdt_screen_record_ok(const sdt_read_screen *r, uint64_t read_len, uint32_t k, uint32_t n_refs);

/* per reference: the reads attributed to it (ref = it) and the sum of their hits; the reads counted */
typedef struct {
	uint64_t *reads, *hits;
	uint32_t n_refs;
	uint64_t total, matched, kept, dropped;
} sdt_screen_stats;
int sdt_screen_stats_init(sdt_screen_stats *st, uint32_t n_refs);               /* 0, or -1: out of memory */
/* one read: 0, or -2 (nothing noted) when sdt_screen_record_ok fails */
int sdt_screen_stats_note(sdt_screen_stats *st, const sdt_read_screen *r, uint64_t read_len, uint32_t k, const sdt_screen_params *prm);
/* "index name bases reads hits" per reference, index 1-based, then "# reads R matched M kept K dropped D"; 0, or -1 when a write failed */
int sdt_screen_stats_write(FILE *f, const sdt_screen_stats *st, const sdt_ref_set *refs);
void sdt_screen_stats_free(sdt_screen_stats *st);

#endif
