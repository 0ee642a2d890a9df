/* clipsplit.h -- the host side of `sdt-kmers clip` that needs no device: adapter FASTA files into the packed adapter set of
 * include/sdt_gpu.h, what a read's record line looks like, and the statistics of a stream's records.  Where a read goes is
 * trimsplit.h's sdt_trim_route.  Plain C, no GPU library (include/sdt_gpu.h only for the types): tools/clip_host_check.c links it on its own. */
#ifndef SDT_CLIPSPLIT_H
#define SDT_CLIPSPLIT_H
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* the adapters of one or more FASTA files, in the order they were read: what sdt_adapter_set points into, and their names */
typedef struct {
	uint32_t *words;            /* 16 bases per word, the first in the most significant pair; one zero word behind the last base */
	uint64_t *offsets;          /* n + 1, in bases */
	uint8_t *ends;              /* 0: 3', 1: 5' */
	char **names;               /* the header line up to the first blank */
	uint32_t n;
	size_t cap, wcap;
} sdt_adapter_list;

/* The records of a FASTA text (len bytes, label: the file's name for the messages) appended as adapters of `end`.  Letters A, C, G, T
 * in either case, coded as host/seqio.h codes reads (A0 C1 T2 G3); the sequence may be wrapped over lines; blank lines are skipped.
 * Refused, with "label line N: ..." in err and nothing of the text appended: any other letter, bases before the first header, a
 * record without bases, a record of more than SDT_CLIP_MAX_ADAPTER_LEN bases, more than SDT_CLIP_MAX_ADAPTERS adapters in all.
 * Returns 0, or -1 (err is filled; out of memory says so). */
int sdt_adapters_parse(sdt_adapter_list *l, const char *text, size_t len, const char *label, int end, char *err, size_t errlen);
/* the same for a file */
int sdt_adapters_load(sdt_adapter_list *l, const char *path, int end, char *err, size_t errlen);
void sdt_adapters_free(sdt_adapter_list *l);
/* the set as the library takes it (points into l) */
sdt_adapter_set sdt_adapters_set(const sdt_adapter_list *l);

/* "adapter3 adapter5 tail3 tail5 start len verdict\n" (adapters 1-based, 0: none); returns the end of what it wrote (at most
 * SDT_CLIP_LINE_MAX bytes) */
enum { SDT_CLIP_LINE_MAX = 7 * 11 };
char *sdt_put_clip_line(char *p, const sdt_read_clip *c);

/* per adapter: the reads it bounded and the bases it removed from them; per tail rule the same; the reads by verdict.  The record of
 * a dropped read does not say where its bounds were: it counts as a read for its adapters and tails, its bases only for the tails. */
typedef struct {
	uint64_t *reads, *bases;    /* n each */
	uint32_t n;
	uint64_t tail_reads[2], tail_bases[2];      /* [0]: 3', [1]: 5' */
	uint64_t whole, clipped, dropped;
} sdt_clip_stats;
int sdt_clip_stats_init(sdt_clip_stats *s, uint32_t n_adapters);                 /* 0, or -1: out of memory */
/* one read of read_len bases; -1 (nothing noted) when the record cannot be one of n adapters and such a read */
int sdt_clip_stats_note(sdt_clip_stats *s, const sdt_read_clip *c, uint64_t read_len);
/* one line per adapter "index name end reads bases" (index 1-based, end 3 or 5), "tail3 reads bases", "tail5 reads bases",
 * "whole n", "clipped n", "dropped n"; 0, or -1 when a write failed */
int sdt_clip_stats_write(FILE *f, const sdt_clip_stats *s, const sdt_adapter_list *l);
void sdt_clip_stats_free(sdt_clip_stats *s);

#endif
