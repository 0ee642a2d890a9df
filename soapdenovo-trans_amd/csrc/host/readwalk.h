/* readwalk.h -- the host side of every read stage of `sdt-kmers` that needs no device: the block buffer the text files are written
 * through, where every ordinal's read lies in the kept batches, and the one walk over the ordinals that writes a stage's record
 * lines and its two FASTA files.  What a stage is comes as a few callbacks (sdt_walk_stage); its statistics file and its summary line
 * are its own business after the walk.  Plain C, no GPU library: tools/readwalk_host_check.c links it on its own. */
#ifndef SDT_READWALK_H
#define SDT_READWALK_H
#include <stdio.h>
#include "normsplit.h"

/* text formatted by hand into a block buffer */
typedef struct { FILE *f; char *buf, *p; int ok; const char *path; } outbuf;
enum { OB_BLOCK = 1 << 20 };
int ob_open(outbuf *o, const char *path);                                    /* 0, or -1 after saying why; path must outlive o */
/* room for `need` more bytes (need <= OB_BLOCK); after a failed write the block is dropped, never overrun: the caller stops on !ok */
void ob_room(outbuf *o, size_t need);
int ob_close(outbuf *o);                                                     /* 0, or -1 after naming the file a write to which failed */

/* the kept batches, and where every ordinal's read is */
typedef struct {
	uint64_t nb, reads, longest;
	uint32_t **bw;                                                           /* words of batch b */
	uint64_t **bo;                                                           /* offsets of batch b */
	uint32_t *at_batch, *at_read;                                            /* by ordinal; at_batch 0xFFFFFFFF: no kept read has it */
} kept_reads;
/* room for nb batches of a stream of `reads` ordinals; 0, or 1 after saying that memory ran out */
int kept_init(kept_reads *k, uint64_t nb, uint64_t reads);
/* batch b: nreads reads with the ordinals ord_base + i * ord_stride, offsets[nreads + 1] in bases into words; both arrays are malloc'ed
 * and belong to k from here on.  0, or 1 after naming the ordinal that the stream does not have */
int kept_add(kept_reads *k, uint64_t b, uint32_t *words, uint64_t *offsets, uint64_t nreads, uint64_t ord_base, uint64_t ord_stride);
void kept_free(kept_reads *k);

/* what a stage says about itself; `state` is the stage's own */
typedef struct {
	const char *suffix[3];                  /* behind the prefix: the record lines, the pairs file (NULL: the stage has none), the singles file */
	size_t line_max;                        /* of a record line */
	int unit;                               /* the mates of a pair are decided together: a kept read of a pair range goes to the pairs file */
	/* the record of read `ord` of read_len bases, noted or checked; *start and *len come as the whole read and are set where the
	 * record keeps a part.  0, or -1 after saying why: an impossible record (its fields are printed), memory */
	int (*note)(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len);
	char *(*put_line)(const void *state, char *p, uint64_t ord);                /* at most line_max bytes; returns their end */
	int (*alive)(const void *state, uint64_t ord);                              /* sdt_alive_fn of trimsplit.h: is anything of it kept */
	/* NULL, or what changes the read (read_len bases from `start` of words) before its FASTA record is written; 0, or -1 */
	int (*edit)(void *state, uint64_t ord, uint32_t *words, uint64_t start, uint64_t read_len);
	/* NULL, or what follows "><read number> " in the name line of a FASTA record, newline included; at most SDT_WALK_NAME_TAIL_MAX bytes */
	char *(*name_tail)(const void *state, char *p, uint64_t ord);
} sdt_walk_stage;
enum { SDT_WALK_NAME_TAIL_MAX = 40 };

typedef struct { unsigned long long kept, bases_in, bases_out; } sdt_walk_tally;   /* reads written; bases of all reads; bases written */

/* The files prefix + suffix[] opened, the ordinals [0, k->reads) once in order, the files closed.  Per ordinal: a write failed: stop
 * (ob_close says which); no kept read has it: refused; note; the record line; edit; the route (trimsplit.h; pairs NULL: no pair
 * ranges); the FASTA record of what the record keeps.  Then the reads written must be the n_kept that the device counted.
 * Returns 0, or 1 after saying why.  A read of more than OB_BLOCK - 64 bases is refused before a file is opened. */
int sdt_walk_reads(const kept_reads *k, const sdt_pair_ranges *pairs, const char *prefix, const sdt_walk_stage *stage, void *state,
                   uint64_t n_kept, sdt_walk_tally *tally);

#endif
