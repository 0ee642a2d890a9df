/* threadsplit.h -- the host side of `sdt-kmers thread` that needs no device: the lines of prefix.readPaths and of prefix.unitigReads
 * and the summary line, as pure functions of the arrays that sdt_gpu_unitigs_reads gives.  Ids are 1-based in every text.  Plain C,
 * no GPU library (include/sdt_gpu.h only for the records' types): tools/thread_host_check.c links it on its own. */
#ifndef SDT_THREADSPLIT_H
#define SDT_THREADSPLIT_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "../../../include/sdt_gpu.h"

/* what the reads left on the unitigs and what the summary line says.  Per unitig by 0-based id: the reads with at least one segment
 * in it, its segments, their k-mers; mark: the last read that was counted for the unitig, + 1 */
typedef struct {
	uint64_t reads, placed, whole, broken, unplaced, too_short, segments, linked, unlinked;
	uint64_t n_unitigs, *u_reads, *u_segs, *u_kmers, *mark;
} sdt_thread_tally;

/* 0, or -1: out of memory */
int sdt_thread_tally_init(sdt_thread_tally *t, uint64_t n_unitigs);
void sdt_thread_tally_free(sdt_thread_tally *t);

/* the path of one read: "*" without a segment, else per segment <sep><dir><id>:<unitig_pos>+<kmers> -- sep: none for the first, '-'
 * join 1 (linked), '~' join 2 (adjacent in the read, no edge of the graph), '/' join 0 (after a gap); dir: '>' o = 0, '<' o = 1.
 * 0, or -1 when a write failed */
int sdt_thread_path_write(FILE *f, const sdt_path_seg *segs, uint64_t n);

/* one read in stream order: the line "kmers live segs breaks path" and the tally.  segs: the rec->segs segments of this read.  0; -1
 * when a write failed; -2 when the record and its segments disagree (a unitig id past n_unitigs, segments that do not sum to live) */
int sdt_thread_read_write(FILE *f, const sdt_read_path *rec, const sdt_path_seg *segs, sdt_thread_tally *t);

/* per unitig in id order "id reads segments kmers".  0, or -1 when a write failed */
int sdt_thread_unitig_reads_write(FILE *f, const sdt_thread_tally *t);

/* "thread: reads R placed P whole W broken B unplaced U short S segments G linked L unlinked X\n" -- placed: at least one segment;
 * whole: live == kmers and breaks == 0; broken: placed and not whole; unplaced: k-mers and no segment; short: no k-mer */
enum { SDT_THREAD_SUMMARY_MAX = 320 };
void sdt_thread_summary(char line[SDT_THREAD_SUMMARY_MAX], const sdt_thread_tally *t);

#endif
