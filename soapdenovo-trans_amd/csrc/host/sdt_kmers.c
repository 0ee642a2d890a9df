/* sdt_kmers.c -- ask the counted node table: the same ingest as sdt-pregraph (library config, library order, truncation, paired
 * interleave and its read ordinals: libcfg.c, readstream.c, seqio.c), pass 1 on the device, optionally `-d`, then
 *
 *   sdt-kmers profile -s lib.cfg -K k [-p threads] [-d d] [-c min_count] -o prefix
 *       prefix.readCov: one line per read in stream order:  kmers found solid min median max   (sdt_gpu_profile_kept_reads)
 *   sdt-kmers query   -s lib.cfg -K k [-p threads] [-d d] -q kmers.txt [-o out.tsv]
 *       per input line:  <kmer> <found 0|1> <strand +|-> <count> <l: A C T G> <r: A C T G> <linear> <deleted>   (sdt_gpu_search_kmers,
 *       the batch form of search_kmerset, newhash.c:239-283; links as the STORED node has them, strand - = stored as the reverse
 *       complement of the query)
 *   sdt-kmers correct -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] -o prefix
 *       substitution errors corrected against the counted table (sdt_gpu_correct_kept_reads; the rule: include/sdt_gpu.h), in stream
 *       (ordinal) order, so paired files come out interleaved, read1 then read2:
 *       prefix.readFix: one line per read:  kmers weak runs fixed
 *       prefix.edits: one line per substitution, ascending:  read pos from to   (read = ordinal + 1, pos 1-based)
 *       prefix.corrected.fa: every read of the stream, > ordinal + 1 and the sequence on one line (the letters of the 2-bit codes)
 *   sdt-kmers normalize -s lib.cfg -K k [-p threads] [-d d] [--target C, default 50] [--max-cv PCT, default 10000, 0 = off]
 *                       [--seed S, default 0] -o prefix
 *       in-silico normalisation against the counted table (sdt_gpu_select_kept_reads; the rule: include/sdt_gpu.h): a read, or the two
 *       mates of a pair, is kept with probability target / median k-mer coverage; the batches of paired files (ord_stride 2) say which
 *       ordinals hold pairs (normsplit.c)
 *       prefix.readPick: one line per read in stream order:  kmers median cov verdict
 *       prefix.norm.pairs.fa: the kept pairs, read 1 then read 2, > ordinal + 1 and the sequence on one line: a p= file of a library
 *       prefix.norm.single.fa: the kept single reads: an f= file.  Library boundaries are not preserved: the pairs of all paired
 *       libraries go into the one pairs file.  Only pairs of files (q1=/q2=, f1=/f2=) come as ord_stride 2: an interleaved p= file
 *       is streamed with stride 1, so its reads are decided one by one and go into the singles file.
 *   sdt-kmers trim -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--min-cov Z, default 0] [--min-len L, default 0]
 *                  [--correct] -o prefix
 *       every read cut back to its longest solid stretch against the counted table (sdt_gpu_trim_kept_reads; the rule:
 *       include/sdt_gpu.h); with --correct the substitutions of `correct` are made first (sdt_gpu_correct_kept_reads and
 *       SDT_TRIM_CORRECTED).  Mates are trimmed independently; pairs as for normalize (normsplit.c, trimsplit.c)
 *       prefix.readTrim: one line per read in stream order:  kmers weak median start len verdict
 *       prefix.trim.pairs.fa: both mates of the pairs of which both survive, read 1 then read 2, > ordinal + 1 and the kept bases
 *       prefix.trim.single.fa: every other surviving read, the mate of a dropped read among them
 *       prefix.edits (--correct): as `correct` writes it
 *   sdt-kmers dedup -s lib.cfg -K k [-p threads] [--mate-swap] -o prefix
 *       exact copies of a read, or of a pair, dropped (sdt_gpu_dedup_kept_reads; the rule: include/sdt_gpu.h): of every class of equal
 *       units the first in stream order is kept; --mate-swap: pairs (a, b) and (b, a) are copies too.  Pairs as for normalize
 *       prefix.readDup: one line per read in stream order:  first copies verdict   (first = the ordinal of the kept unit's first read)
 *       prefix.dedup.pairs.fa / prefix.dedup.single.fa: the kept pairs / single reads, as normalize writes them
 *       prefix.dupLevels: one line per class size present, ascending:  copies classes reads   (dupsplit.c)
 *   sdt-kmers clip -s lib.cfg -K k [-p threads] [-a adapters3.fa] [-g adapters5.fa] [--tail3 LETTERS] [--tail5 LETTERS]
 *                  [--min-overlap N, default 5] [--error-pct P, default 10] [--min-tail N, default 10] [--tail-error-pct P, default 20]
 *                  [--min-len L, default 0] -o prefix
 *       sequencing adapters and poly-A/T tails clipped from every read (sdt_gpu_clip_kept_reads; the rule: include/sdt_gpu.h).  The
 *       adapter files are FASTA, letters ACGT in either case, read and checked before the device is touched; -a: 3' adapters, -g: 5'
 *       adapters, the 3' file first in the numbering.  Mates are clipped independently; pairs and routing as for trim (clipsplit.c)
 *       prefix.readClip: one line per read in stream order:  adapter3 adapter5 tail3 tail5 start len verdict
 *       prefix.clip.pairs.fa / prefix.clip.single.fa: the kept bases of the surviving reads, as trim writes them
 *       prefix.clipStats: per adapter  index name end reads bases,  then tail3 / tail5  reads bases,  then whole, clipped, dropped
 *   sdt-kmers overlap -s lib.cfg -K k [-p threads] [--min-overlap N, default 30] [--max-err PCT, default 10] [--min-len L, default 0]
 *                     -o prefix
 *       the overlap of the two mates of every pair, and what lies past the fragment's end clipped from both mates without an adapter
 *       list (sdt_gpu_overlap_kept_pairs; the rule: include/sdt_gpu.h).  Pairs as for normalize, routing as for clip; a library
 *       without pairs is allowed: every read is whole (overlapsplit.c)
 *       prefix.readOverlap: one line per read in stream order:  overlap mismatches insert start len verdict
 *       prefix.overlap.pairs.fa / prefix.overlap.single.fa: the kept bases of the surviving reads, as clip writes them
 *       prefix.insertHist: per insert that occurs, ascending:  insert pairs,  then  # pairs P overlapping V clipped C median M
 *   sdt-kmers complexity -s lib.cfg -K k [-p threads] [--max-score P, default 10] [--max-low Q, default 50] [--trim-low]
 *                        [--min-len L, default 0] -o prefix
 *       low-complexity reads (homopolymers, short tandem repeats, runs of N, which the stream shows as poly-G) dropped, or with
 *       --trim-low cut back to their longest clean stretch (sdt_gpu_complexity_kept_reads; the rule: include/sdt_gpu.h).  Mates are
 *       judged independently; pairs and routing as for clip (cxsplit.c)
 *       prefix.readComplexity: one line per read in stream order:  windows low score start len verdict
 *       prefix.cx.pairs.fa / prefix.cx.single.fa: the kept bases of the surviving reads, as clip writes them
 *       prefix.scoreHist: per score that occurs, ascending:  score reads,  then  # reads R low V dropped D clipped C
 *   sdt-kmers qtrim -s lib.cfg -K k [-p threads] [--phred 33|64, default 33] [--cut-q Q, default 20] [--low-q Q, default 15]
 *                   [--max-low-bases PCT, default 40] [--max-ee PPM, default 0 = off] [--min-len L, default 0] -o prefix
 *       reads cut to their best segment by their base qualities (Mott's rule) and dropped by low bases and expected errors
 *       (sdt_gpu_quality_reads on every batch as it is parsed; the rule: include/sdt_gpu.h).  FASTQ libraries only.  Mates are
 *       judged independently; pairs and routing as for clip (qualsplit.c)
 *       prefix.readQual: one line per read in stream order:  span low ee_ppm start len verdict
 *       prefix.qtrim.pairs.fa / prefix.qtrim.single.fa: the kept bases of the surviving reads, as clip writes them
 *       prefix.lenHist: per kept length that occurs, ascending:  len reads,  then
 *           # reads R whole W clipped C dropped D short S low V errors X bases_in I bases_out O
 *   sdt-kmers screen -s lib.cfg -K k [-p threads] -r refs.fa [-r more.fa ...] [--screen-k S, default 31] [--min-hits N, default 1]
 *                    [--min-hit-pct P, default 0] [--keep-matched] -o prefix
 *       reads that share k-mers of S bases with reference sequences (rRNA, PhiX, a mitochondrial genome, vectors) dropped, or with
 *       --keep-matched kept alone (sdt_gpu_screen_load, sdt_gpu_screen_kept_reads; the rule: include/sdt_gpu.h).  The reference files
 *       are FASTA, read and checked before the device is touched; a letter other than ACGT cuts a reference, references listed first
 *       win a shared k-mer.  The two mates of a pair are decided together; pairs as for normalize, routing as for clip (screensplit.c)
 *       prefix.readScreen: one line per read in stream order:  kmers hits ref verdict   (ref 1-based in the order of the files, 0 none)
 *       prefix.screen.pairs.fa / prefix.screen.single.fa: the surviving reads, as clip writes them
 *       prefix.screenStats: per reference  index name bases reads hits,  then  # reads R matched M kept K dropped D
 *
 * The query file is read and checked before the device is touched. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <getopt.h>
#include "../sdt_knobs.h"
#include "libcfg.h"
#include "seqio.h"
#include "readstream.h"
#include "normsplit.h"
#include "trimsplit.h"
#include "dupsplit.h"
#include "clipsplit.h"
#include "overlapsplit.h"
#include "cxsplit.h"
#include "qualsplit.h"
#include "screensplit.h"
#include "../../../include/sdt_gpu.h"

#define SDT_MAX_K 127

static void usage(void)
{
	fprintf(stderr,
	        "usage: sdt-kmers profile -s lib.cfg -K k [-p threads] [-d d] [-c min_count] -o prefix\n"
	        "           -> prefix.readCov, one line per read in stream order: kmers found solid min median max\n"
	        "       sdt-kmers query   -s lib.cfg -K k [-p threads] [-d d] -q kmers.txt [-o out.tsv]\n"
	        "           -> per line of kmers.txt: kmer found strand count l_A l_C l_T l_G r_A r_C r_T r_G linear deleted\n"
	        "       sdt-kmers correct -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] -o prefix\n"
	        "           -> prefix.readFix (per read: kmers weak runs fixed), prefix.edits (per substitution: read pos from to),\n"
	        "              prefix.corrected.fa (every read, substitution errors corrected against the counted k-mers)\n"
	        "       sdt-kmers normalize -s lib.cfg -K k [-p threads] [-d d] [--target C, default 50]\n"
	        "                           [--max-cv PCT, default 10000, 0 = off] [--seed S, default 0] -o prefix\n"
	        "           a read, or the two mates of a pair, is kept with probability C / its median k-mer coverage; reads without a\n"
	        "           k-mer, or whose counts have stdev / mean above PCT percent, are dropped; the same seed keeps the same reads\n"
	        "           -> prefix.readPick (per read in stream order: kmers median cov verdict), prefix.norm.pairs.fa (the kept pairs,\n"
	        "              read 1 then read 2), prefix.norm.single.fa (the kept single reads)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files.  Library boundaries are not preserved: the kept pairs of all\n"
	        "           paired libraries go into the one pairs file.  The reads of an interleaved p= file are decided one by one, as\n"
	        "           single reads, and go into the singles file: so do the reads of prefix.norm.pairs.fa given as p= to a second\n"
	        "           normalize run.\n"
	        "       sdt-kmers trim -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--min-cov Z, default 0]\n"
	        "                      [--min-len L, default 0] [--correct] -o prefix\n"
	        "           every read is cut back to its longest stretch of k-mers counted min_count times or more (the first among equals);\n"
	        "           a read without such a stretch, or whose longest covers fewer than L bases, is dropped; a read whose median k-mer\n"
	        "           coverage is below Z stays whole; --correct first corrects substitution errors as `correct` does\n"
	        "           -> prefix.readTrim (per read in stream order: kmers weak median start len verdict; 0 whole, 1 gated, 2 trimmed,\n"
	        "              3 dropped, 4 short), prefix.trim.pairs.fa (read 1 then read 2 of the pairs of which both mates survive),\n"
	        "              prefix.trim.single.fa (every other surviving read, the mate of a dropped read among them), with --correct\n"
	        "              prefix.edits (per substitution: read pos from to)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files, mates are trimmed independently; library boundaries go and\n"
	        "           the reads of a p= file are single reads, as for normalize.\n"
	        "       sdt-kmers dedup -s lib.cfg -K k [-p threads] [--mate-swap] -o prefix\n"
	        "           exact copies of a read, or of the two mates of a pair, are dropped: the first in stream order is kept;\n"
	        "           --mate-swap: pairs (a, b) and (b, a) are copies of each other (an unstranded library)\n"
	        "           -> prefix.readDup (per read in stream order: first copies verdict; first = the ordinal of the first read of the\n"
	        "              kept unit, copies = units in the class, verdict 0 kept, 1 dropped), prefix.dedup.pairs.fa (the kept pairs,\n"
	        "              read 1 then read 2), prefix.dedup.single.fa (the kept single reads), prefix.dupLevels (per class size present,\n"
	        "              ascending: copies classes reads)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files; the reads of a p= file are single reads, as for normalize.\n"
	        "       sdt-kmers clip -s lib.cfg -K k [-p threads] [-a adapters3.fa] [-g adapters5.fa] [--tail3 LETTERS] [--tail5 LETTERS]\n"
	        "                      [--min-overlap N, default 5] [--error-pct P, default 10] [--min-tail N, default 10]\n"
	        "                      [--tail-error-pct P, default 20] [--min-len L, default 0] -o prefix\n"
	        "           sequencing adapters (FASTA files, letters ACGT: -a at the 3' end, -g at the 5' end; an overlap of N bases or more\n"
	        "           with at most P percent mismatches, no indels) and tails of the given letters (--tail3 A, --tail5 T: poly-A and\n"
	        "           poly-T; N bases or more, at most P percent other letters) are clipped from every read; a read of which fewer than\n"
	        "           max(L, 1) bases are left is dropped.  Needs no counted k-mers: run it before every other subcommand.\n"
	        "           -> prefix.readClip (per read in stream order: adapter3 adapter5 tail3 tail5 start len verdict; adapters 1-based in\n"
	        "              the order -a then -g, 0 none; verdict 0 whole, 2 clipped, 3 dropped), prefix.clip.pairs.fa (read 1 then read 2 of\n"
	        "              the pairs of which both mates survive), prefix.clip.single.fa (every other surviving read), prefix.clipStats\n"
	        "              (per adapter: index name end reads bases; tail3 and tail5: reads bases; whole, clipped, dropped: reads)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files, mates are clipped independently, as for trim.\n"
	        "       sdt-kmers overlap -s lib.cfg -K k [-p threads] [--min-overlap N, default 30] [--max-err PCT, default 10]\n"
	        "                         [--min-len L, default 0] -o prefix\n"
	        "           mate 2 of every pair, reverse-complemented, is laid on mate 1 at every shift; the best shift with N columns or more\n"
	        "           and at most PCT percent mismatches (no indels) is the pair's overlap and gives the fragment length (insert); what a\n"
	        "           mate holds past the fragment's end is adapter and is clipped, whatever the adapter was; a read of which fewer than\n"
	        "           max(L, 1) bases are left is dropped.  Needs no adapter list and no counted k-mers: run it in front of clip.\n"
	        "           -> prefix.readOverlap (per read in stream order: overlap mismatches insert start len verdict; verdict 0 whole,\n"
	        "              2 clipped, 3 dropped), prefix.overlap.pairs.fa (read 1 then read 2 of the pairs of which both mates survive),\n"
	        "              prefix.overlap.single.fa (every other surviving read), prefix.insertHist (per insert that occurs, ascending:\n"
	        "              insert pairs; then: # pairs P overlapping V clipped C median M, the lower median of the inserts)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files; the reads of a p= file are single reads, as for normalize.\n"
	        "       sdt-kmers complexity -s lib.cfg -K k [-p threads] [--max-score P, default 10] [--max-low Q, default 50] [--trim-low]\n"
	        "                            [--min-len L, default 0] -o prefix\n"
	        "           every read is scored in windows of 64 bases that start every 32: the score is the percentage of the pairs of the\n"
	        "           window's triplets that are equal (a homopolymer 100, (AC)n 49, random sequence 1 to 2); a window of score P or more\n"
	        "           is low, and so is every base of it.  A read of which more than Q percent of the bases are low is dropped.  Q = 50\n"
	        "           is a choice, not a measurement: a 150-base read with one internal run of 30 bases has 96 low bases and is dropped.\n"
	        "           --trim-low (needs --max-low 0 or none): the longest stretch without a low base is kept instead, the first among\n"
	        "           equals; a low window loses all 64 of its bases.  A read of which fewer than max(L, 1) bases are left is dropped.\n"
	        "           Runs of N are poly-G in the 2-bit stream and are caught as such.  Needs no counted k-mers: run it after clip.\n"
	        "           -> prefix.readComplexity (per read in stream order: windows low score start len verdict; low = the windows that are\n"
	        "              low, score = the highest window score; verdict 0 whole, 2 clipped, 3 dropped), prefix.cx.pairs.fa (read 1 then\n"
	        "              read 2 of the pairs of which both mates survive), prefix.cx.single.fa (every other surviving read),\n"
	        "              prefix.scoreHist (per score that occurs, ascending: score reads; then: # reads R low V dropped D clipped C,\n"
	        "              V = the reads that have a low window)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files, mates are judged independently, as for clip.\n"
	        "       sdt-kmers qtrim -s lib.cfg -K k [-p threads] [--phred 33|64, default 33] [--cut-q Q, default 20] [--low-q Q, default 15]\n"
	        "                       [--max-low-bases PCT, default 40] [--max-ee PPM, default 0] [--min-len L, default 0] -o prefix\n"
	        "           every read is cut to the segment [a, b) with the greatest sum of (quality - Q) over its bases (Mott's rule, as\n"
	        "           seqtk trimfq; the first among equal sums, and the longest of those; --cut-q 0 keeps every read whole).  Then a read\n"
	        "           is dropped if fewer than max(L, 1) bases are left, if more than PCT percent of them have a quality below --low-q\n"
	        "           (PCT 100 or --low-q 0: off), or if --max-ee is not 0 and the expected errors per million bases of the segment\n"
	        "           (10^6 * 10^(-q / 10) per base, rounded; floor of their mean) exceed it.  The defaults are the usual figures of\n"
	        "           fastp and cutadapt: a choice, not a measurement.  The bases are not looked at: a run of N has quality 2 and is cut\n"
	        "           at the ends of a read and counted as low bases inside it.  Run it first: no other stage has the qualities.\n"
	        "           FASTQ libraries only (q1= / q2= / q=): a library with an f=, f1=, f2=, p= or b= file is refused, and so is a record\n"
	        "           whose quality line is not as long as its sequence line, before a data file is written.\n"
	        "           -> prefix.readQual (per read in stream order: span low ee_ppm start len verdict; span = the bases of the segment,\n"
	        "              low = those of them below --low-q, ee_ppm = its expected errors per million bases; verdict 0 whole, 2 clipped,\n"
	        "              3 dropped), prefix.qtrim.pairs.fa (read 1 then read 2 of the pairs of which both mates survive),\n"
	        "              prefix.qtrim.single.fa (every other surviving read), prefix.lenHist (per kept length that occurs, ascending:\n"
	        "              len reads; then: # reads R whole W clipped C dropped D short S low V errors X bases_in I bases_out O, where\n"
	        "              S, V and X are the dropped reads by the line that dropped them)\n"
	        "           Pairs are the reads of q1=/q2= files, mates are judged independently, as for clip.\n"
	        "       sdt-kmers screen -s lib.cfg -K k [-p threads] -r refs.fa [-r more.fa ...] [--screen-k S, default 31]\n"
	        "                        [--min-hits N, default 1] [--min-hit-pct P, default 0] [--keep-matched] -o prefix\n"
	        "           reads that come from sequences one already knows (ribosomal RNA, the PhiX spike-in, a mitochondrial genome, vectors)\n"
	        "           are taken out: the references (FASTA files, any length; a letter other than ACGT cuts a reference) become a set of\n"
	        "           canonical k-mers of S bases (11 to 31; -K is only the k of the counting context), and a read is matched if N or more\n"
	        "           of its k-mers, and P percent or more of them, are in the set.  A read, or the two mates of a pair, is dropped if it is\n"
	        "           matched; --keep-matched keeps the matched ones instead (bait).  A k-mer that several references hold counts for the\n"
	        "           one listed first.  S = 31 is the usual figure of bbduk: a choice, not a measurement.  An N in a read is a G.\n"
	        "           Needs no counted k-mers: run it after clip and in front of complexity and dedup.\n"
	        "           -> prefix.readScreen (per read in stream order: kmers hits ref verdict; ref = the reference of the read's hits that is\n"
	        "              listed first, 1-based, 0 none; verdict 0 kept, 1 dropped), prefix.screen.pairs.fa (read 1 then read 2 of the pairs\n"
	        "              that survive), prefix.screen.single.fa (every other surviving read), prefix.screenStats (per reference: index name\n"
	        "              bases reads hits, reads = the reads whose ref it is, hits = their hits; then: # reads R matched M kept K dropped D)\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files; the reads of a p= file are single reads, as for normalize.\n"
	        "       (--device n: HIP device ordinal; --max-k 31|63|127: the variant whose K limit applies, default by K)\n");
}

/* pooled batches (pinned buffers, seqio.h) are pushed asynchronously, as sdt-pregraph does */
#define PUSH_DEPTH 12
static struct { int slot[PUSH_DEPTH]; uint64_t ticket[PUSH_DEPTH]; int head, n; } g_inflight;

static int inflight_retire(sdt_ctx *gpu, int down_to)
{
	while (g_inflight.n > down_to) {
		if (sdt_gpu_push_wait(gpu, g_inflight.ticket[g_inflight.head]) != SDT_OK) { fprintf(stderr, "sdt_gpu_push_wait: %s\n", sdt_gpu_last_error()); return -1; }
		sdt_pool_release(g_inflight.slot[g_inflight.head]);
		g_inflight.head = (g_inflight.head + 1) % PUSH_DEPTH;
		g_inflight.n--;
	}
	return 0;
}

typedef struct { sdt_ctx *gpu; unsigned long long reads; sdt_pair_ranges *pairs; } push_state;

static int push_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	push_state *st = (push_state *)user;
	st->reads += b->nreads;
	if (!b->nreads) return 0;
	if (st->pairs && sdt_pair_ranges_note(st->pairs, ord_base, ord_stride, b->stream_parity, b->nreads) != 0) { fprintf(stderr, "sdt-kmers: out of memory\n"); return -1; }
	sdt_gpu_set_read_ordinal(st->gpu, ord_base, ord_stride);
	if (b->pool_slot >= 0) {
		uint64_t ticket = 0;
		const int rc = b->fixed_len ? sdt_gpu_push_reads_fixed_async(st->gpu, b->words, b->nwords, b->nreads, b->fixed_len, &ticket)
		                            : sdt_gpu_push_reads_async(st->gpu, b->words, b->nwords, b->offsets, b->nreads, &ticket);
		if (rc != SDT_OK) { fprintf(stderr, "sdt_gpu_push_reads_async: %s\n", sdt_gpu_last_error()); return -1; }
		if (inflight_retire(st->gpu, PUSH_DEPTH - 1) != 0) return -1;
		const int at = (g_inflight.head + g_inflight.n) % PUSH_DEPTH;
		g_inflight.slot[at] = b->pool_slot;
		g_inflight.ticket[at] = ticket;
		g_inflight.n++;
		sdt_pool_take(b->pool_slot);
		return 0;
	}
	if (sdt_gpu_push_reads(st->gpu, b->words, b->nwords, b->offsets, b->nreads) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_push_reads: %s\n", sdt_gpu_last_error());
		return -1;
	}
	return 0;
}

static char *put_u32(char *p, uint32_t v, char sep)
{
	char t[10];
	int n = 0;
	do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (n) *p++ = t[--n];
	*p++ = sep;
	return p;
}

/* prefix.readCov: "kmers found solid min median max" per read (8 M reads are 180 MB of digits: formatted by hand into a block buffer) */
static int write_read_cov(const char *path, const sdt_read_cov *cov, unsigned long long n)
{
	FILE *fo = fopen(path, "w");
	if (!fo) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path); return -1; }
	enum { BLOCK = 1 << 20, LINE_MAX_BYTES = 6 * 11 };
	char *buf = (char *)malloc(BLOCK), *p = buf;
	int ok = buf != NULL;
	for (unsigned long long i = 0; ok && i < n; i++) {
		p = put_u32(p, cov[i].kmers, ' ');
		p = put_u32(p, cov[i].found, ' ');
		p = put_u32(p, cov[i].solid, ' ');
		p = put_u32(p, cov[i].min, ' ');
		p = put_u32(p, cov[i].median, ' ');
		p = put_u32(p, cov[i].max, '\n');
		if (p - buf > BLOCK - LINE_MAX_BYTES) { ok = fwrite(buf, 1, (size_t)(p - buf), fo) == (size_t)(p - buf); p = buf; }
	}
	if (ok && p != buf) ok = fwrite(buf, 1, (size_t)(p - buf), fo) == (size_t)(p - buf);
	free(buf);
	if (fclose(fo) != 0) ok = 0;
	if (!ok) fprintf(stderr, "sdt-kmers: write to %s failed\n", path);
	return ok ? 0 : -1;
}

/* text formatted by hand into a block buffer, as write_read_cov does */
typedef struct { FILE *f; char *buf, *p; int ok; const char *path; } outbuf;
enum { OB_BLOCK = 1 << 20 };

static int ob_open(outbuf *o, const char *path)
{
	o->path = path;
	o->f = fopen(path, "w");
	if (!o->f) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path); return -1; }
	o->buf = o->p = (char *)malloc(OB_BLOCK);
	o->ok = 1;
	if (!o->buf) { fprintf(stderr, "sdt-kmers: out of memory\n"); fclose(o->f); o->f = NULL; return -1; }
	return 0;
}

/* room for `need` more bytes (need <= OB_BLOCK); after a failed write the block is dropped, never overrun: the caller stops on !ok */
static void ob_room(outbuf *o, size_t need)
{
	if ((size_t)(o->p - o->buf) + need > OB_BLOCK) {
		if (o->ok) o->ok = fwrite(o->buf, 1, (size_t)(o->p - o->buf), o->f) == (size_t)(o->p - o->buf);
		o->p = o->buf;
	}
}

static int ob_close(outbuf *o)
{
	if (o->ok && o->p != o->buf) o->ok = fwrite(o->buf, 1, (size_t)(o->p - o->buf), o->f) == (size_t)(o->p - o->buf);
	free(o->buf);
	if (fclose(o->f) != 0) o->ok = 0;
	if (!o->ok) fprintf(stderr, "sdt-kmers: write to %s failed\n", o->path);
	return o->ok ? 0 : -1;
}

static char *put_u64(char *p, uint64_t v, char sep)
{
	char t[20];
	int n = 0;
	do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (n) *p++ = t[--n];
	*p++ = sep;
	return p;
}

/* the kept batches back from HBM, and where every ordinal's read is */
typedef struct {
	uint64_t nb, longest;
	uint32_t **bw;                                                           /* words of batch b */
	uint64_t **bo;                                                           /* offsets of batch b */
	uint32_t *at_batch, *at_read;                                            /* by ordinal; at_batch 0xFFFFFFFF: no kept read has it */
} kept_reads;

static int kept_fetch(sdt_ctx *gpu, unsigned long long reads, kept_reads *k)
{
	const uint64_t m = reads ? reads : 1;
	memset(k, 0, sizeof *k);
	if (sdt_gpu_kept_batches(gpu, &k->nb) != SDT_OK) { fprintf(stderr, "sdt_gpu_kept_batches: %s\n", sdt_gpu_last_error()); return 1; }
	k->bw = (uint32_t **)calloc(k->nb ? k->nb : 1, sizeof(uint32_t *));
	k->bo = (uint64_t **)calloc(k->nb ? k->nb : 1, sizeof(uint64_t *));
	k->at_batch = (uint32_t *)malloc(m * sizeof(uint32_t));
	k->at_read = (uint32_t *)malloc(m * sizeof(uint32_t));
	if (!k->bw || !k->bo || !k->at_batch || !k->at_read) { fprintf(stderr, "sdt-kmers: out of memory\n"); return 1; }
	memset(k->at_batch, 0xFF, m * sizeof(uint32_t));
	for (uint64_t b = 0; b < k->nb; b++) {
		uint64_t info[4];
		if (sdt_gpu_fetch_kept_batch(gpu, b, info, NULL, 0, NULL, 0) != SDT_OK) { fprintf(stderr, "sdt_gpu_fetch_kept_batch: %s\n", sdt_gpu_last_error()); return 1; }
		k->bw[b] = (uint32_t *)malloc((info[0] ? info[0] : 1) * sizeof(uint32_t));
		k->bo[b] = (uint64_t *)malloc((info[1] + 1) * sizeof(uint64_t));
		if (!k->bw[b] || !k->bo[b]) { fprintf(stderr, "sdt-kmers: out of memory for the reads\n"); return 1; }
		if (sdt_gpu_fetch_kept_batch(gpu, b, info, k->bw[b], info[0], k->bo[b], info[1] + 1) != SDT_OK) { fprintf(stderr, "sdt_gpu_fetch_kept_batch: %s\n", sdt_gpu_last_error()); return 1; }
		for (uint64_t i = 0; i < info[1]; i++) {
			const uint64_t ord = info[2] + i * info[3];
			if (ord >= reads) { fprintf(stderr, "sdt-kmers: a kept read has ordinal %llu of %llu\n", (unsigned long long)ord, reads); return 1; }
			k->at_batch[ord] = (uint32_t)b;
			k->at_read[ord] = (uint32_t)i;
			if (k->bo[b][i + 1] - k->bo[b][i] > k->longest) k->longest = k->bo[b][i + 1] - k->bo[b][i];
		}
	}
	if (k->longest + 64 > OB_BLOCK) { fprintf(stderr, "sdt-kmers: a read of %llu bases\n", (unsigned long long)k->longest); return 1; }
	return 0;
}

static void kept_free(kept_reads *k)
{
	for (uint64_t b = 0; b < k->nb; b++) { free(k->bw[b]); free(k->bo[b]); }
	free(k->bw); free(k->bo); free(k->at_batch); free(k->at_read);
}

/* sdt_gpu_correct_kept_reads: fix[] by ordinal and the edits, ascending, in a list of the size they need */
static int correct_kept(sdt_ctx *gpu, unsigned long long reads, uint32_t min_count, sdt_read_fix *fix, uint64_t **edits_out, uint64_t *n_edits_out)
{
	/* (room for one edit per read at first: too little means the whole correction runs again just to hand over the edits) */
	uint64_t cap = reads + 1024, n_edits = 0, got = 0;
	uint64_t *edits = (uint64_t *)malloc(cap * sizeof(uint64_t));
	if (!edits) { fprintf(stderr, "sdt-kmers: out of memory for %llu edits\n", (unsigned long long)cap); return 1; }
	int rc = sdt_gpu_correct_kept_reads(gpu, min_count, fix, reads, &got, edits, cap, &n_edits);
	if (rc == SDT_EFULL && n_edits > cap) {                                  /* more edits than guessed: once more with room for all */
		cap = n_edits;
		free(edits);
		edits = (uint64_t *)malloc(cap * sizeof(uint64_t));
		if (!edits) { fprintf(stderr, "sdt-kmers: out of memory for %llu edits\n", (unsigned long long)cap); return 1; }
		rc = sdt_gpu_correct_kept_reads(gpu, min_count, fix, reads, &got, edits, cap, &n_edits);
	}
	if (rc != SDT_OK) { fprintf(stderr, "sdt_gpu_correct_kept_reads: %s\n", sdt_gpu_last_error()); return 1; }
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu corrected\n", reads, (unsigned long long)got); return 1; }
	*edits_out = edits;
	*n_edits_out = n_edits;
	return 0;
}

/* one edit of read `ord` (its bases from `start` of w, len of them) applied to the words and written as "read pos from to"; -1: the
 * edit names a base the read does not have */
static int apply_edit(outbuf *oe, uint64_t edit, uint64_t ord, uint32_t *w, uint64_t start, uint64_t len)
{
	static const char letters[4] = {'A', 'C', 'T', 'G'};
	const uint64_t pos = (edit >> 2) & 0xFFFFu, g = start + pos;
	if (pos >= len) { fprintf(stderr, "sdt-kmers: an edit at base %llu of a read of %llu\n", (unsigned long long)pos, (unsigned long long)len); return -1; }
	const int sh = 30 - 2 * (int)(g & 15);
	const uint32_t old = (w[g >> 4] >> sh) & 3u, neu = (uint32_t)(edit & 3u);
	w[g >> 4] ^= (old ^ neu) << sh;
	ob_room(oe, 2 * 21 + 4);
	oe->p = put_u64(oe->p, ord + 1, ' ');
	oe->p = put_u64(oe->p, pos + 1, ' ');
	*oe->p++ = letters[old];
	*oe->p++ = ' ';
	*oe->p++ = letters[neu];
	*oe->p++ = '\n';
	return 0;
}

/* `correct`: the records and the edits from the device, the kept batches back from HBM, the edits applied here */
static int correct_and_write(sdt_ctx *gpu, unsigned long long reads, uint32_t min_count, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_fix *fix = (sdt_read_fix *)calloc(m, sizeof(sdt_read_fix));
	uint64_t *edits = NULL, n_edits = 0;
	if (!fix) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	if (correct_kept(gpu, reads, min_count, fix, &edits, &n_edits) != 0) return 1;
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[3][4200];
	snprintf(path[0], sizeof path[0], "%s.readFix", prefix);
	snprintf(path[1], sizeof path[1], "%s.edits", prefix);
	snprintf(path[2], sizeof path[2], "%s.corrected.fa", prefix);
	outbuf of, oe, oa;
	if (ob_open(&of, path[0]) != 0) return 1;
	if (ob_open(&oe, path[1]) != 0) { ob_close(&of); return 1; }
	if (ob_open(&oa, path[2]) != 0) { ob_close(&of); ob_close(&oe); return 1; }
	unsigned long long with_weak = 0, runs = 0, fixed = 0;
	uint64_t e = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads && !bad; ord++) {
		if (!of.ok || !oe.ok || !oa.ok) break;                               /* a write failed: ob_close says which */
		ob_room(&of, 4 * 11);
		of.p = put_u32(of.p, fix[ord].kmers, ' ');
		of.p = put_u32(of.p, fix[ord].weak, ' ');
		of.p = put_u32(of.p, fix[ord].runs, ' ');
		of.p = put_u32(of.p, fix[ord].fixed, '\n');
		with_weak += fix[ord].weak != 0;
		runs += fix[ord].runs;
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		uint32_t *w = k.bw[k.at_batch[ord]];
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		for (; e < n_edits && (edits[e] >> 18) == ord && !bad; e++, fixed++)
			bad = apply_edit(&oe, edits[e], ord, w, start, len) != 0;
		ob_room(&oa, (size_t)len + 24);
		oa.p = sdt_put_fasta_record(oa.p, ord, w, start, len);
	}
	const int all_written = of.ok && oe.ok && oa.ok;
	if ((ob_close(&of) != 0) | (ob_close(&oe) != 0) | (ob_close(&oa) != 0) || bad) return 1;
	if (all_written && e != n_edits) { fprintf(stderr, "sdt-kmers: %llu of %llu edits name no read of the stream\n", (unsigned long long)(n_edits - e), (unsigned long long)n_edits); return 1; }
	kept_free(&k);
	free(fix); free(edits);
	printf("%llu reads, %llu with weak k-mers, %llu runs, %llu bases corrected into %s\n", reads, with_weak, runs, fixed, path[2]);
	return 0;
}

/* `normalize`: the verdicts from the device, the kept batches back from HBM, the kept reads into the pairs file or the singles file */
static int normalize_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_norm_params *prm, const sdt_pair_ranges *pairs, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_pick *pick = (sdt_read_pick *)malloc(m * sizeof(sdt_read_pick));
	if (!pick) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	memset(pick, 0xFF, m * sizeof(sdt_read_pick));                           /* (an ordinal that no read has keeps verdict 0xFFFFFFFF) */
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_select_kept_reads(gpu, prm, pairs->v, pairs->n, pick, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_select_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu decided\n", reads, (unsigned long long)got); return 1; }
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[3][4200];
	snprintf(path[0], sizeof path[0], "%s.readPick", prefix);
	snprintf(path[1], sizeof path[1], "%s.norm.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.norm.single.fa", prefix);
	outbuf opick, opair, osingle;
	if (ob_open(&opick, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&opick); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&opick); ob_close(&opair); return 1; }
	unsigned long long kept = 0, n_short = 0, aberrant = 0, drawn = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!opick.ok || !opair.ok || !osingle.ok) break;                               /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		ob_room(&opick, 4 * 11);
		opick.p = put_u32(opick.p, pick[ord].kmers, ' ');
		opick.p = put_u32(opick.p, pick[ord].median, ' ');
		opick.p = put_u32(opick.p, pick[ord].cov, ' ');
		opick.p = put_u32(opick.p, pick[ord].verdict, '\n');
		const uint32_t cls = pick[ord].verdict & 7u;
		n_short += cls == 4;
		aberrant += cls == 3;
		drawn += cls == 2;
		if (cls > 1) continue;
		kept++;
		outbuf *o = sdt_pair_ranges_holds(pairs, ord, &cursor) ? &opair : &osingle;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		ob_room(o, (size_t)len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start, len);
	}
	if ((ob_close(&opick) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	kept_free(&k);
	free(pick);
	printf("%llu of %llu reads kept (%llu short, %llu aberrant, %llu dropped by draw)\n", kept, reads, n_short, aberrant, drawn);
	return 0;
}

/* `dedup`: the records from the device, the kept batches back from HBM, the kept reads into the pairs file or the singles file, the
 * table of duplication levels (dupsplit.c) */
static int dedup_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_dedup_params *prm, const sdt_pair_ranges *pairs, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_dup *dup = (sdt_read_dup *)malloc(m * sizeof(sdt_read_dup));
	if (!dup) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	memset(dup, 0xFF, m * sizeof(sdt_read_dup));                             /* (an ordinal that no read has keeps verdict 0xFFFFFFFF) */
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_dedup_kept_reads(gpu, prm, pairs->v, pairs->n, dup, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_dedup_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu decided\n", reads, (unsigned long long)got); return 1; }
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readDup", prefix);
	snprintf(path[1], sizeof path[1], "%s.dedup.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.dedup.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.dupLevels", prefix);
	outbuf odup, opair, osingle, olev;
	if (ob_open(&odup, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&odup); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&odup); ob_close(&opair); return 1; }
	if (ob_open(&olev, path[3]) != 0) { ob_close(&odup); ob_close(&opair); ob_close(&osingle); return 1; }
	sdt_dup_levels lv;
	memset(&lv, 0, sizeof lv);
	unsigned long long kept = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!odup.ok || !opair.ok || !osingle.ok) break;                                /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_dup *r = dup + ord;
		if (r->verdict > 1 || r->copies == 0 || r->first > ord) {
			fprintf(stderr, "sdt-kmers: the record of read %llu is %llu %u %u\n", (unsigned long long)ord + 1, (unsigned long long)r->first, r->copies, r->verdict);
			bad = 1;
			break;
		}
		ob_room(&odup, SDT_DUP_LINE_MAX);
		odup.p = sdt_put_dup_line(odup.p, r);
		/* (every ordinal has a read here, so the first read of a kept unit is the one whose ordinal is the unit's id) */
		if (sdt_dup_levels_note(&lv, r, r->verdict == 0 && r->first == ord) != 0) { fprintf(stderr, "sdt-kmers: out of memory\n"); bad = 1; break; }
		if (r->verdict != 0) continue;
		kept++;
		outbuf *o = sdt_pair_ranges_holds(pairs, ord, &cursor) ? &opair : &osingle;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		ob_room(o, (size_t)len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start, len);
	}
	unsigned long long classes = 0;
	for (size_t i = 0; i < lv.n && !bad; i++) {
		ob_room(&olev, SDT_DUP_LEVEL_LINE_MAX);
		olev.p = sdt_put_dup_level_line(olev.p, lv.v + i);
		classes += lv.v[i].classes;
	}
	sdt_dup_levels_free(&lv);
	const int all_written = odup.ok && opair.ok && osingle.ok && olev.ok;
	if ((ob_close(&odup) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) | (ob_close(&olev) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	kept_free(&k);
	free(dup);
	printf("%llu of %llu reads kept in %llu classes\n", kept, reads, classes);
	return 0;
}

/* `trim`: the records (and with --correct the edits) from the device, the kept batches back from HBM, the edits applied here, the kept
 * bases of every read into the pairs file (both mates survive) or the singles file (trimsplit.c) */
static int trim_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_trim_params *prm, const sdt_pair_ranges *pairs, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	const int correct = (prm->flags & SDT_TRIM_CORRECTED) != 0;
	sdt_read_trim *trim = (sdt_read_trim *)calloc(m, sizeof(sdt_read_trim));
	sdt_read_fix *fix = correct ? (sdt_read_fix *)calloc(m, sizeof(sdt_read_fix)) : NULL;
	if (!trim || (correct && !fix)) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	uint64_t got = 0, n_kept = 0, *edits = NULL, n_edits = 0;
	if (sdt_gpu_trim_kept_reads(gpu, prm, trim, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_trim_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu trimmed\n", reads, (unsigned long long)got); return 1; }
	if (correct && correct_kept(gpu, reads, prm->min_count, fix, &edits, &n_edits) != 0) return 1;
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readTrim", prefix);
	snprintf(path[1], sizeof path[1], "%s.trim.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.trim.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.edits", prefix);
	outbuf otrim, opair, osingle, oe;
	if (ob_open(&otrim, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&otrim); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&otrim); ob_close(&opair); return 1; }
	if (correct && ob_open(&oe, path[3]) != 0) { ob_close(&otrim); ob_close(&opair); ob_close(&osingle); return 1; }
	unsigned long long by_verdict[5] = {0, 0, 0, 0, 0}, kept = 0, bases_in = 0, bases_out = 0;
	size_t cursor = 0;
	uint64_t e = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads && !bad; ord++) {
		if (!otrim.ok || !opair.ok || !osingle.ok || (correct && !oe.ok)) break;    /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_trim *t = trim + ord;
		ob_room(&otrim, SDT_TRIM_LINE_MAX);
		otrim.p = sdt_put_trim_line(otrim.p, t);
		uint32_t *w = k.bw[k.at_batch[ord]];
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		if (t->verdict > 4 || (uint64_t)t->start + t->len > len) {
			fprintf(stderr, "sdt-kmers: the record of read %llu keeps [%u, %u + %u) of %llu bases, verdict %u\n", (unsigned long long)ord + 1, t->start,
			        t->start, t->len, (unsigned long long)len, t->verdict);
			bad = 1;
			break;
		}
		by_verdict[t->verdict]++;
		bases_in += len;
		for (; e < n_edits && (edits[e] >> 18) == ord && !bad; e++)
			bad = apply_edit(&oe, edits[e], ord, w, start, len) != 0;
		const int to = sdt_trim_route(pairs, &cursor, trim, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		bases_out += t->len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, w, start + t->start, t->len);
	}
	const int all_written = otrim.ok && opair.ok && osingle.ok && (!correct || oe.ok);
	if ((ob_close(&otrim) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) | (correct && ob_close(&oe) != 0) || bad) return 1;
	if (all_written && e != n_edits) { fprintf(stderr, "sdt-kmers: %llu of %llu edits name no read of the stream\n", (unsigned long long)(n_edits - e), (unsigned long long)n_edits); return 1; }
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	kept_free(&k);
	free(trim); free(fix); free(edits);
	printf("%llu reads: %llu whole, %llu gated, %llu trimmed, %llu dropped, %llu short; %llu bases in, %llu bases out\n", reads, by_verdict[0],
	       by_verdict[1], by_verdict[2], by_verdict[3], by_verdict[4], bases_in, bases_out);
	return 0;
}

/* `clip`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both mates
 * survive) or the singles file, routed as trim routes them; the statistics (clipsplit.c) */
static int clip_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_clip_params *prm, const sdt_adapter_list *ads, const sdt_pair_ranges *pairs,
                          const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_clip *clip = (sdt_read_clip *)calloc(m, sizeof(sdt_read_clip));
	sdt_clip_stats stats;
	if (!clip || sdt_clip_stats_init(&stats, ads->n) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	const sdt_adapter_set set = sdt_adapters_set(ads);
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_clip_kept_reads(gpu, prm, &set, clip, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_clip_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu clipped\n", reads, (unsigned long long)got); return 1; }
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readClip", prefix);
	snprintf(path[1], sizeof path[1], "%s.clip.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.clip.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.clipStats", prefix);
	outbuf oclip, opair, osingle;
	if (ob_open(&oclip, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&oclip); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&oclip); ob_close(&opair); return 1; }
	unsigned long long kept = 0, bases_in = 0, bases_out = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!oclip.ok || !opair.ok || !osingle.ok) break;                              /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_clip *t = clip + ord;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		if (sdt_clip_stats_note(&stats, t, len) != 0) {
			fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->adapters, t->tail3,
			        t->tail5, t->start, t->len, t->verdict, (unsigned long long)len);
			bad = 1;
			break;
		}
		ob_room(&oclip, SDT_CLIP_LINE_MAX);
		oclip.p = sdt_put_clip_line(oclip.p, t);
		bases_in += len;
		/* (start and len sit where sdt_read_trim has them: clipsplit.h) */
		const int to = sdt_trim_route(pairs, &cursor, (const sdt_read_trim *)clip, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		bases_out += t->len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start + t->start, t->len);
	}
	const int all_written = oclip.ok && opair.ok && osingle.ok;
	if ((ob_close(&oclip) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	FILE *fs = fopen(path[3], "w");
	if (!fs || (sdt_clip_stats_write(fs, &stats, ads) != 0) | (fclose(fs) != 0)) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path[3]); return 1; }
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped; %llu bases in, %llu bases out\n", reads, (unsigned long long)stats.whole,
	       (unsigned long long)stats.clipped, (unsigned long long)stats.dropped, bases_in, bases_out);
	kept_free(&k);
	sdt_clip_stats_free(&stats);
	free(clip);
	return 0;
}

/* `overlap`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both mates
 * survive) or the singles file, routed as trim routes them; the histogram of the inserts (overlapsplit.c) */
static int overlap_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_overlap_params *prm, const sdt_pair_ranges *pairs, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_overlap *ov = (sdt_read_overlap *)calloc(m, sizeof(sdt_read_overlap));
	if (!ov) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_overlap_kept_pairs(gpu, prm, pairs->v, pairs->n, ov, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_overlap_kept_pairs: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu decided\n", reads, (unsigned long long)got); return 1; }
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readOverlap", prefix);
	snprintf(path[1], sizeof path[1], "%s.overlap.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.overlap.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.insertHist", prefix);
	outbuf oov, opair, osingle;
	if (ob_open(&oov, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&oov); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&oov); ob_close(&opair); return 1; }
	sdt_insert_hist hist;
	memset(&hist, 0, sizeof hist);
	unsigned long long kept = 0, by_verdict[4] = {0, 0, 0, 0}, bases_in = 0, bases_out = 0;
	size_t cursor = 0, pcursor = 0;
	uint64_t len_first = 0;                                                  /* the first mate's bases, while the second is awaited */
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!oov.ok || !opair.ok || !osingle.ok) break;                              /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_overlap *t = ov + ord;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		int ok = sdt_overlap_record_ok(t, len);
		if (ok && sdt_pair_ranges_holds(pairs, ord, &pcursor)) {
			if (((ord - pairs->v[2 * pcursor]) & 1) == 0) len_first = len;
			else {
				const int rc = sdt_insert_hist_note(&hist, t - 1, t, len_first, len);
				if (rc == -1) { fprintf(stderr, "sdt-kmers: out of memory\n"); bad = 1; break; }
				ok = rc == 0;
			}
		}
		if (!ok) {
			fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->overlap, t->mismatches,
			        t->insert, t->start, t->len, t->verdict, (unsigned long long)len);
			bad = 1;
			break;
		}
		ob_room(&oov, SDT_OVERLAP_LINE_MAX);
		oov.p = sdt_put_overlap_line(oov.p, t);
		by_verdict[t->verdict]++;
		bases_in += len;
		/* (start and len sit where sdt_read_trim has them: overlapsplit.h) */
		const int to = sdt_trim_route(pairs, &cursor, (const sdt_read_trim *)ov, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		bases_out += t->len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start + t->start, t->len);
	}
	const int all_written = oov.ok && opair.ok && osingle.ok;
	if ((ob_close(&oov) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	const unsigned long long overlapping = hist.n, median = sdt_insert_hist_median(&hist);
	FILE *fh = fopen(path[3], "w");
	if (!fh || (sdt_insert_hist_write(fh, &hist) != 0) | (fclose(fh) != 0)) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path[3]); return 1; }
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped; %llu bases in, %llu bases out; %llu pairs, %llu overlapping, median insert %llu\n", reads,
	       by_verdict[0], by_verdict[2], by_verdict[3], bases_in, bases_out, (unsigned long long)hist.pairs, overlapping, median);
	kept_free(&k);
	sdt_insert_hist_free(&hist);
	free(ov);
	return 0;
}

/* `complexity`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both
 * mates survive) or the singles file, routed as clip routes them; the histogram of the scores (cxsplit.c) */
static int complexity_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_complexity_params *prm, const sdt_pair_ranges *pairs, const char *prefix)
{
	const uint64_t m = reads ? reads : 1;
	sdt_read_complexity *cx = (sdt_read_complexity *)calloc(m, sizeof(sdt_read_complexity));
	if (!cx) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_complexity_kept_reads(gpu, prm, cx, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_complexity_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu decided\n", reads, (unsigned long long)got); return 1; }
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readComplexity", prefix);
	snprintf(path[1], sizeof path[1], "%s.cx.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.cx.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.scoreHist", prefix);
	outbuf ocx, opair, osingle;
	if (ob_open(&ocx, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&ocx); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&ocx); ob_close(&opair); return 1; }
	sdt_score_hist hist;
	memset(&hist, 0, sizeof hist);
	unsigned long long kept = 0, bases_in = 0, bases_out = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!ocx.ok || !opair.ok || !osingle.ok) break;                                /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_complexity *t = cx + ord;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		if (sdt_score_hist_note(&hist, t, len) != 0) {
			fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->windows, t->low,
			        t->score, t->start, t->len, t->verdict, (unsigned long long)len);
			bad = 1;
			break;
		}
		ob_room(&ocx, SDT_CX_LINE_MAX);
		ocx.p = sdt_put_cx_line(ocx.p, t);
		bases_in += len;
		/* (start and len sit where sdt_read_trim has them: cxsplit.h) */
		const int to = sdt_trim_route(pairs, &cursor, (const sdt_read_trim *)cx, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		bases_out += t->len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start + t->start, t->len);
	}
	const int all_written = ocx.ok && opair.ok && osingle.ok;
	if ((ob_close(&ocx) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	FILE *fh = fopen(path[3], "w");
	if (!fh || (sdt_score_hist_write(fh, &hist) != 0) | (fclose(fh) != 0)) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path[3]); return 1; }
	printf("%llu reads: %llu with a low window, %llu clipped, %llu dropped; %llu bases in, %llu bases out\n", reads, (unsigned long long)hist.low,
	       (unsigned long long)hist.clipped, (unsigned long long)hist.dropped, bases_in, bases_out);
	kept_free(&k);
	free(cx);
	return 0;
}

/* `screen`: the references into the device's set, the records from the device, the kept batches back from HBM, every surviving read
 * into the pairs file (both mates of a pair) or the singles file, routed as clip routes them; the statistics (screensplit.c) */
static int screen_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_screen_params *prm, uint32_t k, const sdt_ref_set *refs,
                            const sdt_pair_ranges *pairs, const char *prefix)
{
	uint64_t distinct = 0;
	if (sdt_gpu_screen_load(gpu, refs->words, refs->nwords, refs->offsets, refs->nseqs, refs->ref_of_seq, refs->n_refs, k, &distinct) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_screen_load: %s\n", sdt_gpu_last_error());
		return 1;
	}
	const uint64_t m = reads ? reads : 1;
	sdt_read_screen *rec = (sdt_read_screen *)calloc(m, sizeof(sdt_read_screen));
	sdt_screen_stats stats;
	if (!rec || sdt_screen_stats_init(&stats, refs->n_refs) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	uint64_t got = 0, n_kept = 0;
	if (sdt_gpu_screen_kept_reads(gpu, prm, pairs->v, pairs->n, rec, reads, &got, &n_kept) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_screen_kept_reads: %s\n", sdt_gpu_last_error());
		return 1;
	}
	if (got != reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu decided\n", reads, (unsigned long long)got); return 1; }
	kept_reads kr;
	if (kept_fetch(gpu, reads, &kr) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readScreen", prefix);
	snprintf(path[1], sizeof path[1], "%s.screen.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.screen.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.screenStats", prefix);
	outbuf orec, opair, osingle;
	if (ob_open(&orec, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&orec); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&orec); ob_close(&opair); return 1; }
	unsigned long long kept = 0, bases_in = 0, bases_out = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!orec.ok || !opair.ok || !osingle.ok) break;                               /* a write failed: ob_close says which */
		if (kr.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_screen *t = rec + ord;
		const uint64_t start = kr.bo[kr.at_batch[ord]][kr.at_read[ord]], len = kr.bo[kr.at_batch[ord]][kr.at_read[ord] + 1] - start;
		if (sdt_screen_stats_note(&stats, t, len, k, prm) != 0) {
			fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->kmers, t->hits, t->ref,
			        t->start, t->len, t->verdict, (unsigned long long)len);
			bad = 1;
			break;
		}
		ob_room(&orec, SDT_SCREEN_LINE_MAX);
		orec.p = sdt_put_screen_line(orec.p, t);
		bases_in += len;
		/* (start and len sit where sdt_read_trim has them: screensplit.h) */
		const int to = sdt_trim_route(pairs, &cursor, (const sdt_read_trim *)rec, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		bases_out += t->len;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, kr.bw[kr.at_batch[ord]], start, t->len);
	}
	const int all_written = orec.ok && opair.ok && osingle.ok;
	if ((ob_close(&orec) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	FILE *fs = fopen(path[3], "w");
	if (!fs || (sdt_screen_stats_write(fs, &stats, refs) != 0) | (fclose(fs) != 0)) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path[3]); return 1; }
	printf("%llu reads against %llu k-mers of %u references: %llu matched, %llu kept, %llu dropped; %llu bases in, %llu bases out\n", reads,
	       (unsigned long long)distinct, refs->n_refs, (unsigned long long)stats.matched, (unsigned long long)stats.kept, (unsigned long long)stats.dropped,
	       bases_in, bases_out);
	kept_free(&kr);
	sdt_screen_stats_free(&stats);
	free(rec);
	return 0;
}

/* `qtrim`, while the reads stream: every FASTQ batch's qualities through sdt_gpu_quality_reads on a context of its own (nothing of the
 * asynchronous push path is touched), the records to the batch's ordinals; then the batch is pushed like any other */
typedef struct {
	push_state push;
	sdt_ctx *qgpu;
	const sdt_quality_params *prm;
	sdt_read_quality *rec, *dense;                                           /* by ordinal; of one batch */
	uint64_t cap, dense_cap, n_kept;
} qtrim_state;

static int qtrim_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	qtrim_state *q = (qtrim_state *)user;
	if (b->qual_faults) {
		fprintf(stderr, "sdt-kmers: %llu records of the batch at read %llu have a quality line that is not as long as their sequence line\n",
		        (unsigned long long)b->qual_faults, (unsigned long long)ord_base + 1);
		return -1;
	}
	if (b->nreads) {
		if (!b->quals) { fprintf(stderr, "sdt-kmers: the batch at read %llu has no qualities\n", (unsigned long long)ord_base + 1); return -1; }
		const uint64_t need = ord_base + (b->nreads - 1) * ord_stride + 1;
		if (need > q->cap) {
			uint64_t ncap = q->cap ? q->cap : 1 << 16;
			while (ncap < need) ncap *= 2;
			sdt_read_quality *nr = (sdt_read_quality *)realloc(q->rec, ncap * sizeof(sdt_read_quality));
			if (!nr) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", (unsigned long long)ncap); return -1; }
			memset(nr + q->cap, 0, (ncap - q->cap) * sizeof(sdt_read_quality));
			q->rec = nr;
			q->cap = ncap;
		}
		if (b->nreads > q->dense_cap) {
			free(q->dense);
			q->dense = (sdt_read_quality *)malloc(b->nreads * sizeof(sdt_read_quality));
			q->dense_cap = q->dense ? b->nreads : 0;
			if (!q->dense) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", (unsigned long long)b->nreads); return -1; }
		}
		uint64_t kept = 0;
		if (sdt_gpu_quality_reads(q->qgpu, b->quals, b->offsets[b->nreads], b->offsets, b->nreads, q->prm, q->dense, NULL, &kept) != SDT_OK) {
			fprintf(stderr, "sdt_gpu_quality_reads: %s\n", sdt_gpu_last_error());
			return -1;
		}
		q->n_kept += kept;
		for (uint64_t i = 0; i < b->nreads; i++) q->rec[ord_base + i * ord_stride] = q->dense[i];
	}
	return push_batch(&q->push, b, ord_base, ord_stride);
}

/* `qtrim`, after the stream: the kept batches back from HBM, the kept bases of every read into the pairs file (both mates survive) or
 * the singles file, routed as clip routes them; the histogram of the kept lengths (qualsplit.c) */
static int qtrim_and_write(sdt_ctx *gpu, unsigned long long reads, const sdt_quality_params *prm, const sdt_read_quality *rec, uint64_t n_kept,
                           const sdt_pair_ranges *pairs, const char *prefix)
{
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0) return 1;
	char path[4][4200];
	snprintf(path[0], sizeof path[0], "%s.readQual", prefix);
	snprintf(path[1], sizeof path[1], "%s.qtrim.pairs.fa", prefix);
	snprintf(path[2], sizeof path[2], "%s.qtrim.single.fa", prefix);
	snprintf(path[3], sizeof path[3], "%s.lenHist", prefix);
	outbuf oq, opair, osingle;
	if (ob_open(&oq, path[0]) != 0) return 1;
	if (ob_open(&opair, path[1]) != 0) { ob_close(&oq); return 1; }
	if (ob_open(&osingle, path[2]) != 0) { ob_close(&oq); ob_close(&opair); return 1; }
	sdt_len_hist hist;
	memset(&hist, 0, sizeof hist);
	unsigned long long kept = 0;
	size_t cursor = 0;
	int bad = 0;
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (!oq.ok || !opair.ok || !osingle.ok) break;                                 /* a write failed: ob_close says which */
		if (k.at_batch[ord] == 0xFFFFFFFFu) { fprintf(stderr, "sdt-kmers: no kept read has ordinal %llu\n", (unsigned long long)ord); bad = 1; break; }
		const sdt_read_quality *t = rec + ord;
		const uint64_t start = k.bo[k.at_batch[ord]][k.at_read[ord]], len = k.bo[k.at_batch[ord]][k.at_read[ord] + 1] - start;
		const int noted = sdt_len_hist_note(&hist, t, len, prm);
		if (noted != 0) {
			if (noted == -1) fprintf(stderr, "sdt-kmers: out of memory for the histogram\n");
			else fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->span, t->low,
			             t->ee_ppm, t->start, t->len, t->verdict, (unsigned long long)len);
			bad = 1;
			break;
		}
		ob_room(&oq, SDT_QUAL_LINE_MAX);
		oq.p = sdt_put_qual_line(oq.p, t);
		/* (start and len sit where sdt_read_trim has them: qualsplit.h) */
		const int to = sdt_trim_route(pairs, &cursor, (const sdt_read_trim *)rec, reads, ord);
		if (to == SDT_TRIM_TO_NONE) continue;
		kept++;
		outbuf *o = to == SDT_TRIM_TO_PAIRS ? &opair : &osingle;
		ob_room(o, (size_t)t->len + 24);
		o->p = sdt_put_fasta_record(o->p, ord, k.bw[k.at_batch[ord]], start + t->start, t->len);
	}
	const int all_written = oq.ok && opair.ok && osingle.ok;
	if ((ob_close(&oq) != 0) | (ob_close(&opair) != 0) | (ob_close(&osingle) != 0) || bad) return 1;
	if (all_written && kept != n_kept) { fprintf(stderr, "sdt-kmers: the device kept %llu reads, the records say %llu\n", (unsigned long long)n_kept, kept); return 1; }
	FILE *fh = fopen(path[3], "w");
	if (!fh || (sdt_len_hist_write(fh, &hist) != 0) | (fclose(fh) != 0)) { fprintf(stderr, "sdt-kmers: cannot write %s\n", path[3]); return 1; }
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped (%llu short, %llu low bases, %llu expected errors); %llu bases in, %llu bases out\n", reads,
	       (unsigned long long)hist.whole, (unsigned long long)hist.clipped, (unsigned long long)hist.dropped, (unsigned long long)hist.n_short,
	       (unsigned long long)hist.n_low, (unsigned long long)hist.n_errors, (unsigned long long)hist.bases_in, (unsigned long long)hist.bases_out);
	sdt_len_hist_free(&hist);
	kept_free(&k);
	return 0;
}

/* the letters of a tail option as a mask of base codes (A0 C1 T2 G3), or -1 */
static int tail_mask(const char *opt, const char *text)
{
	int mask = 0;
	for (const char *c = text; *c; c++) {
		if (!strchr("ACGTacgt", *c)) { fprintf(stderr, "sdt-kmers: %s %s: letters of ACGT are expected\n", opt, text); return -1; }
		mask |= 1 << ((*c & 6) >> 1);
	}
	return mask;
}

/* the whole of text as a decimal number of at most `most`, or the option is refused by name */
static int parse_number(const char *opt, const char *text, unsigned long long most, unsigned long long *v)
{
	char *end = NULL;
	errno = 0;
	*v = strtoull(text, &end, 10);
	if (text[0] < '0' || text[0] > '9' || *end || errno || *v > most) {
		fprintf(stderr, "sdt-kmers: %s %s: a whole number from 0 to %llu is expected\n", opt, text, most);
		return -1;
	}
	return 0;
}

typedef struct { char **text; uint64_t *keys; uint64_t n, cap; } query_set;

/* one k-mer per line, letters ACGT (either case), exactly K of them; blank lines are skipped.  Base codes A0 C1 T2 G3. */
static int load_queries(const char *path, int K, int nw, query_set *q)
{
	FILE *fi = fopen(path, "r");
	if (!fi) { fprintf(stderr, "sdt-kmers: cannot open %s\n", path); return 2; }
	char *line = NULL;
	size_t cap = 0;
	unsigned long long lineno = 0;
	memset(q, 0, sizeof *q);
	while (getline(&line, &cap, fi) >= 0) {
		lineno++;
		size_t len = strlen(line);
		while (len && (line[len - 1] == '\n' || line[len - 1] == '\r' || line[len - 1] == ' ' || line[len - 1] == '\t')) line[--len] = 0;
		if (!len) continue;
		if (len != (size_t)K) {
			fprintf(stderr, "sdt-kmers: %s line %llu: the k-mer has %zu letters, K is %d\n", path, lineno, len, K);
			fclose(fi);
			return 2;
		}
		if (q->n == q->cap) {
			q->cap = q->cap ? 2 * q->cap : 1024;
			q->text = (char **)realloc(q->text, q->cap * sizeof(char *));
			q->keys = (uint64_t *)realloc(q->keys, q->cap * (size_t)nw * sizeof(uint64_t));
			if (!q->text || !q->keys) { fprintf(stderr, "sdt-kmers: out of memory\n"); fclose(fi); return 1; }
		}
		uint64_t *key = q->keys + q->n * (size_t)nw;
		memset(key, 0, (size_t)nw * sizeof(uint64_t));
		for (int i = 0; i < K; i++) {
			int code;
			switch (line[i]) {
			case 'A': case 'a': code = 0; break;
			case 'C': case 'c': code = 1; break;
			case 'T': case 't': code = 2; break;
			case 'G': case 'g': code = 3; break;
			default:
				fprintf(stderr, "sdt-kmers: %s line %llu: '%c' at position %d is not one of ACGT\n", path, lineno, line[i], i + 1);
				fclose(fi);
				return 2;
			}
			const int bit = 2 * (K - 1 - i);                     /* first base in the most significant pair, words most significant first */
			key[nw - 1 - bit / 64] |= (uint64_t)code << (bit % 64);
		}
		q->text[q->n++] = strdup(line);
	}
	free(line);
	fclose(fi);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2 || (strcmp(argv[1], "profile") != 0 && strcmp(argv[1], "query") != 0 && strcmp(argv[1], "correct") != 0 &&
	                 strcmp(argv[1], "normalize") != 0 && strcmp(argv[1], "trim") != 0 && strcmp(argv[1], "dedup") != 0 && strcmp(argv[1], "clip") != 0 &&
	                 strcmp(argv[1], "overlap") != 0 && strcmp(argv[1], "complexity") != 0 && strcmp(argv[1], "qtrim") != 0 &&
	                 strcmp(argv[1], "screen") != 0)) { usage(); return 255; }
	const int do_query = strcmp(argv[1], "query") == 0, do_correct = strcmp(argv[1], "correct") == 0, do_norm = strcmp(argv[1], "normalize") == 0;
	const int do_trim = strcmp(argv[1], "trim") == 0, do_dedup = strcmp(argv[1], "dedup") == 0, do_clip = strcmp(argv[1], "clip") == 0;
	const int do_overlap = strcmp(argv[1], "overlap") == 0, do_cx = strcmp(argv[1], "complexity") == 0, do_qtrim = strcmp(argv[1], "qtrim") == 0;
	const int do_screen = strcmp(argv[1], "screen") == 0;
	sdt_screen_params sprm = {1, 0, 0, 0};
	uint32_t screen_k = 31;                                                  /* bbduk's usual figure: a choice, not a measurement */
	enum { MAX_REF_FILES = 256 };
	static char *rfile[MAX_REF_FILES];
	int n_rfiles = 0;
	sdt_quality_params qprm = {33, 20, 15, 40, 0, 0, 0, 0};
	sdt_overlap_params oprm = {30, 10, 0, 0};
	sdt_complexity_params xprm = {10, 50, 0, 0};
	int max_low_given = 0;
	sdt_clip_params cprm = {5, 10, 0, 10, 20, 0, 0, 0};
	char afile[2][4096] = {"", ""};                                          /* -a: 3' adapters, -g: 5' adapters */
	sdt_dedup_params dprm = {0, 0};
	sdt_norm_params prm = {50, 10000, 0};
	sdt_trim_params tprm = {0, 0, 0, 0};
	char cfgfile[4096] = "", outname[4096] = "", qfile[4096] = "";
	int K = 23, threads = 8, d = 0, max_k = 0, device = 0, c;
	unsigned long min_count = do_correct || do_trim ? 2 : 0;
	static struct option longopts[] = {{"max-k", required_argument, 0, 1000}, {"device", required_argument, 0, 1001},
	                                   {"target", required_argument, 0, 1002}, {"max-cv", required_argument, 0, 1003},
	                                   {"seed", required_argument, 0, 1004}, {"min-cov", required_argument, 0, 1005},
	                                   {"min-len", required_argument, 0, 1006}, {"correct", no_argument, 0, 1007},
	                                   {"mate-swap", no_argument, 0, 1008}, {"tail3", required_argument, 0, 1009},
	                                   {"tail5", required_argument, 0, 1010}, {"min-overlap", required_argument, 0, 1011},
	                                   {"error-pct", required_argument, 0, 1012}, {"min-tail", required_argument, 0, 1013},
	                                   {"tail-error-pct", required_argument, 0, 1014}, {"max-err", required_argument, 0, 1015},
	                                   {"max-score", required_argument, 0, 1016}, {"max-low", required_argument, 0, 1017},
	                                   {"trim-low", no_argument, 0, 1018}, {"phred", required_argument, 0, 1019},
	                                   {"cut-q", required_argument, 0, 1020}, {"low-q", required_argument, 0, 1021},
	                                   {"max-low-bases", required_argument, 0, 1022}, {"max-ee", required_argument, 0, 1023},
	                                   {"screen-k", required_argument, 0, 1024}, {"min-hits", required_argument, 0, 1025},
	                                   {"min-hit-pct", required_argument, 0, 1026}, {"keep-matched", no_argument, 0, 1027},
	                                   {0, 0, 0, 0}};
	argv++; argc--;
	while ((c = getopt_long(argc, argv, "s:K:p:d:c:o:q:a:g:r:", longopts, NULL)) != -1) {
		switch (c) {
		case 's': snprintf(cfgfile, sizeof cfgfile, "%s", optarg); break;
		case 'o': snprintf(outname, sizeof outname, "%s", optarg); break;
		case 'q': snprintf(qfile, sizeof qfile, "%s", optarg); break;
		case 'K': K = atoi(optarg); break;
		case 'p': threads = atoi(optarg) > 0 ? atoi(optarg) : 1; break;
		case 'd': d = atoi(optarg) >= 0 ? atoi(optarg) : 0; break;           /* pregraph.c:159 */
		case 'c': min_count = strtoul(optarg, NULL, 10); break;
		case 1000: max_k = atoi(optarg); break;
		case 1001: device = atoi(optarg); break;
		case 1002: case 1003: case 1004: {
			const char *opt = c == 1002 ? "--target" : (c == 1003 ? "--max-cv" : "--seed");
			unsigned long long v;
			if (!do_norm) { fprintf(stderr, "sdt-kmers: %s belongs to normalize\n", opt); usage(); return 255; }
			if (parse_number(opt, optarg, c == 1004 ? UINT64_MAX : UINT32_MAX, &v) != 0) return 255;
			if (c == 1002) prm.target = (uint32_t)v;
			else if (c == 1003) prm.max_cv_pct = (uint32_t)v;
			else prm.seed = v;
			break;
		}
		case 1005: case 1006: case 1007: {
			const char *opt = c == 1005 ? "--min-cov" : (c == 1006 ? "--min-len" : "--correct");
			unsigned long long v;
			if (!do_trim && !((do_clip || do_overlap || do_cx || do_qtrim) && c == 1006)) {
				fprintf(stderr, "sdt-kmers: %s belongs to trim%s\n", opt, c == 1006 ? ", clip, overlap, complexity and qtrim" : "");
				usage();
				return 255;
			}
			if (c == 1007) { tprm.flags |= SDT_TRIM_CORRECTED; break; }
			if (parse_number(opt, optarg, UINT32_MAX, &v) != 0) return 255;
			if (c == 1005) tprm.min_cov = (uint32_t)v;
			else tprm.min_len = cprm.min_len = oprm.min_len = xprm.min_len = qprm.min_len = (uint32_t)v;
			break;
		}
		case 'a': case 'g': case 1009: case 1010: case 1011: case 1012: case 1013: case 1014: {
			static const char *const names[] = {"--tail3", "--tail5", "--min-overlap", "--error-pct", "--min-tail", "--tail-error-pct"};
			const char *opt = c == 'a' ? "-a" : (c == 'g' ? "-g" : names[c - 1009]);
			unsigned long long v;
			if (!do_clip && !(do_overlap && c == 1011)) { fprintf(stderr, "sdt-kmers: %s belongs to clip\n", opt); usage(); return 255; }
			if (c == 'a' || c == 'g') { snprintf(afile[c == 'g'], sizeof afile[0], "%s", optarg); break; }
			if (c == 1009 || c == 1010) {
				const int mask = tail_mask(opt, optarg);
				if (mask < 0) return 255;
				if (c == 1009) cprm.tail3_bases = (uint32_t)mask; else cprm.tail5_bases = (uint32_t)mask;
				break;
			}
			if (parse_number(opt, optarg, c == 1012 || c == 1014 ? 100 : UINT32_MAX, &v) != 0) return 255;
			if ((c == 1011 || c == 1013) && v == 0) { fprintf(stderr, "sdt-kmers: %s must be at least 1\n", opt); return 255; }
			if (c == 1011) cprm.min_overlap = oprm.min_overlap = (uint32_t)v;
			else if (c == 1012) cprm.max_err_pct = (uint32_t)v;
			else if (c == 1013) cprm.min_tail = (uint32_t)v;
			else cprm.tail_err_pct = (uint32_t)v;
			break;
		}
		case 1015: {
			unsigned long long v;
			if (!do_overlap) { fprintf(stderr, "sdt-kmers: --max-err belongs to overlap\n"); usage(); return 255; }
			if (parse_number("--max-err", optarg, 100, &v) != 0) return 255;
			oprm.max_err_pct = (uint32_t)v;
			break;
		}
		case 1016: case 1017: case 1018: {
			const char *opt = c == 1016 ? "--max-score" : (c == 1017 ? "--max-low" : "--trim-low");
			unsigned long long v;
			if (!do_cx) { fprintf(stderr, "sdt-kmers: %s belongs to complexity\n", opt); usage(); return 255; }
			if (c == 1018) { xprm.flags |= SDT_COMPLEXITY_TRIM; break; }
			if (parse_number(opt, optarg, 100, &v) != 0) return 255;
			if (c == 1016 && v == 0) { fprintf(stderr, "sdt-kmers: --max-score must be at least 1: at 0 every window would be low\n"); return 255; }
			if (c == 1016) xprm.max_score_pct = (uint32_t)v;
			else { xprm.max_low_pct = (uint32_t)v; max_low_given = 1; }
			break;
		}
		case 1019: case 1020: case 1021: case 1022: case 1023: {
			static const char *const names[] = {"--phred", "--cut-q", "--low-q", "--max-low-bases", "--max-ee"};
			const char *opt = names[c - 1019];
			unsigned long long v;
			if (!do_qtrim) { fprintf(stderr, "sdt-kmers: %s belongs to qtrim\n", opt); usage(); return 255; }
			if (parse_number(opt, optarg, c == 1019 ? 64 : (c == 1022 ? 100 : (c == 1023 ? UINT32_MAX : 93)), &v) != 0) return 255;
			if (c == 1019 && v != 33 && v != 64) { fprintf(stderr, "sdt-kmers: --phred %llu: 33 or 64\n", v); return 255; }
			if (c == 1019) qprm.phred_offset = (uint32_t)v;
			else if (c == 1020) qprm.cut_q = (uint32_t)v;
			else if (c == 1021) qprm.low_q = (uint32_t)v;
			else if (c == 1022) qprm.max_low_pct = (uint32_t)v;
			else qprm.max_ee_ppm = (uint32_t)v;
			break;
		}
		case 'r': case 1024: case 1025: case 1026: case 1027: {
			static const char *const names[] = {"--screen-k", "--min-hits", "--min-hit-pct", "--keep-matched"};
			const char *opt = c == 'r' ? "-r" : names[c - 1024];
			unsigned long long v;
			if (!do_screen) { fprintf(stderr, "sdt-kmers: %s belongs to screen\n", opt); usage(); return 255; }
			if (c == 'r') {
				if (n_rfiles == MAX_REF_FILES) { fprintf(stderr, "sdt-kmers: more than %d -r files\n", MAX_REF_FILES); return 255; }
				rfile[n_rfiles++] = optarg;
				break;
			}
			if (c == 1027) { sprm.flags |= SDT_SCREEN_KEEP_MATCHED; break; }
			if (parse_number(opt, optarg, c == 1024 ? 31 : (c == 1026 ? 100 : UINT32_MAX), &v) != 0) return 255;
			if (c == 1024 && v < 11) { fprintf(stderr, "sdt-kmers: --screen-k %llu: 11 to 31\n", v); return 255; }
			if (c == 1024) screen_k = (uint32_t)v;
			else if (c == 1025) sprm.min_hits = (uint32_t)v;
			else sprm.min_hit_pct = (uint32_t)v;
			break;
		}
		case 1008:
			if (!do_dedup) { fprintf(stderr, "sdt-kmers: --mate-swap belongs to dedup\n"); usage(); return 255; }
			dprm.flags |= SDT_DEDUP_MATE_SWAP;
			break;
		default: usage(); return 255;
		}
	}
	if (!cfgfile[0] || (do_query ? !qfile[0] : !outname[0])) { usage(); return 255; }
	if (do_screen && n_rfiles == 0) { fprintf(stderr, "sdt-kmers: screen needs a reference file: -r refs.fa\n"); usage(); return 255; }
	if (do_norm && prm.target == 0) { fprintf(stderr, "sdt-kmers: --target must be at least 1\n"); return 255; }
	if (xprm.flags & SDT_COMPLEXITY_TRIM) {
		if (max_low_given && xprm.max_low_pct != 0) {
			fprintf(stderr, "sdt-kmers: --max-low %u with --trim-low: the longest clean stretch is kept, whatever fraction is low; give --max-low 0 or none\n",
			        xprm.max_low_pct);
			return 255;
		}
		xprm.max_low_pct = 0;
	}
	if (max_k == 0) max_k = K <= 31 ? 31 : SDT_MAX_K;
	if (d > 127) d = (signed char)d;                                         /* deLowKmer is a char */
	/* pregraph.c:38-59 */
	if (K % 2 == 0) { K++; printf("K should be an odd number\n"); }
	if (K < 13) { K = 13; printf("K should not be less than 13\n"); }
	else if (K > max_k) K = max_k;
	const int nw = K <= 31 ? 1 : (K <= 63 ? 2 : 4);

	/* the adapter files are read and checked before the device is touched, the 3' file first */
	sdt_adapter_list ads;
	memset(&ads, 0, sizeof ads);
	for (int e = 0; e < 2 && do_clip; e++) {
		char err[4400];
		if (afile[e][0] && sdt_adapters_load(&ads, afile[e], e, err, sizeof err) != 0) { fprintf(stderr, "sdt-kmers: %s\n", err); return 2; }
	}
	for (uint32_t i = 0; i < ads.n; i++)
		if (ads.offsets[i + 1] - ads.offsets[i] < cprm.min_overlap) {
			fprintf(stderr, "sdt-kmers: adapter %s has %llu bases, fewer than --min-overlap %u\n", ads.names[i],
			        (unsigned long long)(ads.offsets[i + 1] - ads.offsets[i]), cprm.min_overlap);
			return 2;
		}
	/* the reference files are read and checked before the device is touched, in the order given */
	sdt_ref_set refs;
	memset(&refs, 0, sizeof refs);
	for (int i = 0; i < n_rfiles; i++) {
		char err[4400];
		if (sdt_refs_load(&refs, rfile[i], err, sizeof err) != 0) { fprintf(stderr, "sdt-kmers: %s\n", err); return 2; }
	}
	if (do_screen) {
		if (sdt_refs_pack(&refs) != 0) { fprintf(stderr, "sdt-kmers: out of memory for the references\n"); return 2; }
		uint64_t positions = 0;
		for (uint64_t i = 0; i < refs.nseqs; i++)
			if (refs.offsets[i + 1] - refs.offsets[i] >= screen_k) positions += refs.offsets[i + 1] - refs.offsets[i] - screen_k + 1;
		if (positions == 0) { fprintf(stderr, "sdt-kmers: the references hold no stretch of %u letters ACGT: no k-mer to screen against\n", screen_k); return 2; }
	}
	query_set qs;
	memset(&qs, 0, sizeof qs);
	if (do_query) {
		const int rq = load_queries(qfile, K, nw, &qs);
		if (rq != 0) return rq;
	}
	sdt_cfg cfg;
	if (sdt_cfg_load(cfgfile, &cfg) != 0) return 255;
	const int max_read_len = cfg.max_rd_len ? cfg.max_rd_len : 100;         /* prlHashReads.c:361-364 */
	/* qtrim: every read needs its qualities; refused before the device is touched and before anything is written */
	for (int i = 0; i < cfg.nlibs && do_qtrim; i++) {
		const sdt_lib *l = &cfg.libs[i];
		const char *fasta = l->nf ? l->f[0] : (l->nf1 ? l->f1[0] : (l->nf2 ? l->f2[0] : (l->np ? l->p[0] : (l->nb ? l->b[0] : NULL))));
		if (fasta) { fprintf(stderr, "sdt-kmers: qtrim needs base qualities: %s is not a FASTQ file (q1= / q2= / q=)\n", fasta); return 2; }
	}

	sdt_ctx *gpu = NULL;
	if (sdt_gpu_init(&gpu, device, K, 0, do_query ? 0u : SDT_FLAG_KEEP_READS) != SDT_OK) {
		fprintf(stderr, "sdt_gpu_init: %s\n", sdt_gpu_last_error());
		return 1;
	}
	sdt_pair_ranges pairs;
	memset(&pairs, 0, sizeof pairs);
	push_state st = {gpu, 0, do_norm || do_trim || do_dedup || do_clip || do_overlap || do_cx || do_qtrim || do_screen ? &pairs : NULL};
	qtrim_state qst;
	memset(&qst, 0, sizeof qst);
	if (do_qtrim) {
		if (sdt_gpu_init(&qst.qgpu, device, K, 1, 0) != SDT_OK) { fprintf(stderr, "sdt_gpu_init: %s\n", sdt_gpu_last_error()); return 1; }
		qst.push = st;
		qst.prm = &qprm;
		sdt_read_quals(1);
	}
	const size_t chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);
	const int parse_threads = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : threads;
	sdt_pool_enable(sdt_gpu_host_alloc, sdt_gpu_host_free, parse_threads + PUSH_DEPTH + 8);
	int rc = do_qtrim ? sdt_stream_reads(&cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, qtrim_batch, &qst, NULL)
	                  : sdt_stream_reads(&cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, push_batch, &st, NULL);
	if (do_qtrim) {
		st.reads = qst.push.reads;
		sdt_read_quals(0);
		sdt_gpu_destroy(qst.qgpu);
	}
	if (rc == 0 && inflight_retire(gpu, 0) != 0) rc = -1;
	sdt_pool_disable();
	if (rc != 0) { sdt_gpu_destroy(gpu); return 1; }
	uint64_t kmers = 0, nodes = 0, removed = 0;
	if (sdt_gpu_finish_count(gpu, &kmers, &nodes) != SDT_OK) { fprintf(stderr, "sdt_gpu_finish_count: %s\n", sdt_gpu_last_error()); return 1; }
	printf("%llu reads, %llu nodes allocated, %llu kmer in reads\n", st.reads, (unsigned long long)nodes, (unsigned long long)kmers);
	if (d && sdt_gpu_delow(gpu, d, &removed) != SDT_OK) { fprintf(stderr, "sdt_gpu_delow: %s\n", sdt_gpu_last_error()); return 1; }
	if (d) printf("%llu kmer removed\n", (unsigned long long)removed);

	if (do_norm) {
		if (normalize_and_write(gpu, st.reads, &prm, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
	} else if (do_trim) {
		tprm.min_count = (uint32_t)min_count;
		if (trim_and_write(gpu, st.reads, &tprm, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
	} else if (do_dedup) {
		if (dedup_and_write(gpu, st.reads, &dprm, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
	} else if (do_clip) {
		if (clip_and_write(gpu, st.reads, &cprm, &ads, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
		sdt_adapters_free(&ads);
	} else if (do_overlap) {
		if (overlap_and_write(gpu, st.reads, &oprm, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
	} else if (do_cx) {
		if (complexity_and_write(gpu, st.reads, &xprm, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
	} else if (do_screen) {
		if (screen_and_write(gpu, st.reads, &sprm, screen_k, &refs, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
		sdt_refs_free(&refs);
	} else if (do_qtrim) {
		if (st.reads > qst.cap) { fprintf(stderr, "sdt-kmers: %llu reads streamed, records for %llu\n", st.reads, (unsigned long long)qst.cap); return 1; }
		if (qtrim_and_write(gpu, st.reads, &qprm, qst.rec, qst.n_kept, &pairs, outname) != 0) return 1;
		sdt_pair_ranges_free(&pairs);
		free(qst.rec); free(qst.dense);
	} else if (do_correct) {
		if (correct_and_write(gpu, st.reads, (uint32_t)min_count, outname) != 0) return 1;
	} else if (!do_query) {
		char path[4200];
		snprintf(path, sizeof path, "%s.readCov", outname);
		sdt_read_cov *cov = (sdt_read_cov *)calloc(st.reads ? st.reads : 1, sizeof(sdt_read_cov));
		if (!cov) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", st.reads); return 1; }
		uint64_t got = 0;
		if (sdt_gpu_profile_kept_reads(gpu, (uint32_t)min_count, cov, st.reads, &got) != SDT_OK) {
			fprintf(stderr, "sdt_gpu_profile_kept_reads: %s\n", sdt_gpu_last_error());
			return 1;
		}
		if (got != st.reads) { fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu profiled\n", st.reads, (unsigned long long)got); return 1; }
		if (write_read_cov(path, cov, st.reads) != 0) return 1;
		printf("%llu reads profiled into %s\n", st.reads, path);
		free(cov);
	} else {
		/* `linear` is thread_mark's flag (prlHashReads.c:911-967): marked on the table as it is now */
		int64_t hist[257];
		uint64_t linear = 0;
		if (sdt_gpu_mark_and_hist(gpu, hist, &linear) != SDT_OK) { fprintf(stderr, "sdt_gpu_mark_and_hist: %s\n", sdt_gpu_last_error()); return 1; }
		const uint64_t n = qs.n, m = n ? n : 1;
		uint32_t *cnt = (uint32_t *)calloc(m, 4), *ll = (uint32_t *)calloc(m, 4), *rf = (uint32_t *)calloc(m, 4);
		uint8_t *stt = (uint8_t *)calloc(m, 1);
		if (!cnt || !ll || !rf || !stt) { fprintf(stderr, "sdt-kmers: out of memory\n"); return 1; }
		if (sdt_gpu_search_kmers(gpu, qs.keys, n, cnt, ll, rf, stt) != SDT_OK) { fprintf(stderr, "sdt_gpu_search_kmers: %s\n", sdt_gpu_last_error()); return 1; }
		FILE *fo = outname[0] ? fopen(outname, "w") : stdout;
		if (!fo) { fprintf(stderr, "sdt-kmers: cannot write %s\n", outname); return 1; }
		for (uint64_t i = 0; i < n; i++)
			fprintf(fo, "%s\t%d\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", qs.text[i], stt[i] & 1, (stt[i] & 2) ? '-' : '+', cnt[i],
			        ll[i] & 63u, (ll[i] >> 6) & 63u, (ll[i] >> 12) & 63u, (ll[i] >> 18) & 63u,
			        rf[i] & 63u, (rf[i] >> 6) & 63u, (rf[i] >> 12) & 63u, (rf[i] >> 18) & 63u, (rf[i] >> 24) & 1u, (rf[i] >> 25) & 1u);
		if (fo != stdout && fclose(fo) != 0) { fprintf(stderr, "sdt-kmers: write to %s failed\n", outname); return 1; }
		free(cnt); free(ll); free(rf); free(stt);
	}
	sdt_gpu_destroy(gpu);
	sdt_cfg_free(&cfg);
	return 0;
}
