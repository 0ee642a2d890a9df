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
 *   sdt-kmers merge -s lib.cfg -K k [-p threads] [--min-overlap N, default 30] [--max-err PCT, default 10] [--min-len L, default 0]
 *                   [--min-merged L, default 0] [--max-merged L, default 0 = no limit] -o prefix
 *       the two mates of every pair that overlaps merged into one fragment read (sdt_gpu_overlap_kept_pairs, then
 *       sdt_gpu_merge_kept_pairs; the rule: include/sdt_gpu.h); FASTA and FASTQ libraries alike, no qualities are used: a mismatch
 *       column takes mate 1's base.  Pairs as for normalize; a library without pairs is allowed: nothing merges (mergesplit.c)
 *       prefix.readMerge: one line per read in stream order:  merged mismatches from_b start len verdict
 *       prefix.merge.fa: the merged fragments, one record per merged pair, > the first mate's ordinal + 1
 *       prefix.merge.pairs.fa / prefix.merge.single.fa: the kept bases of the reads that did not merge, as overlap writes them
 *       prefix.insertHist: as overlap writes it
 *   sdt-kmers qc -s lib.cfg -K k [-p threads] [--cycles C, default 1024] [--phred 33|64, default 33] [--from-end] -o prefix
 *       the per-cycle QC report of the libraries as they stream: base composition and qualities by cycle, read lengths, GC and mean
 *       quality, by class of reads (0 single reads, 1 first mates, 2 second mates).  One sdt_gpu_qc_reads per batch into the report of
 *       the batch's class (the rule: include/sdt_gpu.h); nothing is counted or kept.  FASTQ and FASTA libraries alike: the quality
 *       outputs say which class came without qualities (qcsplit.c, which documents the three files)
 *       prefix.qcBases / prefix.qcQuals / prefix.qcReads, and one line per class on stdout
 *   sdt-kmers evaluate -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] --assembly contigs.fa [--assembly more.fa ...]
 *                      [--rows R, default 256] -o prefix
 *       an assembly scored against the counted k-mers of the reads (sdt_gpu_asm_begin / _add / _spectrum; the rule: include/sdt_gpu.h):
 *       how much of the reads' solid k-mer content it holds, how much of it has no read support, and how many times it holds each
 *       read k-mer.  The assembly files are FASTA, read and checked before the device is touched; every letter outside ACGT cuts a
 *       contig into segments, so the N runs of a scaffold never become k-mers (asmsplit.c folds the segments back)
 *       prefix.asmSupport: per contig  index name bases kmers found solid sum gaps longest_gap longest_at
 *       prefix.asmSpectrum: row c0 .. c7 for the rows of the copy-number spectrum that hold a node
 *       and one line: evaluate: sequences S kmers N found F solid V nodes D solid_nodes E covered C completeness_x100 P qv_x100 Q
 *   sdt-kmers compare -s a.cfg --against b.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--rows R, default 64]
 *                     [--cols C, default 64] [--select MINA:MAXA:MINB:MAXB] [--max-list N, default 1000000] -o prefix
 *       the counted k-mers of two sets of libraries against each other (sdt_gpu_compare_tables, sdt_gpu_compare_select; the rule:
 *       include/sdt_gpu.h): a.cfg is counted into one context, b.cfg into a second on the same device, -d applied to both
 *       prefix.cmpMatrix: the joint spectrum; prefix.cmpKmers (--select): the k-mers of A in the ranges, with both counts
 *       and one line: compare: nodes_a X nodes_b Y shared S solid_a P solid_b Q solid_shared T jaccard_x10000 J contain_a_x10000 U
 *       contain_b_x10000 V braycurtis_x10000 W   (cmpsplit.c, which documents the files and the ratios)
 *   sdt-kmers cluster -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0 = no limit]
 *                     [--min-link N, default 1] [--pick LO:HI] -o prefix
 *       the reads split along the connected components of the counted k-mer graph (sdt_gpu_cluster_begin, sdt_gpu_cluster_kept_reads,
 *       sdt_gpu_cluster_components; the rule: include/sdt_gpu.h).  The two mates of a pair are one unit; pairs as for normalize.  Ids
 *       are 1-based in every file and 0 means none (clustersplit.c, which documents the files)
 *       prefix.readCluster: one line per read in stream order:  kmers live split cluster unit verdict
 *       prefix.clusters: per cluster  id kmer nodes count_sum reads bases,  then  # live L link_ends E clusters C largest N unassigned U
 *       prefix.cluster.pairs.fa / prefix.cluster.single.fa: the reads, as dedup routes and names them, with " cluster=<id>" behind the
 *       name; with --pick only the units of the clusters LO .. HI
 *       and one line: cluster: reads R assigned A whole W through_mate M unassigned U short S clusters C largest_nodes N largest_reads X
 *   sdt-kmers bubbles -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0 = no limit]
 *                     [--min-link N, default 1] [--max-branch L, default 1000] -o prefix
 *       the bubbles of the counted k-mer graph, the variants that graph cleaning would merge (sdt_gpu_bubbles_begin, sdt_gpu_bubbles_fetch,
 *       sdt_gpu_bubbles_paths; the rule: include/sdt_gpu.h).  No read is kept.  Ids are 1-based (bubblesplit.c, which documents the files)
 *       prefix.bubbles: per bubble  id source sink base_a base_b len_a len_b min_a min_b sum_a sum_b link_a link_b kind
 *       prefix.bubbles.fa: the two alleles of every bubble, >id_a and >id_b
 *       and one line: bubbles: live L forks F branches B reached R bubbles N kind0 X kind1 Y kind2 Z longest M
 *   sdt-kmers unitigs -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0 = no limit]
 *                     [--min-link N, default 1] -o prefix
 *       the unitigs of the counted k-mer graph and their links, the compacted graph before any cleaning (sdt_gpu_unitigs_begin,
 *       sdt_gpu_unitigs_fetch, sdt_gpu_unitigs_seqs, sdt_gpu_unitigs_links; the rule: include/sdt_gpu.h).  No read is kept.  Ids are
 *       1-based (unitigsplit.c, which documents the files)
 *       prefix.unitigs: per unitig  id first last nodes bases sum mean_x100 min max in out circular
 *       prefix.unitigs.fa: >id nodes=.. sum=.. min=.. max=.. circular=.. and the sequence on one line
 *       prefix.unitigs.gfa: GFA 1: H, an S line per unitig (LN:i: bases, KC:i: sum), an L line per link, written once (lc:i: its counter)
 *       and one line: unitigs: live L unitigs N circular C isolated I dead_ends D links E bases B longest M n50 X
 *   sdt-kmers thread -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0 = no limit]
 *                    [--min-link L, default 1] -o prefix
 *       every read as a path over the unitig list (sdt_gpu_unitigs_begin, sdt_gpu_unitigs_index, sdt_gpu_unitigs_reads; the rule:
 *       include/sdt_gpu.h).  No read is kept: the libraries are streamed a second time, in the same ordinals.  Ids are 1-based
 *       (threadsplit.c, which documents the files)
 *       prefix.readPaths: per read in stream order  kmers live segs breaks path
 *       prefix.unitigReads: per unitig  id reads segments kmers
 *       prefix.unitigs, prefix.unitigs.fa, prefix.unitigs.gfa: as `unitigs` writes them
 *       and one line: thread: reads R placed P whole W broken B unplaced U short S segments G linked L unlinked X
 *   sdt-kmers support -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0 = no limit]
 *                     [--min-link L, default 1] [--max-junctions J, default 4194304] -o prefix
 *       what the reads support of the unitig list, tallied on the device (sdt_gpu_unitigs_support_*; the rule: include/sdt_gpu.h).  No
 *       read is kept and no segment comes to the host: the libraries are streamed a second time.  Ids are 1-based, an oriented unitig
 *       is <id><+|-> (supportsplit.c, which documents the files).  The mates of a library in two files come in different batches, so
 *       every batch is added as single reads and no mate link is tallied: those are for the callers of the library
 *       prefix.unitigSupport: per unitig  id segments kmers cov_x100
 *       prefix.linkSupport: per link that the GFA writes  from o to o' along against
 *       prefix.junctions: from via to count
 *       prefix.unitigs, prefix.unitigs.fa, prefix.unitigs.gfa: as `unitigs` writes them
 *       and one line: support: reads R placed P segments G kmers L traversals T no_record N passages X junctions J dropped Z
 *
 * The query file is read and checked before the device is touched.
 *
 * What a read stage does after the device has decided -- the record lines and the two FASTA files, by ordinal -- is one walk for all of
 * them (readwalk.c); a stage here is its device calls, a few callbacks for the walk, its statistics file and its summary line. */
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
#include "putdec.h"
#include "readwalk.h"
#include "normsplit.h"
#include "trimsplit.h"
#include "dupsplit.h"
#include "clipsplit.h"
#include "overlapsplit.h"
#include "cxsplit.h"
#include "qualsplit.h"
#include "screensplit.h"
#include "mergesplit.h"
#include "qcsplit.h"
#include "asmsplit.h"
#include "cmpsplit.h"
#include "clustersplit.h"
#include "bubblesplit.h"
#include "unitigsplit.h"
#include "threadsplit.h"
#include "supportsplit.h"
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
	        "       sdt-kmers merge -s lib.cfg -K k [-p threads] [--min-overlap N, default 30] [--max-err PCT, default 10]\n"
	        "                       [--min-len L, default 0] [--min-merged L, default 0] [--max-merged L, default 0] -o prefix\n"
	        "           the overlap of the two mates of every pair is found as `overlap` finds it (--min-overlap, --max-err, --min-len are\n"
	        "           its options); a pair that overlaps with a fragment of at least max(--min-merged, 1) and, unless --max-merged is 0, at\n"
	        "           most --max-merged bases is merged into one read of the fragment's length: mate 1, then what mate 2,\n"
	        "           reverse-complemented, adds behind it.  Where the two mates differ in the overlap, the base of mate 1 stays (the\n"
	        "           command line has no qualities: FASTA and FASTQ libraries alike).  The reads of every other pair are kept as\n"
	        "           `overlap` keeps them.  Needs no counted k-mers: run it in the place of overlap.\n"
	        "           -> prefix.readMerge (per read in stream order: merged mismatches from_b start len verdict; merged = the fragment's\n"
	        "              bases, 0 if the pair did not merge; mismatches = the columns of the overlap in which the mates differ; start,\n"
	        "              len and verdict say what is left of the read outside the merged file: verdict 5 merged, else 0 whole,\n"
	        "              2 clipped, 3 dropped), prefix.merge.fa (one record per merged pair, named by the first mate's read number),\n"
	        "              prefix.merge.pairs.fa (read 1 then read 2 of the pairs that did not merge and of which both mates survive),\n"
	        "              prefix.merge.single.fa (every other surviving read), prefix.insertHist (as overlap writes it)\n"
	        "           and one line: merge: reads R pairs P overlapping V merged M mismatch columns C bases in I bases out O\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files; a library without pairs is allowed: nothing merges.\n"
	        "       sdt-kmers qc -s lib.cfg -K k [-p threads] [--cycles C, default 1024] [--phred 33|64, default 33] [--from-end] -o prefix\n"
	        "           what the parameters of the other stages act on, before or after any of them: per cycle (the position of a base in\n"
	        "           its read, from 0; --from-end: counted from the read's last base) the base composition and the qualities, per read\n"
	        "           its length, its GC content and its mean quality; by class of reads: 0 single reads, 1 first mates, 2 second mates\n"
	        "           (the reads of q1=/q2= and f1=/f2= files).  Row C, written as C+, takes everything past the C-th cycle (C from 1 to\n"
	        "           4096).  FASTQ and FASTA libraries alike; -K is only the k of the context.  Nothing is counted, kept or changed.\n"
	        "           A record whose quality line is not as long as its sequence line stops the run before a file is written.\n"
	        "           -> prefix.qcBases (# class row reads A C T G: per class and row that has a base; reads = the reads that reach the\n"
	        "              row, in row C+ the bases past it), prefix.qcQuals (# class row bases mean_x100 min q10 q25 median q75 q90 max: per\n"
	        "              class and row; mean_x100 = floor(100 * mean quality); the percentile at p = the smallest quality whose cumulative\n"
	        "              count reaches ceil(p * bases / 100); a class without qualities has the one line: # class K: no qualities),\n"
	        "              prefix.qcReads (# hist class bin reads: the histograms len, gc and meanq, only the bins that hold a read; len =\n"
	        "              min(bases, C), bin C written as C+; gc = floor of the percentage of C and G; meanq = floor of the mean quality)\n"
	        "           and one line per class: qc: class K reads R empty E bases B gc G q20 X q30 Y (G, X, Y in hundredths of a percent:\n"
	        "           the share of C and G, of the bases of quality 20 and more, of 30 and more; - without qualities)\n"
	        "       sdt-kmers evaluate -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] --assembly contigs.fa\n"
	        "                          [--assembly more.fa ...] [--rows R, default 256] -o prefix\n"
	        "           an assembly (FASTA files, any line wrapping; a letter other than ACGT cuts a contig, so a scaffold's N runs give no\n"
	        "           k-mers) is scored against the counted k-mers of the reads.  A k-mer of the assembly is weak if the reads hold it\n"
	        "           fewer than max(min_count, 1) times; a gap is a maximal run of weak k-mers: one wrong base makes a gap of K, a\n"
	        "           chimeric junction one of K - 1.  Every node of the table gets the number of times the assembly holds it, either\n"
	        "           strand, up to 255.  R from 2 to 1024, above min_count: row R - 1 takes every larger count.\n"
	        "           -> prefix.asmSupport (per contig: index name bases kmers found solid sum gaps longest_gap longest_at; found = the\n"
	        "              k-mers the reads hold at all, solid = those not weak, sum = the sum of the counts, longest_at = the first base of\n"
	        "              the longest gap's first k-mer, 0-based in the contig, kmers if there is no gap), prefix.asmSpectrum (row c0 .. c7\n"
	        "              for every row that holds a node: the nodes counted min(row, R - 1) times that the assembly holds 0, 1, .. 6, 7 or\n"
	        "              more times)\n"
	        "           and one line: evaluate: sequences S kmers N found F solid V nodes D solid_nodes E covered C completeness_x100 P\n"
	        "           qv_x100 Q (S = the stretches of ACGT scored; E = the nodes counted min_count times or more, C = those of them in\n"
	        "           the assembly, P = floor(10000 C / E); Q = round(100 * -10 log10(1 - (V / N)^(1 / K))), inf when V = N; - when the\n"
	        "           divisor is 0)\n"
	        "       sdt-kmers compare -s a.cfg --against b.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--rows R, default 64]\n"
	        "                         [--cols C, default 64] [--select MINA:MAXA:MINB:MAXB] [--max-list N, default 1000000] -o prefix\n"
	        "           the k-mers of the libraries of a.cfg (A) and of b.cfg (B) are counted into two tables on one device, -d applied to\n"
	        "           both, and the tables are compared: cA and cB are the counts of a canonical k-mer in A and in B, 0 where it is absent.\n"
	        "           R and C from 2, R x C up to 16384, both above min_count: row R - 1 and column C - 1 take every larger count.\n"
	        "           -> prefix.cmpMatrix (a header line a\\b 0 1 .. C-1+ that names the columns, then per row r: r m[r][0] .. m[r][C-1], the\n"
	        "              distinct k-mers of A and B together with min(cA, R - 1) = r and min(cB, C - 1) = c; the last row is written R-1+),\n"
	        "              prefix.cmpKmers (with --select: kmer cA cB for the k-mers of A with MINA <= cA <= MAXA and MINB <= cB <= MAXB, in\n"
	        "              letters, ascending; at most N lines, and when more matched a last line # M matched; the k-mers of B alone: swap\n"
	        "              the two configs)\n"
	        "           and per library its count line, prefixed A: / B:, and one line: compare: nodes_a X nodes_b Y shared S solid_a P\n"
	        "           solid_b Q solid_shared T jaccard_x10000 J contain_a_x10000 U contain_b_x10000 V braycurtis_x10000 W (P, Q, T = the\n"
	        "           k-mers counted min_count times or more in A, in B, in both; J = floor(10000 S / (X + Y - S)), U = floor(10000 S / X),\n"
	        "           V = floor(10000 S / Y), W = floor(10000 (sum cA + sum cB - 2 sum min(cA, cB)) / (sum cA + sum cB)); 0 when the\n"
	        "           divisor is 0)\n"
	        "       sdt-kmers cluster -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0]\n"
	        "                         [--min-link N, default 1] [--pick LO:HI] -o prefix\n"
	        "           the reads are split along the connected components of the counted k-mer graph.  A node is live if it is not deleted\n"
	        "           and counted max(min_count, 1) times or more and, unless M is 0, at most M times (M takes the k-mers of adapters and\n"
	        "           low-complexity sequence out, which glue unrelated transcripts together); a link counted N times or more (1 to 63)\n"
	        "           between two live nodes joins them.  Clusters are numbered from 1 in ascending order of their smallest k-mer; a read\n"
	        "           goes to the cluster of its first live k-mer, a pair to that of mate 1 if it has one, else of mate 2.\n"
	        "           -> prefix.readCluster (per read in stream order: kmers live split cluster unit verdict; live = its live k-mers, split\n"
	        "              = those of them in another cluster than its own, unit = the cluster of the read or pair, 0 none; verdict 0 whole,\n"
	        "              1 assigned but split or apart from its unit, 2 assigned through its mate, 3 unassigned, 4 shorter than K),\n"
	        "              prefix.clusters (per cluster: id kmer nodes count_sum reads bases, the smallest k-mer in letters; then:\n"
	        "              # live L link_ends E clusters C largest N unassigned U), prefix.cluster.pairs.fa (read 1 then read 2 of the\n"
	        "              pairs), prefix.cluster.single.fa (the single reads), every name followed by cluster=<unit>; with --pick only\n"
	        "              the units of the clusters LO to HI are written\n"
	        "           and one line: cluster: reads R assigned A whole W through_mate M unassigned U short S clusters C largest_nodes N\n"
	        "           largest_reads X\n"
	        "           Pairs are the reads of q1=/q2= and f1=/f2= files; the reads of a p= file are single reads, as for normalize.\n"
	        "       sdt-kmers bubbles -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0]\n"
	        "                         [--min-link N, default 1] [--max-branch L, default 1000] -o prefix\n"
	        "           the bubbles of the counted k-mer graph: two paths without a branch that leave one k-mer and meet again -- a SNP or a\n"
	        "           recurring error (K nodes on each side), an indel (unequal sides), a skipped exon (a short side against a long one):\n"
	        "           what graph cleaning would merge.  Live nodes and links as for cluster; a side has at most L inner nodes (1 to 1048576).\n"
	        "           -> prefix.bubbles (per bubble: id source sink base_a base_b len_a len_b min_a min_b sum_a sum_b link_a link_b kind;\n"
	        "              source and sink are k-mers in letters as the bubble is read, base_a < base_b (A C T G) follow the source, len =\n"
	        "              the inner nodes of a side, min and sum = their counts, link = the counter of the side's first step; kind 0:\n"
	        "              len_a = len_b = K, 1: other equal lengths, 2: unequal), prefix.bubbles.fa (>id_a len=.. min=.. sum=.. and the\n"
	        "              allele from source to sink, then the same for b); ids from 1 in ascending order of (source, base_a, base_b)\n"
	        "           and one line: bubbles: live L forks F branches B reached R bubbles N kind0 X kind1 Y kind2 Z longest M\n"
	        "       sdt-kmers unitigs -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0]\n"
	        "                         [--min-link N, default 1] -o prefix\n"
	        "           the unitigs of the counted k-mer graph and their links: the maximal paths without a branch, the compacted graph\n"
	        "           before any cleaning.  Live nodes and links as for cluster.\n"
	        "           -> prefix.unitigs (per unitig: id first last nodes bases sum mean_x100 min max in out circular; first and last are\n"
	        "              k-mers in letters as the unitig is read, bases = nodes + K - 1, sum min max and the mean (x 100, a floor) are over\n"
	        "              the counts of its nodes, in and out the degrees at its ends), prefix.unitigs.fa (>id nodes=.. sum=.. min=.. max=..\n"
	        "              circular=.. and the sequence), prefix.unitigs.gfa (GFA 1: S id seq LN:i:bases KC:i:sum; L from +/- to +/- <K-1>M\n"
	        "              lc:i:link, every link once); ids from 1 in ascending order of the first k-mer\n"
	        "           and one line: unitigs: live L unitigs N circular C isolated I dead_ends D links E bases B longest M n50 X\n"
	        "       sdt-kmers thread -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0]\n"
	        "                        [--min-link L, default 1] -o prefix\n"
	        "           every read laid on the unitig list as a path: the unitigs as `unitigs` finds and writes them, a k-mer -> unitig index\n"
	        "           on the device, and the libraries streamed a second time through it\n"
	        "           -> prefix.readPaths (per read in stream order: kmers live segs breaks path; path = * or the read's segments, each\n"
	        "              <sep><dir><id>:<unitig_pos>+<kmers> with sep none for the first, - over a link of the graph, ~ adjacent in the read\n"
	        "              without such a link, / after k-mers that are not in the graph, and dir > along the unitig, < against it),\n"
	        "              prefix.unitigReads (per unitig: id reads segments kmers), prefix.unitigs, .unitigs.fa and .unitigs.gfa as above\n"
	        "           and one line: thread: reads R placed P whole W broken B unplaced U short S segments G linked L unlinked X\n"
	        "       sdt-kmers support -s lib.cfg -K k [-p threads] [-d d] [-c min_count, default 2] [--max-count M, default 0]\n"
	        "                         [--min-link L, default 1] [--max-junctions J, default 4194304] -o prefix\n"
	        "           what the reads support of the unitig list, tallied on the device; every batch is added as single reads\n"
	        "           prefix.unitigSupport: id segments kmers cov_x100    prefix.linkSupport: from o to o' along against\n"
	        "           prefix.junctions: from via to count    and the files of `unitigs`\n"
	        "           and one line: support: reads R placed P segments G kmers L traversals T no_record N passages X junctions J dropped Z\n"
	        "       (--device n: HIP device ordinal; --max-k 31|63|127: the variant whose K limit applies, default by K)\n");
}

/* "call the ABI, on failure print and leave": 0 when the entry point returned SDT_OK; otherwise 1, after `<entry point>: <error>` has
 * gone to stderr (the twin of sdt-pregraph's, which knows about ranks: pg_ranks.h) */
static int gpu_fail(const char *entry)
{
	fprintf(stderr, "%s: %s\n", entry, sdt_gpu_last_error());
	return 1;
}
#define SDT_CALL(fn, ...) (fn(__VA_ARGS__) == SDT_OK ? 0 : gpu_fail(#fn))

/* pooled batches (pinned buffers, seqio.h) are pushed asynchronously, as sdt-pregraph does */
#define PUSH_DEPTH 12
static struct { int slot[PUSH_DEPTH]; uint64_t ticket[PUSH_DEPTH]; int head, n; } g_inflight;

static int inflight_retire(sdt_ctx *gpu, int down_to)
{
	while (g_inflight.n > down_to) {
		if (SDT_CALL(sdt_gpu_push_wait, gpu, g_inflight.ticket[g_inflight.head])) return -1;
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
		if (rc != SDT_OK) { gpu_fail("sdt_gpu_push_reads_async"); return -1; }
		if (inflight_retire(st->gpu, PUSH_DEPTH - 1) != 0) return -1;
		const int at = (g_inflight.head + g_inflight.n) % PUSH_DEPTH;
		g_inflight.slot[at] = b->pool_slot;
		g_inflight.ticket[at] = ticket;
		g_inflight.n++;
		sdt_pool_take(b->pool_slot);
		return 0;
	}
	return SDT_CALL(sdt_gpu_push_reads, st->gpu, b->words, b->nwords, b->offsets, b->nreads) ? -1 : 0;
}

/* everything the command line says, and what the files it names held */
enum { MAX_REF_FILES = 256 };
typedef struct { char **text; uint64_t *keys; uint64_t n, cap; } query_set;
typedef struct qtrim_state qtrim_state;
typedef struct {
	char cfgfile[4096], outname[4096], qfile[4096];
	int K, threads, d, max_k, device;
	unsigned long min_count;
	sdt_norm_params norm;
	sdt_trim_params trim;
	sdt_dedup_params dedup;
	sdt_clip_params clip;
	char afile[2][4096];                                                     /* -a: 3' adapters, -g: 5' adapters */
	sdt_overlap_params overlap;
	sdt_merge_params merge;
	sdt_complexity_params cx;
	int max_low_given;
	sdt_quality_params qual;
	sdt_qc_params qc;
	sdt_screen_params screen;
	uint32_t screen_k;
	char *rfile[MAX_REF_FILES];
	int n_rfiles;
	char *asmfile[MAX_REF_FILES];                                            /* --assembly: into refs, as the references of screen */
	int n_asmfiles;
	uint32_t rows;
	char againstfile[4096];                                                  /* compare: --against, the library config of B */
	sdt_cfg against;                                                         /* of againstfile */
	uint32_t cols, select[4];                                                /* compare: --cols; --select min_a max_a min_b max_b */
	int select_given;
	unsigned long long max_list;
	sdt_cluster_params cluster;
	uint32_t pick[2];                                                        /* cluster: --pick, as the library takes it */
	int pick_given;
	uint64_t max_junctions;                                                  /* support: the distinct junctions its set may hold */
	uint32_t max_branch;                                                     /* bubbles: --max-branch, the inner nodes of a side at the most */
	sdt_adapter_list ads;                                                    /* of afile[] */
	sdt_ref_set refs;                                                        /* of rfile[] */
	query_set qs;                                                            /* of qfile */
	qtrim_state *qtrim;                                                      /* qtrim's records, taken while the reads streamed */
	const sdt_cfg *cfg;                                                      /* thread: the libraries, for its second pass over them */
} options;

/* ---- the device half that every read stage shares ------------------------------------------------------------------------------------ */

/* by ordinal, every byte `fill` (0xFF: an ordinal that no read has keeps verdict 0xFFFFFFFF); NULL after saying that memory ran out */
static void *records_alloc(unsigned long long reads, size_t size, int fill)
{
	const uint64_t m = reads ? reads : 1;
	void *rec = fill ? malloc(m * size) : calloc(m, size);
	if (!rec) fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads);
	else if (fill) memset(rec, fill, m * size);
	return rec;
}

static int all_reads_came_back(unsigned long long reads, uint64_t got, const char *done)
{
	if (got != reads) fprintf(stderr, "sdt-kmers: %llu reads streamed, %llu %s\n", reads, (unsigned long long)got, done);
	return got == reads;
}

/* the kept batches back from HBM, and where every ordinal's read is */
static int kept_fetch(sdt_ctx *gpu, unsigned long long reads, kept_reads *k)
{
	uint64_t nb = 0;
	if (SDT_CALL(sdt_gpu_kept_batches, gpu, &nb) || kept_init(k, nb, reads)) return 1;
	for (uint64_t b = 0; b < nb; b++) {
		uint64_t info[4];
		if (SDT_CALL(sdt_gpu_fetch_kept_batch, gpu, b, info, NULL, 0, NULL, 0)) return 1;
		uint32_t *w = (uint32_t *)malloc((info[0] ? info[0] : 1) * sizeof(uint32_t));
		uint64_t *o = (uint64_t *)malloc((info[1] + 1) * sizeof(uint64_t));
		if (!w || !o) { fprintf(stderr, "sdt-kmers: out of memory for the reads\n"); return 1; }
		if (SDT_CALL(sdt_gpu_fetch_kept_batch, gpu, b, info, w, info[0], o, info[1] + 1)) return 1;
		if (kept_add(k, b, w, o, info[1], info[2], info[3])) return 1;
	}
	return 0;
}

/* the kept batches back from HBM, walked by ordinal into the stage's three files under the prefix (readwalk.h), and released */
static int fetch_and_walk(sdt_ctx *gpu, unsigned long long reads, const sdt_pair_ranges *pairs, const char *prefix, const sdt_walk_stage *stage, void *state,
                          uint64_t n_kept, sdt_walk_tally *tally)
{
	kept_reads k;
	if (kept_fetch(gpu, reads, &k) != 0 || sdt_walk_reads(&k, pairs, prefix, stage, state, n_kept, tally) != 0) return 1;
	kept_free(&k);
	return 0;
}

/* a stage's statistics file, prefix + suffix; NULL: it cannot be written */
static FILE *stats_open(char path[4200], const char *prefix, const char *suffix)
{
	snprintf(path, 4200, "%s%s", prefix, suffix);
	return fopen(path, "w");
}

static int cannot_write(const char *path)
{
	fprintf(stderr, "sdt-kmers: cannot write %s\n", path);
	return 1;
}

/* ---- correct, and the edits of `trim --correct` -------------------------------------------------------------------------------------- */

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
	if (rc != SDT_OK) return gpu_fail("sdt_gpu_correct_kept_reads");
	if (!all_reads_came_back(reads, got, "corrected")) return 1;
	*edits_out = edits;
	*n_edits_out = n_edits;
	return 0;
}

/* the edits on their way into the reads and into prefix.edits: the first member of the state of the two stages that have them */
typedef struct { outbuf oe; char path[4200]; uint64_t *edits, n, e; } edit_walk;

static int edits_open(edit_walk *ed, const char *prefix)
{
	snprintf(ed->path, sizeof ed->path, "%s.edits", prefix);
	return ob_open(&ed->oe, ed->path);
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
	oe->p = sdt_put_dec(oe->p, ord + 1, ' ');
	oe->p = sdt_put_dec(oe->p, pos + 1, ' ');
	*oe->p++ = letters[old];
	*oe->p++ = ' ';
	*oe->p++ = letters[neu];
	*oe->p++ = '\n';
	return 0;
}

/* sdt_walk_stage.edit: the edits of read `ord` */
static int edits_apply(void *state, uint64_t ord, uint32_t *w, uint64_t start, uint64_t len)
{
	edit_walk *ed = (edit_walk *)state;
	if (!ed->oe.ok) return -1;                                               /* a write failed: ob_close says which */
	for (; ed->e < ed->n && (ed->edits[ed->e] >> 18) == ord; ed->e++)
		if (apply_edit(&ed->oe, ed->edits[ed->e], ord, w, start, len) != 0) return -1;
	return 0;
}

/* after the walk (walked: it went through): the file closed; 0 iff all of it is written and every edit named a read */
static int edits_close(edit_walk *ed, int walked)
{
	if (ob_close(&ed->oe) != 0 || !walked) return 1;
	if (ed->e != ed->n) {
		fprintf(stderr, "sdt-kmers: %llu of %llu edits name no read of the stream\n", (unsigned long long)(ed->n - ed->e), (unsigned long long)ed->n);
		return 1;
	}
	free(ed->edits);
	return 0;
}

typedef struct { edit_walk ed; const sdt_read_fix *rec; unsigned long long with_weak, runs; } correct_state;

static int correct_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	correct_state *s = (correct_state *)state;
	(void)read_len; (void)start; (void)len;                                  /* every read is kept whole */
	s->with_weak += s->rec[ord].weak != 0;
	s->runs += s->rec[ord].runs;
	return 0;
}

static char *correct_line(const void *state, char *p, uint64_t ord)
{
	const sdt_read_fix *r = ((const correct_state *)state)->rec + ord;
	p = sdt_put_dec(p, r->kmers, ' ');
	p = sdt_put_dec(p, r->weak, ' ');
	p = sdt_put_dec(p, r->runs, ' ');
	return sdt_put_dec(p, r->fixed, '\n');
}

static int correct_alive(const void *state, uint64_t ord)
{
	(void)state; (void)ord;
	return 1;
}

/* `correct`: the records and the edits from the device, the kept batches back from HBM, the edits applied on the way into the one file */
static int run_correct(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readFix", NULL, ".corrected.fa"}, 4 * 11, 1, correct_note, correct_line, correct_alive, edits_apply, NULL};
	sdt_read_fix *fix = (sdt_read_fix *)records_alloc(reads, sizeof *fix, 0);
	correct_state st;
	memset(&st, 0, sizeof st);
	if (!fix || correct_kept(gpu, reads, (uint32_t)opt->min_count, fix, &st.ed.edits, &st.ed.n) != 0) return 1;
	st.rec = fix;
	sdt_walk_tally t;
	if (edits_open(&st.ed, opt->outname) != 0) return 1;
	const int walked = fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, reads, &t) == 0;
	const unsigned long long fixed = st.ed.e;
	if (edits_close(&st.ed, walked) != 0) return 1;
	printf("%llu reads, %llu with weak k-mers, %llu runs, %llu bases corrected into %s.corrected.fa\n", reads, st.with_weak, st.runs, fixed, opt->outname);
	free(fix);
	return 0;
}

/* ---- normalize ------------------------------------------------------------------------------------------------------------------------- */
typedef struct { const sdt_read_pick *rec; unsigned long long n_short, aberrant, drawn; } norm_state;

static int norm_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	norm_state *s = (norm_state *)state;
	const uint32_t cls = s->rec[ord].verdict & 7u;
	(void)read_len; (void)start; (void)len;                                  /* a kept read is kept whole */
	s->n_short += cls == 4;
	s->aberrant += cls == 3;
	s->drawn += cls == 2;
	return 0;
}

static char *norm_line(const void *state, char *p, uint64_t ord)
{
	const sdt_read_pick *r = ((const norm_state *)state)->rec + ord;
	p = sdt_put_dec(p, r->kmers, ' ');
	p = sdt_put_dec(p, r->median, ' ');
	p = sdt_put_dec(p, r->cov, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

static int norm_alive(const void *state, uint64_t ord) { return (((const norm_state *)state)->rec[ord].verdict & 7u) <= 1; }

/* `normalize`: the verdicts from the device, the kept batches back from HBM, the kept reads into the pairs file or the singles file */
static int run_normalize(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readPick", ".norm.pairs.fa", ".norm.single.fa"}, 4 * 11, 1, norm_note, norm_line, norm_alive, NULL, NULL};
	sdt_read_pick *pick = (sdt_read_pick *)records_alloc(reads, sizeof *pick, 0xFF);
	uint64_t got = 0, n_kept = 0;
	if (!pick || SDT_CALL(sdt_gpu_select_kept_reads, gpu, &opt->norm, pairs->v, pairs->n, pick, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	norm_state st = {pick, 0, 0, 0};
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	printf("%llu of %llu reads kept (%llu short, %llu aberrant, %llu dropped by draw)\n", t.kept, reads, st.n_short, st.aberrant, st.drawn);
	free(pick);
	return 0;
}

/* ---- dedup ----------------------------------------------------------------------------------------------------------------------------- */
typedef struct { const sdt_read_dup *rec; sdt_dup_levels lv; } dedup_state;

static int dedup_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	dedup_state *s = (dedup_state *)state;
	const sdt_read_dup *r = s->rec + ord;
	(void)read_len; (void)start; (void)len;                                  /* a kept read is kept whole */
	if (r->verdict > 1 || r->copies == 0 || r->first > ord) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %llu %u %u\n", (unsigned long long)ord + 1, (unsigned long long)r->first, r->copies, r->verdict);
		return -1;
	}
	/* (every ordinal has a read here, so the first read of a kept unit is the one whose ordinal is the unit's id) */
	if (sdt_dup_levels_note(&s->lv, r, r->verdict == 0 && r->first == ord) != 0) { fprintf(stderr, "sdt-kmers: out of memory\n"); return -1; }
	return 0;
}

static char *dedup_line(const void *state, char *p, uint64_t ord) { return sdt_put_dup_line(p, ((const dedup_state *)state)->rec + ord); }
static int dedup_alive(const void *state, uint64_t ord) { return ((const dedup_state *)state)->rec[ord].verdict == 0; }

/* `dedup`: the records from the device, the kept batches back from HBM, the kept reads into the pairs file or the singles file, the
 * table of duplication levels (dupsplit.c) */
static int run_dedup(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readDup", ".dedup.pairs.fa", ".dedup.single.fa"}, SDT_DUP_LINE_MAX, 1, dedup_note, dedup_line, dedup_alive, NULL, NULL};
	sdt_read_dup *dup = (sdt_read_dup *)records_alloc(reads, sizeof *dup, 0xFF);
	uint64_t got = 0, n_kept = 0;
	if (!dup || SDT_CALL(sdt_gpu_dedup_kept_reads, gpu, &opt->dedup, pairs->v, pairs->n, dup, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	dedup_state st;
	memset(&st, 0, sizeof st);
	st.rec = dup;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	char path[4200];
	outbuf olev;
	snprintf(path, sizeof path, "%s.dupLevels", opt->outname);
	if (ob_open(&olev, path) != 0) return 1;
	unsigned long long classes = 0;
	for (size_t i = 0; i < st.lv.n; i++) {
		ob_room(&olev, SDT_DUP_LEVEL_LINE_MAX);
		olev.p = sdt_put_dup_level_line(olev.p, st.lv.v + i);
		classes += st.lv.v[i].classes;
	}
	if (ob_close(&olev) != 0) return 1;
	printf("%llu of %llu reads kept in %llu classes\n", t.kept, reads, classes);
	sdt_dup_levels_free(&st.lv);
	free(dup);
	return 0;
}

/* ---- trim ------------------------------------------------------------------------------------------------------------------------------ */
typedef struct { edit_walk ed; const sdt_read_trim *rec; unsigned long long by_verdict[5]; } trim_state;

static int trim_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	trim_state *s = (trim_state *)state;
	const sdt_read_trim *t = s->rec + ord;
	if (t->verdict > 4 || (uint64_t)t->start + t->len > read_len) {
		fprintf(stderr, "sdt-kmers: the record of read %llu keeps [%u, %u + %u) of %llu bases, verdict %u\n", (unsigned long long)ord + 1, t->start,
		        t->start, t->len, (unsigned long long)read_len, t->verdict);
		return -1;
	}
	s->by_verdict[t->verdict]++;
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *trim_line(const void *state, char *p, uint64_t ord) { return sdt_put_trim_line(p, ((const trim_state *)state)->rec + ord); }
static int trim_alive(const void *state, uint64_t ord) { return ((const trim_state *)state)->rec[ord].len != 0; }

/* `trim`: the records (and with --correct the edits) from the device, the kept batches back from HBM, the edits applied here, the kept
 * bases of every read into the pairs file (both mates survive) or the singles file (trimsplit.c) */
static int run_trim(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	sdt_walk_stage stage = {{".readTrim", ".trim.pairs.fa", ".trim.single.fa"}, SDT_TRIM_LINE_MAX, 0, trim_note, trim_line, trim_alive, NULL, NULL};
	const int correct = (opt->trim.flags & SDT_TRIM_CORRECTED) != 0;
	opt->trim.min_count = (uint32_t)opt->min_count;
	sdt_read_trim *trim = (sdt_read_trim *)records_alloc(reads, sizeof *trim, 0);
	sdt_read_fix *fix = correct ? (sdt_read_fix *)records_alloc(reads, sizeof *fix, 0) : NULL;
	uint64_t got = 0, n_kept = 0;
	if (!trim || (correct && !fix) || SDT_CALL(sdt_gpu_trim_kept_reads, gpu, &opt->trim, trim, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "trimmed")) return 1;
	trim_state st;
	memset(&st, 0, sizeof st);
	st.rec = trim;
	if (correct && correct_kept(gpu, reads, opt->trim.min_count, fix, &st.ed.edits, &st.ed.n) != 0) return 1;
	sdt_walk_tally t;
	if (correct) {
		if (edits_open(&st.ed, opt->outname) != 0) return 1;
		stage.edit = edits_apply;
	}
	const int walked = fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) == 0;
	if (correct ? edits_close(&st.ed, walked) != 0 : !walked) return 1;
	printf("%llu reads: %llu whole, %llu gated, %llu trimmed, %llu dropped, %llu short; %llu bases in, %llu bases out\n", reads, st.by_verdict[0],
	       st.by_verdict[1], st.by_verdict[2], st.by_verdict[3], st.by_verdict[4], t.bases_in, t.bases_out);
	free(trim); free(fix);
	return 0;
}

/* ---- clip ------------------------------------------------------------------------------------------------------------------------------ */
typedef struct { const sdt_read_clip *rec; sdt_clip_stats stats; } clip_state;

static int clip_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	clip_state *s = (clip_state *)state;
	const sdt_read_clip *t = s->rec + ord;
	if (sdt_clip_stats_note(&s->stats, t, read_len) != 0) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->adapters, t->tail3,
		        t->tail5, t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *clip_line(const void *state, char *p, uint64_t ord) { return sdt_put_clip_line(p, ((const clip_state *)state)->rec + ord); }
static int clip_alive(const void *state, uint64_t ord) { return ((const clip_state *)state)->rec[ord].len != 0; }

/* `clip`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both mates
 * survive) or the singles file, routed as trim routes them; the statistics (clipsplit.c) */
static int run_clip(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readClip", ".clip.pairs.fa", ".clip.single.fa"}, SDT_CLIP_LINE_MAX, 0, clip_note, clip_line, clip_alive, NULL, NULL};
	sdt_read_clip *clip = (sdt_read_clip *)records_alloc(reads, sizeof *clip, 0);
	clip_state st = {clip, {0}};
	if (!clip) return 1;
	if (sdt_clip_stats_init(&st.stats, opt->ads.n) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	const sdt_adapter_set set = sdt_adapters_set(&opt->ads);
	uint64_t got = 0, n_kept = 0;
	if (SDT_CALL(sdt_gpu_clip_kept_reads, gpu, &opt->clip, &set, clip, reads, &got, &n_kept) || !all_reads_came_back(reads, got, "clipped")) return 1;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	char path[4200];
	FILE *fs = stats_open(path, opt->outname, ".clipStats");
	if (!fs || (sdt_clip_stats_write(fs, &st.stats, &opt->ads) != 0) | (fclose(fs) != 0)) return cannot_write(path);
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped; %llu bases in, %llu bases out\n", reads, (unsigned long long)st.stats.whole,
	       (unsigned long long)st.stats.clipped, (unsigned long long)st.stats.dropped, t.bases_in, t.bases_out);
	sdt_clip_stats_free(&st.stats);
	free(clip);
	return 0;
}

/* ---- overlap --------------------------------------------------------------------------------------------------------------------------- */
typedef struct {
	const sdt_read_overlap *rec;
	const sdt_pair_ranges *pairs;
	size_t cursor;                                                           /* into pairs, the note's own */
	uint64_t len_first;                                                      /* the first mate's bases, while the second is awaited */
	sdt_insert_hist hist;
	unsigned long long by_verdict[4];
} overlap_state;

static int overlap_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	overlap_state *s = (overlap_state *)state;
	const sdt_read_overlap *t = s->rec + ord;
	int ok = sdt_overlap_record_ok(t, read_len);
	if (ok && sdt_pair_ranges_holds(s->pairs, ord, &s->cursor)) {
		if (((ord - s->pairs->v[2 * s->cursor]) & 1) == 0) s->len_first = read_len;
		else {
			const int rc = sdt_insert_hist_note(&s->hist, t - 1, t, s->len_first, read_len);
			if (rc == -1) { fprintf(stderr, "sdt-kmers: out of memory\n"); return -1; }
			ok = rc == 0;
		}
	}
	if (!ok) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->overlap, t->mismatches,
		        t->insert, t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	s->by_verdict[t->verdict]++;
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *overlap_line(const void *state, char *p, uint64_t ord) { return sdt_put_overlap_line(p, ((const overlap_state *)state)->rec + ord); }
static int overlap_alive(const void *state, uint64_t ord) { return ((const overlap_state *)state)->rec[ord].len != 0; }

/* `overlap`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both mates
 * survive) or the singles file, routed as trim routes them; the histogram of the inserts (overlapsplit.c) */
static int run_overlap(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readOverlap", ".overlap.pairs.fa", ".overlap.single.fa"}, SDT_OVERLAP_LINE_MAX, 0,
	                                     overlap_note, overlap_line, overlap_alive, NULL, NULL};
	sdt_read_overlap *ov = (sdt_read_overlap *)records_alloc(reads, sizeof *ov, 0);
	uint64_t got = 0, n_kept = 0;
	if (!ov || SDT_CALL(sdt_gpu_overlap_kept_pairs, gpu, &opt->overlap, pairs->v, pairs->n, ov, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	overlap_state st;
	memset(&st, 0, sizeof st);
	st.rec = ov;
	st.pairs = pairs;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	const unsigned long long overlapping = st.hist.n, median = sdt_insert_hist_median(&st.hist);
	char path[4200];
	FILE *fh = stats_open(path, opt->outname, ".insertHist");
	if (!fh || (sdt_insert_hist_write(fh, &st.hist) != 0) | (fclose(fh) != 0)) return cannot_write(path);
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped; %llu bases in, %llu bases out; %llu pairs, %llu overlapping, median insert %llu\n", reads,
	       st.by_verdict[0], st.by_verdict[2], st.by_verdict[3], t.bases_in, t.bases_out, (unsigned long long)st.hist.pairs, overlapping, median);
	sdt_insert_hist_free(&st.hist);
	free(ov);
	return 0;
}

/* ---- merge ----------------------------------------------------------------------------------------------------------------------------- */
typedef struct {
	overlap_state ov;                                                        /* the overlap records, checked and counted as `overlap` does */
	const sdt_read_merge *rec;
	uint64_t first_ord;                                                      /* the first mate's ordinal, while the second is awaited */
	sdt_merge_stats stats;
} merge_state;

static int merge_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	merge_state *s = (merge_state *)state;
	const sdt_read_merge *t = s->rec + ord;
	uint64_t ov_start = 0, ov_len = read_len;
	if (overlap_note(&s->ov, ord, read_len, &ov_start, &ov_len) != 0) return -1;
	int ok = sdt_merge_record_ok(t, s->ov.rec + ord, read_len);
	/* (overlap_note has moved the cursor: the range that holds ord, if one does) */
	if (ok && sdt_pair_ranges_holds(s->ov.pairs, ord, &s->ov.cursor)) {
		if (((ord - s->ov.pairs->v[2 * s->ov.cursor]) & 1) == 0) s->first_ord = ord;
		else ok = sdt_merge_stats_note(&s->stats, s->rec + s->first_ord, t, s->ov.rec + s->first_ord, s->ov.rec + ord) == 0;
	} else if (ok) ok = t->merged == 0;                                      /* a single read is never merged */
	if (!ok) {
		fprintf(stderr, "sdt-kmers: the merge record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->merged, t->mismatches,
		        t->from_b, t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *merge_line(const void *state, char *p, uint64_t ord) { return sdt_put_merge_line(p, ((const merge_state *)state)->rec + ord); }
static int merge_alive(const void *state, uint64_t ord) { return ((const merge_state *)state)->rec[ord].len != 0; }

/* prefix.merge.fa: output read j of the merged stream under the name of the j-th merged pair's first mate; 0, or 1 after saying why */
static int merged_write(const char *prefix, const sdt_pair_ranges *pairs, const sdt_read_merge *mg, uint64_t reads, const uint32_t *words,
                        const uint64_t *offsets, uint64_t n_merged)
{
	static const char letters[4] = {'A', 'C', 'T', 'G'};
	char path[4200];
	outbuf o;
	snprintf(path, sizeof path, "%s.merge.fa", prefix);
	if (ob_open(&o, path) != 0) return 1;
	uint64_t j = 0;
	for (size_t r = 0; r < pairs->n && o.ok; r++)
		for (uint64_t ord = pairs->v[2 * r]; ord + 1 < pairs->v[2 * r + 1] && ord + 1 < reads && o.ok; ord += 2) {
			if (!mg[ord].merged) continue;
			if (j == n_merged || offsets[j + 1] - offsets[j] != mg[ord].merged) {
				fprintf(stderr, "sdt-kmers: the merged stream does not hold the %u bases of the pair at read %llu\n", mg[ord].merged, (unsigned long long)ord + 1);
				ob_close(&o);
				return 1;
			}
			ob_room(&o, 24);
			*o.p++ = '>';
			o.p = sdt_put_dec(o.p, ord + 1, '\n');
			for (uint64_t b = offsets[j]; b < offsets[j + 1] && o.ok;) {       /* (a fragment may be longer than a block) */
				const uint64_t n = offsets[j + 1] - b < 65536 ? offsets[j + 1] - b : 65536;
				ob_room(&o, (size_t)n + 1);
				for (uint64_t e = b + n; b < e; b++) *o.p++ = letters[(words[b >> 4] >> (30 - 2 * (int)(b & 15))) & 3u];
			}
			*o.p++ = '\n';
			j++;
		}
	if (ob_close(&o) != 0) return 1;
	if (j != n_merged) { fprintf(stderr, "sdt-kmers: %llu pairs merged, the records name %llu\n", (unsigned long long)n_merged, (unsigned long long)j); return 1; }
	return 0;
}

/* `merge`: the overlap records and then the merge records and the merged stream from the device, the kept batches back from HBM, the
 * kept bases of the reads that did not merge into the pairs file or the singles file as overlap routes them, the merged fragments
 * into a file of their own; the histogram of the inserts (overlapsplit.c), the statistics (mergesplit.c) */
static int run_merge(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readMerge", ".merge.pairs.fa", ".merge.single.fa"}, SDT_MERGE_LINE_MAX, 0, merge_note, merge_line, merge_alive, NULL, NULL};
	sdt_read_overlap *ov = (sdt_read_overlap *)records_alloc(reads, sizeof *ov, 0);
	sdt_read_merge *mg = (sdt_read_merge *)records_alloc(reads, sizeof *mg, 0);
	uint64_t got = 0, n_kept = 0, n_merged = 0, n_words = 0;
	if (!ov || !mg || SDT_CALL(sdt_gpu_overlap_kept_pairs, gpu, &opt->overlap, pairs->v, pairs->n, ov, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	/* only a pair with an overlap merges, into as many bases as its insert says: that bounds the merged stream */
	uint64_t cap_bases = 0, cap_reads = 0;
	for (size_t r = 0; r < pairs->n; r++)
		for (uint64_t ord = pairs->v[2 * r]; ord + 1 < pairs->v[2 * r + 1] && ord + 1 < reads; ord += 2)
			if (ov[ord].insert) { cap_bases += ov[ord].insert; cap_reads++; }
	const uint64_t cap_words = ((cap_bases + 15) >> 4) + 4;
	uint32_t *words = (uint32_t *)malloc(cap_words * sizeof(uint32_t));
	uint64_t *offsets = (uint64_t *)malloc((cap_reads + 1) * sizeof(uint64_t));
	if (!words || !offsets) { fprintf(stderr, "sdt-kmers: out of memory for %llu merged bases\n", (unsigned long long)cap_bases); return 1; }
	offsets[0] = 0;
	if (SDT_CALL(sdt_gpu_merge_kept_pairs, gpu, &opt->merge, pairs->v, pairs->n, ov, mg, reads, words, cap_words, offsets, cap_reads, &got, &n_merged, &n_words)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	n_kept = 0;
	for (unsigned long long i = 0; i < reads; i++) n_kept += mg[i].len != 0;
	merge_state st;
	memset(&st, 0, sizeof st);
	st.ov.rec = ov;
	st.ov.pairs = pairs;
	st.rec = mg;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	if (st.stats.merged != n_merged || st.stats.merged_bases != offsets[n_merged]) {
		fprintf(stderr, "sdt-kmers: the records say %llu pairs merged into %llu bases, the device %llu into %llu\n", (unsigned long long)st.stats.merged,
		        (unsigned long long)st.stats.merged_bases, (unsigned long long)n_merged, (unsigned long long)offsets[n_merged]);
		return 1;
	}
	if (merged_write(opt->outname, pairs, mg, reads, words, offsets, n_merged) != 0) return 1;
	char path[4200], summary[512];
	FILE *fh = stats_open(path, opt->outname, ".insertHist");
	if (!fh || (sdt_insert_hist_write(fh, &st.ov.hist) != 0) | (fclose(fh) != 0)) return cannot_write(path);
	sdt_merge_summary(summary, sizeof summary, &st.stats, reads, t.bases_in, t.bases_out);
	printf("%s\n", summary);
	sdt_insert_hist_free(&st.ov.hist);
	free(words); free(offsets); free(ov); free(mg);
	return 0;
}

/* ---- complexity ------------------------------------------------------------------------------------------------------------------------ */
typedef struct { const sdt_read_complexity *rec; sdt_score_hist hist; } cx_state;

static int cx_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	cx_state *s = (cx_state *)state;
	const sdt_read_complexity *t = s->rec + ord;
	if (sdt_score_hist_note(&s->hist, t, read_len) != 0) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->windows, t->low,
		        t->score, t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *cx_line(const void *state, char *p, uint64_t ord) { return sdt_put_cx_line(p, ((const cx_state *)state)->rec + ord); }
static int cx_alive(const void *state, uint64_t ord) { return ((const cx_state *)state)->rec[ord].len != 0; }

/* `complexity`: the records from the device, the kept batches back from HBM, the kept bases of every read into the pairs file (both
 * mates survive) or the singles file, routed as clip routes them; the histogram of the scores (cxsplit.c) */
static int run_complexity(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readComplexity", ".cx.pairs.fa", ".cx.single.fa"}, SDT_CX_LINE_MAX, 0, cx_note, cx_line, cx_alive, NULL, NULL};
	sdt_read_complexity *cx = (sdt_read_complexity *)records_alloc(reads, sizeof *cx, 0);
	uint64_t got = 0, n_kept = 0;
	if (!cx || SDT_CALL(sdt_gpu_complexity_kept_reads, gpu, &opt->cx, cx, reads, &got, &n_kept) || !all_reads_came_back(reads, got, "decided")) return 1;
	cx_state st;
	memset(&st, 0, sizeof st);
	st.rec = cx;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	char path[4200];
	FILE *fh = stats_open(path, opt->outname, ".scoreHist");
	if (!fh || (sdt_score_hist_write(fh, &st.hist) != 0) | (fclose(fh) != 0)) return cannot_write(path);
	printf("%llu reads: %llu with a low window, %llu clipped, %llu dropped; %llu bases in, %llu bases out\n", reads, (unsigned long long)st.hist.low,
	       (unsigned long long)st.hist.clipped, (unsigned long long)st.hist.dropped, t.bases_in, t.bases_out);
	free(cx);
	return 0;
}

/* ---- screen ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct { const sdt_read_screen *rec; const sdt_screen_params *prm; uint32_t k; sdt_screen_stats stats; } screen_state;

static int screen_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	screen_state *s = (screen_state *)state;
	const sdt_read_screen *t = s->rec + ord;
	if (sdt_screen_stats_note(&s->stats, t, read_len, s->k, s->prm) != 0) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->kmers, t->hits, t->ref,
		        t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	(void)start;                                                             /* (0 in every possible record) */
	*len = t->len;
	return 0;
}

static char *screen_line(const void *state, char *p, uint64_t ord) { return sdt_put_screen_line(p, ((const screen_state *)state)->rec + ord); }
/* (the device decides the mates of a pair together and says so in len, all or nothing: routed by it, as clip routes) */
static int screen_alive(const void *state, uint64_t ord) { return ((const screen_state *)state)->rec[ord].len != 0; }

/* `screen`: the references into the device's set, the records from the device, the kept batches back from HBM, every surviving read
 * into the pairs file (both mates of a pair) or the singles file, routed as clip routes them; the statistics (screensplit.c) */
static int run_screen(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readScreen", ".screen.pairs.fa", ".screen.single.fa"}, SDT_SCREEN_LINE_MAX, 0,
	                                     screen_note, screen_line, screen_alive, NULL, NULL};
	const sdt_ref_set *refs = &opt->refs;
	uint64_t distinct = 0;
	if (SDT_CALL(sdt_gpu_screen_load, gpu, refs->words, refs->nwords, refs->offsets, refs->nseqs, refs->ref_of_seq, refs->n_refs, opt->screen_k, &distinct)) return 1;
	sdt_read_screen *rec = (sdt_read_screen *)records_alloc(reads, sizeof *rec, 0);
	screen_state st = {rec, &opt->screen, opt->screen_k, {0}};
	if (!rec) return 1;
	if (sdt_screen_stats_init(&st.stats, refs->n_refs) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu records\n", reads); return 1; }
	uint64_t got = 0, n_kept = 0;
	if (SDT_CALL(sdt_gpu_screen_kept_reads, gpu, &opt->screen, pairs->v, pairs->n, rec, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "decided")) return 1;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, n_kept, &t) != 0) return 1;
	char path[4200];
	FILE *fs = stats_open(path, opt->outname, ".screenStats");
	if (!fs || (sdt_screen_stats_write(fs, &st.stats, refs) != 0) | (fclose(fs) != 0)) return cannot_write(path);
	printf("%llu reads against %llu k-mers of %u references: %llu matched, %llu kept, %llu dropped; %llu bases in, %llu bases out\n", reads,
	       (unsigned long long)distinct, refs->n_refs, (unsigned long long)st.stats.matched, (unsigned long long)st.stats.kept,
	       (unsigned long long)st.stats.dropped, t.bases_in, t.bases_out);
	sdt_screen_stats_free(&st.stats);
	free(rec);
	return 0;
}

/* ---- qtrim ----------------------------------------------------------------------------------------------------------------------------- */

/* while the reads stream: every FASTQ batch's qualities through sdt_gpu_quality_reads on a context of its own (nothing of the
 * asynchronous push path is touched), the records to the batch's ordinals; then the batch is pushed like any other */
struct qtrim_state {
	push_state push;
	sdt_ctx *qgpu;
	const sdt_quality_params *prm;
	sdt_read_quality *rec, *dense;                                           /* by ordinal; of one batch */
	uint64_t cap, dense_cap, n_kept;
	sdt_len_hist hist;                                                       /* after the stream */
};

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
		if (SDT_CALL(sdt_gpu_quality_reads, q->qgpu, b->quals, b->offsets[b->nreads], b->offsets, b->nreads, q->prm, q->dense, NULL, &kept)) return -1;
		q->n_kept += kept;
		for (uint64_t i = 0; i < b->nreads; i++) q->rec[ord_base + i * ord_stride] = q->dense[i];
	}
	return push_batch(&q->push, b, ord_base, ord_stride);
}

static int qtrim_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	qtrim_state *q = (qtrim_state *)state;
	const sdt_read_quality *t = q->rec + ord;
	const int noted = sdt_len_hist_note(&q->hist, t, read_len, q->prm);
	if (noted != 0) {
		if (noted == -1) fprintf(stderr, "sdt-kmers: out of memory for the histogram\n");
		else fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u of %llu bases\n", (unsigned long long)ord + 1, t->span, t->low,
		             t->ee_ppm, t->start, t->len, t->verdict, (unsigned long long)read_len);
		return -1;
	}
	*start = t->start;
	*len = t->len;
	return 0;
}

static char *qtrim_line(const void *state, char *p, uint64_t ord) { return sdt_put_qual_line(p, ((const qtrim_state *)state)->rec + ord); }
static int qtrim_alive(const void *state, uint64_t ord) { return ((const qtrim_state *)state)->rec[ord].len != 0; }

/* `qtrim`, after the stream: the kept batches back from HBM, the kept bases of every read into the pairs file (both mates survive) or
 * the singles file, routed as clip routes them; the histogram of the kept lengths (qualsplit.c) */
static int run_qtrim(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readQual", ".qtrim.pairs.fa", ".qtrim.single.fa"}, SDT_QUAL_LINE_MAX, 0, qtrim_note, qtrim_line, qtrim_alive, NULL, NULL};
	qtrim_state *q = opt->qtrim;
	if (reads > q->cap) { fprintf(stderr, "sdt-kmers: %llu reads streamed, records for %llu\n", reads, (unsigned long long)q->cap); return 1; }
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, q, q->n_kept, &t) != 0) return 1;
	const sdt_len_hist *h = &q->hist;
	char path[4200];
	FILE *fh = stats_open(path, opt->outname, ".lenHist");
	if (!fh || (sdt_len_hist_write(fh, h) != 0) | (fclose(fh) != 0)) return cannot_write(path);
	printf("%llu reads: %llu whole, %llu clipped, %llu dropped (%llu short, %llu low bases, %llu expected errors); %llu bases in, %llu bases out\n", reads,
	       (unsigned long long)h->whole, (unsigned long long)h->clipped, (unsigned long long)h->dropped, (unsigned long long)h->n_short,
	       (unsigned long long)h->n_low, (unsigned long long)h->n_errors, (unsigned long long)h->bases_in, (unsigned long long)h->bases_out);
	sdt_len_hist_free(&q->hist);
	return 0;
}

/* ---- qc ------------------------------------------------------------------------------------------------------------------------------ */

/* while the reads stream: every batch through sdt_gpu_qc_reads into the host report of its class.  A batch of a pair of files takes
 * every second ordinal (ord_stride 2), the first ordinal of a pair in the read-1 file: the rule by which sdt_pair_ranges_note makes
 * the pair ranges; every other batch holds single reads.  So the class bytes of a batch are all the same, and one call covers it */
typedef struct {
	sdt_ctx *gpu;
	sdt_qc_params prm;
	uint64_t words, reads;
	uint64_t *report[SDT_QC_CLASSES], with_quals[SDT_QC_CLASSES];
	uint8_t *classes;
	uint64_t classes_cap;
} qc_state;

static int qc_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	qc_state *q = (qc_state *)user;
	if (b->qual_faults) {
		fprintf(stderr, "sdt-kmers: %llu records of the batch at read %llu have a quality line that is not as long as their sequence line\n",
		        (unsigned long long)b->qual_faults, (unsigned long long)ord_base + 1);
		return -1;
	}
	q->reads += b->nreads;
	if (!b->nreads) return 0;
	const int k = ord_stride == 2 ? 1 + (b->stream_parity & 1) : 0;
	if (b->nreads > q->classes_cap) {
		free(q->classes);
		q->classes = (uint8_t *)malloc(b->nreads);
		q->classes_cap = q->classes ? b->nreads : 0;
	}
	if (!q->report[k]) q->report[k] = (uint64_t *)calloc(q->words, sizeof(uint64_t));
	if (!q->classes || !q->report[k]) { fprintf(stderr, "sdt-kmers: out of memory for the report\n"); return -1; }
	memset(q->classes, k, b->nreads);
	q->prm.class_sel = (uint32_t)k;
	if (SDT_CALL(sdt_gpu_qc_reads, q->gpu, b->words, b->nwords, b->quals, b->quals ? b->offsets[b->nreads] : 0, b->offsets, b->nreads, NULL, q->classes,
	             &q->prm, q->report[k], q->words)) return -1;
	if (b->quals) q->with_quals[k] += b->nreads;
	return 0;
}

/* `qc`: the libraries streamed once with their qualities, then the three files (qcsplit.c) and a line per class */
static int run_qc(options *opt, const sdt_cfg *cfg)
{
	static qc_state q;
	q.prm = opt->qc;
	q.words = sdt_gpu_qc_report_words(opt->qc.cycles);
	if (q.words != sdt_qc_words(opt->qc.cycles)) { fprintf(stderr, "sdt-kmers: the library's report has %llu words\n", (unsigned long long)q.words); return 1; }
	if (SDT_CALL(sdt_gpu_init, &q.gpu, opt->device, opt->K, 1, 0)) return 1;
	const int max_read_len = cfg->max_rd_len ? cfg->max_rd_len : 100;
	const size_t chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);
	const int parse_threads = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : opt->threads;
	sdt_read_quals(1);
	const int rc = sdt_stream_reads(cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, qc_batch, &q, NULL);
	sdt_read_quals(0);
	sdt_gpu_destroy(q.gpu);
	if (rc != 0) return 1;
	sdt_qc_class cls[SDT_QC_CLASSES];
	for (int k = 0; k < SDT_QC_CLASSES; k++) { cls[k].report = q.report[k]; cls[k].with_quals = q.with_quals[k]; }
	static int (*const writers[3])(FILE *, const sdt_qc_class *, uint32_t) = {sdt_qc_bases_write, sdt_qc_quals_write, sdt_qc_reads_write};
	static const char *const suffix[3] = {".qcBases", ".qcQuals", ".qcReads"};
	for (int i = 0; i < 3; i++) {
		char path[4200];
		FILE *f = stats_open(path, opt->outname, suffix[i]);
		if (!f || (writers[i](f, cls, opt->qc.cycles) != 0) | (fclose(f) != 0)) return cannot_write(path);
	}
	printf("%llu reads\n", (unsigned long long)q.reads);
	for (int k = 0; k < SDT_QC_CLASSES; k++) {
		char line[SDT_QC_LINE_MAX];
		if (!cls[k].report) continue;
		sdt_qc_summary(line, k, &cls[k], opt->qc.cycles);
		fputs(line, stdout);
		free(q.report[k]);
	}
	free(q.classes);
	return 0;
}

/* ---- profile and query ----------------------------------------------------------------------------------------------------------------- */

/* prefix.readCov: "kmers found solid min median max" per read */
static int run_profile(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)pairs;
	char path[4200];
	snprintf(path, sizeof path, "%s.readCov", opt->outname);
	sdt_read_cov *cov = (sdt_read_cov *)records_alloc(reads, sizeof *cov, 0);
	uint64_t got = 0;
	if (!cov || SDT_CALL(sdt_gpu_profile_kept_reads, gpu, (uint32_t)opt->min_count, cov, reads, &got) || !all_reads_came_back(reads, got, "profiled")) return 1;
	outbuf o;
	if (ob_open(&o, path) != 0) return 1;
	for (unsigned long long i = 0; i < reads && o.ok; i++) {
		ob_room(&o, 6 * 11);
		o.p = sdt_put_dec(o.p, cov[i].kmers, ' ');
		o.p = sdt_put_dec(o.p, cov[i].found, ' ');
		o.p = sdt_put_dec(o.p, cov[i].solid, ' ');
		o.p = sdt_put_dec(o.p, cov[i].min, ' ');
		o.p = sdt_put_dec(o.p, cov[i].median, ' ');
		o.p = sdt_put_dec(o.p, cov[i].max, '\n');
	}
	if (ob_close(&o) != 0) return 1;
	printf("%llu reads profiled into %s\n", reads, path);
	free(cov);
	return 0;
}

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

/* per line of the query file: kmer found strand count l_A l_C l_T l_G r_A r_C r_T r_G linear deleted */
static int run_query(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)reads; (void)pairs;
	const query_set *qs = &opt->qs;
	/* `linear` is thread_mark's flag (prlHashReads.c:911-967): marked on the table as it is now */
	int64_t hist[257];
	uint64_t linear = 0;
	if (SDT_CALL(sdt_gpu_mark_and_hist, gpu, hist, &linear)) return 1;
	const uint64_t n = qs->n, m = n ? n : 1;
	uint32_t *cnt = (uint32_t *)calloc(m, 4), *ll = (uint32_t *)calloc(m, 4), *rf = (uint32_t *)calloc(m, 4);
	uint8_t *stt = (uint8_t *)calloc(m, 1);
	if (!cnt || !ll || !rf || !stt) { fprintf(stderr, "sdt-kmers: out of memory\n"); return 1; }
	if (SDT_CALL(sdt_gpu_search_kmers, gpu, qs->keys, n, cnt, ll, rf, stt)) return 1;
	FILE *fo = opt->outname[0] ? fopen(opt->outname, "w") : stdout;
	if (!fo) return cannot_write(opt->outname);
	for (uint64_t i = 0; i < n; i++)
		fprintf(fo, "%s\t%d\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", qs->text[i], stt[i] & 1, (stt[i] & 2) ? '-' : '+', cnt[i],
		        ll[i] & 63u, (ll[i] >> 6) & 63u, (ll[i] >> 12) & 63u, (ll[i] >> 18) & 63u,
		        rf[i] & 63u, (rf[i] >> 6) & 63u, (rf[i] >> 12) & 63u, (rf[i] >> 18) & 63u, (rf[i] >> 24) & 1u, (rf[i] >> 25) & 1u);
	if (fo != stdout && fclose(fo) != 0) { fprintf(stderr, "sdt-kmers: write to %s failed\n", opt->outname); return 1; }
	free(cnt); free(ll); free(rf); free(stt);
	return 0;
}

/* ---- evaluate -------------------------------------------------------------------------------------------------------------------------- */

/* `evaluate`: the segments of the assembly against the counted table in one add, the spectrum, and the three outputs (asmsplit.c) */
static int run_evaluate(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)reads; (void)pairs;
	const sdt_ref_set *refs = &opt->refs;
	const sdt_asm_params prm = {(uint32_t)opt->min_count, opt->rows, 0, 0};
	sdt_seq_support *seg = (sdt_seq_support *)records_alloc(refs->nseqs, sizeof *seg, 0);
	sdt_asm_contig *ctg = (sdt_asm_contig *)records_alloc(refs->n_refs, sizeof *ctg, 0);
	uint64_t *matrix = (uint64_t *)records_alloc((unsigned long long)opt->rows * SDT_ASM_CN_COLS, sizeof *matrix, 0);
	uint64_t totals[4];
	if (!seg || !ctg || !matrix) return 1;
	if (SDT_CALL(sdt_gpu_asm_begin, gpu, &prm) || SDT_CALL(sdt_gpu_asm_add, gpu, refs->words, refs->nwords, refs->offsets, refs->nseqs, seg) ||
	    SDT_CALL(sdt_gpu_asm_spectrum, gpu, matrix, totals) || SDT_CALL(sdt_gpu_asm_end, gpu))
		return 1;
	sdt_asm_fold(refs, seg, ctg);
	sdt_asm_nodes nodes;
	if (sdt_asm_nodes_of(matrix, opt->rows, (uint32_t)opt->min_count, &nodes) != 0) { fprintf(stderr, "sdt-kmers: --rows %u does not exceed -c %lu\n", opt->rows, opt->min_count); return 1; }
	char path[4200], line[SDT_ASM_SUMMARY_MAX];
	FILE *fs = stats_open(path, opt->outname, ".asmSupport");
	if (!fs || (sdt_asm_support_write(fs, refs, ctg) != 0) | (fclose(fs) != 0)) return cannot_write(path);
	fs = stats_open(path, opt->outname, ".asmSpectrum");
	if (!fs || (sdt_asm_spectrum_write(fs, matrix, opt->rows) != 0) | (fclose(fs) != 0)) return cannot_write(path);
	sdt_asm_summary(line, totals, &nodes, opt->K);
	fputs(line, stdout);
	free(seg); free(ctg); free(matrix);
	return 0;
}

/* ---- compare --------------------------------------------------------------------------------------------------------------------------- */

/* `compare`: two counted tables, A and B; the matrix with its totals, the selection where asked for, and the outputs (cmpsplit.c) */
static int run_compare(sdt_ctx *a, sdt_ctx *b, const options *opt)
{
	const sdt_cmp_params prm = {opt->rows, opt->cols, 0, 0};
	uint64_t *matrix = (uint64_t *)records_alloc((unsigned long long)opt->rows * opt->cols, sizeof *matrix, 0);
	uint64_t totals[8];
	if (!matrix) return 1;
	if (SDT_CALL(sdt_gpu_compare_tables, a, b, &prm, matrix, totals)) return 1;
	sdt_cmp_solid solid;
	if (sdt_cmp_solid_of(matrix, opt->rows, opt->cols, (uint32_t)opt->min_count, &solid) != 0) {
		fprintf(stderr, "sdt-kmers: --rows %u and --cols %u must exceed -c %lu\n", opt->rows, opt->cols, opt->min_count);
		return 1;
	}
	char path[4200], line[SDT_CMP_SUMMARY_MAX];
	FILE *fs = stats_open(path, opt->outname, ".cmpMatrix");
	if (!fs || (sdt_cmp_matrix_write(fs, matrix, opt->rows, opt->cols) != 0) | (fclose(fs) != 0)) return cannot_write(path);
	if (opt->select_given) {
		const sdt_cmp_range rg = {opt->select[0], opt->select[1], opt->select[2], opt->select[3]};
		uint64_t matched = 0, got = 0;
		if (SDT_CALL(sdt_gpu_compare_select, a, b, &rg, NULL, NULL, NULL, 0, &matched)) return 1;
		const uint64_t cap = matched < opt->max_list ? matched : opt->max_list;
		const int nw = sdt_gpu_key_words(a);
		uint64_t *keys = (uint64_t *)records_alloc(cap * (unsigned long long)nw, sizeof *keys, 0);
		uint32_t *ca = (uint32_t *)records_alloc(cap, sizeof *ca, 0), *cb = (uint32_t *)records_alloc(cap, sizeof *cb, 0);
		if (!keys || !ca || !cb) return 1;
		if (cap && SDT_CALL(sdt_gpu_compare_select, a, b, &rg, keys, ca, cb, cap, &got)) return 1;
		if (cap && got != matched) { fprintf(stderr, "sdt-kmers: %llu k-mers matched, then %llu\n", (unsigned long long)matched, (unsigned long long)got); return 1; }
		fs = stats_open(path, opt->outname, ".cmpKmers");
		if (!fs || (sdt_cmp_kmers_write(fs, keys, ca, cb, cap, nw, opt->K, matched) != 0) | (fclose(fs) != 0)) return cannot_write(path);
		free(keys); free(ca); free(cb);
	}
	sdt_cmp_summary(line, totals, &solid);
	fputs(line, stdout);
	free(matrix);
	return 0;
}

/* ---- cluster ----------------------------------------------------------------------------------------------------------------------------- */
typedef struct { const sdt_read_cluster *rec; sdt_cluster_tally tally; const uint32_t *pick; } cluster_state;

static int cluster_note(void *state, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	cluster_state *s = (cluster_state *)state;
	const sdt_read_cluster *r = s->rec + ord;
	(void)start; (void)len;                                                  /* a read is written whole */
	if (sdt_cluster_tally_note(&s->tally, r, read_len) != 0) {
		fprintf(stderr, "sdt-kmers: the record of read %llu is %u %u %u %u %u %u\n", (unsigned long long)ord + 1, r->kmers, r->live, r->split, r->cluster, r->unit, r->verdict);
		return -1;
	}
	return 0;
}

static char *cluster_line(const void *state, char *p, uint64_t ord) { return sdt_put_cluster_line(p, ((const cluster_state *)state)->rec + ord); }
static char *cluster_name(const void *state, char *p, uint64_t ord) { return sdt_put_cluster_name_tail(p, ((const cluster_state *)state)->rec + ord); }
static int cluster_alive(const void *state, uint64_t ord)
{
	const cluster_state *s = (const cluster_state *)state;
	return !s->pick || sdt_cluster_picked(s->rec + ord, s->pick);
}

/* `cluster`: the clustering on the device, the records of the kept reads, the component list; the kept batches back from HBM, every
 * read (with --pick: of the picked units) into the pairs file or the singles file; the cluster list with the reads of each */
static int run_cluster(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	static const sdt_walk_stage stage = {{".readCluster", ".cluster.pairs.fa", ".cluster.single.fa"}, SDT_CLUSTER_LINE_MAX, 1, cluster_note, cluster_line,
	                                     cluster_alive, NULL, cluster_name};
	uint64_t info[8], got = 0, n_kept = 0, n_comp = 0;
	opt->cluster.min_count = (uint32_t)opt->min_count;
	if (SDT_CALL(sdt_gpu_cluster_begin, gpu, &opt->cluster, info)) return 1;
	sdt_read_cluster *rec = (sdt_read_cluster *)records_alloc(reads, sizeof *rec, 0xFF);
	if (!rec || SDT_CALL(sdt_gpu_cluster_kept_reads, gpu, pairs->v, pairs->n, opt->pick[0], opt->pick[1], rec, reads, &got, &n_kept)) return 1;
	if (!all_reads_came_back(reads, got, "clustered")) return 1;
	const int nw = sdt_gpu_key_words(gpu);
	uint64_t *keys = (uint64_t *)malloc((info[2] ? info[2] : 1) * (size_t)nw * sizeof(uint64_t));
	sdt_cluster_comp *comp = (sdt_cluster_comp *)malloc((info[2] ? info[2] : 1) * sizeof *comp);
	cluster_state st = {rec, {0}, opt->pick_given ? opt->pick : NULL};
	if (!keys || !comp || sdt_cluster_tally_init(&st.tally, info[2]) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu clusters\n", (unsigned long long)info[2]); return 1; }
	if (SDT_CALL(sdt_gpu_cluster_components, gpu, keys, comp, info[2], &n_comp)) return 1;
	if (SDT_CALL(sdt_gpu_cluster_end, gpu)) return 1;
	sdt_walk_tally t;
	if (fetch_and_walk(gpu, reads, pairs, opt->outname, &stage, &st, opt->pick_given ? n_kept : reads, &t) != 0) return 1;
	char path[4200], line[SDT_CLUSTER_SUMMARY_MAX];
	FILE *f = stats_open(path, opt->outname, ".clusters");
	if (!f) return cannot_write(path);
	const int bad = sdt_cluster_list_write(f, keys, comp, nw, opt->K, info, &st.tally) != 0;
	if ((fclose(f) != 0) | bad) { fprintf(stderr, "sdt-kmers: write to %s failed\n", path); return 1; }
	sdt_cluster_summary(line, info, &st.tally);
	fputs(line, stdout);
	sdt_cluster_tally_free(&st.tally);
	free(keys); free(comp); free(rec);
	return 0;
}

/* ---- bubbles ----------------------------------------------------------------------------------------------------------------------------- */
/* `bubbles`: the list on the device, then fetched and written a piece at a time with the paths of that piece (bubblesplit.c) */
static int run_bubbles(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)reads; (void)pairs;
	enum { PIECE = 1 << 16 };
	const sdt_bubble_params prm = {(uint32_t)opt->min_count, opt->cluster.max_count, opt->cluster.min_link, opt->max_branch, 0, 0};
	uint64_t info[8], kinds[3] = {0, 0, 0}, cap = 0;
	if (SDT_CALL(sdt_gpu_bubbles_begin, gpu, &prm, info)) return 1;
	const int nw = sdt_gpu_key_words(gpu);
	uint64_t *keys = (uint64_t *)malloc((size_t)PIECE * 2 * (size_t)nw * sizeof *keys), *offs = (uint64_t *)malloc((2 * (size_t)PIECE + 1) * sizeof *offs);
	sdt_bubble *rec = (sdt_bubble *)malloc((size_t)PIECE * sizeof *rec);
	uint8_t *bases = NULL;
	if (!keys || !offs || !rec) { fprintf(stderr, "sdt-kmers: out of memory for the bubbles\n"); return 1; }
	char path[4200], fa_path[4200], line[SDT_BUBBLE_SUMMARY_MAX];
	FILE *f = stats_open(path, opt->outname, ".bubbles");
	if (!f) return cannot_write(path);
	FILE *fa = stats_open(fa_path, opt->outname, ".bubbles.fa");
	if (!fa) return cannot_write(fa_path);
	for (uint64_t first = 0; first < info[4]; first += PIECE) {
		const uint64_t n = info[4] - first < PIECE ? info[4] - first : PIECE;
		if (SDT_CALL(sdt_gpu_bubbles_fetch, gpu, first, n, keys, rec) || SDT_CALL(sdt_gpu_bubbles_paths, gpu, first, n, NULL, 0, offs)) return 1;
		if (offs[2 * n] > cap) {
			free(bases);
			cap = offs[2 * n];
			if (!(bases = (uint8_t *)malloc(cap))) { fprintf(stderr, "sdt-kmers: out of memory for %llu bases of paths\n", (unsigned long long)cap); return 1; }
		}
		if (SDT_CALL(sdt_gpu_bubbles_paths, gpu, first, n, bases, cap, offs)) return 1;
		if (sdt_bubble_list_write(f, keys, rec, first, n, nw, opt->K, kinds) != 0) return cannot_write(path);
		if (sdt_bubble_fasta_write(fa, keys, rec, bases, offs, first, n, nw, opt->K) != 0) return cannot_write(fa_path);
	}
	if (fclose(f) != 0) return cannot_write(path);
	if (fclose(fa) != 0) return cannot_write(fa_path);
	if (SDT_CALL(sdt_gpu_bubbles_end, gpu)) return 1;
	sdt_bubble_summary(line, info, kinds);
	fputs(line, stdout);
	free(keys); free(offs); free(rec); free(bases);
	return 0;
}

/* ---- unitigs ----------------------------------------------------------------------------------------------------------------------------- */
/* `unitigs`: the list on the device, then fetched and written a piece at a time with the sequences of that piece, then the links of
 * every piece behind the S lines (unitigsplit.c) */
/* sdt_gpu_unitigs_begin and the three files; the list stays open, line: the summary */
static int unitigs_files(sdt_ctx *gpu, options *opt, uint64_t info[8], char line[SDT_UNITIG_SUMMARY_MAX])
{
	enum { PIECE = 1 << 16 };
	const sdt_unitig_params prm = {(uint32_t)opt->min_count, opt->cluster.max_count, opt->cluster.min_link, 0};
	uint64_t cap = 0, link_cap = 0;
	if (SDT_CALL(sdt_gpu_unitigs_begin, gpu, &prm, info)) return 1;
	const int nw = sdt_gpu_key_words(gpu);
	uint64_t *keys = (uint64_t *)malloc((size_t)PIECE * 2 * (size_t)nw * sizeof *keys), *offs = (uint64_t *)malloc(((size_t)PIECE + 1) * sizeof *offs);
	sdt_unitig *rec = (sdt_unitig *)malloc((size_t)PIECE * sizeof *rec);
	sdt_unitig_tally tally = {0, 0, 0, 0, (uint32_t *)malloc((size_t)(info[2] ? info[2] : 1) * sizeof(uint32_t))};
	uint8_t *bases = NULL;
	sdt_unitig_link *links = NULL;
	if (!keys || !offs || !rec || !tally.nodes) { fprintf(stderr, "sdt-kmers: out of memory for the unitigs\n"); return 1; }
	char path[4200], fa_path[4200], gfa_path[4200];
	FILE *f = stats_open(path, opt->outname, ".unitigs");
	if (!f) return cannot_write(path);
	FILE *fa = stats_open(fa_path, opt->outname, ".unitigs.fa");
	if (!fa) return cannot_write(fa_path);
	FILE *gfa = stats_open(gfa_path, opt->outname, ".unitigs.gfa");
	if (!gfa || sdt_unitig_gfa_header(gfa) != 0) return cannot_write(gfa_path);
	for (uint64_t first = 0; first < info[2]; first += PIECE) {
		const uint64_t n = info[2] - first < PIECE ? info[2] - first : PIECE;
		if (SDT_CALL(sdt_gpu_unitigs_fetch, gpu, first, n, keys, rec) || SDT_CALL(sdt_gpu_unitigs_seqs, gpu, first, n, NULL, 0, offs)) return 1;
		if (offs[n] > cap) {
			free(bases);
			cap = offs[n];
			if (!(bases = (uint8_t *)malloc(cap))) { fprintf(stderr, "sdt-kmers: out of memory for %llu bases of unitigs\n", (unsigned long long)cap); return 1; }
		}
		if (SDT_CALL(sdt_gpu_unitigs_seqs, gpu, first, n, bases, cap, offs)) return 1;
		if (sdt_unitig_list_write(f, keys, rec, first, n, nw, opt->K, &tally) != 0) return cannot_write(path);
		if (sdt_unitig_fasta_write(fa, rec, bases, offs, first, n) != 0) return cannot_write(fa_path);
		if (sdt_unitig_gfa_segments(gfa, rec, bases, offs, first, n) != 0) return cannot_write(gfa_path);
	}
	for (uint64_t first = 0; first < info[2]; first += PIECE) {
		const uint64_t n = info[2] - first < PIECE ? info[2] - first : PIECE;
		uint64_t n_links = 0, n_dangling = 0;
		if (SDT_CALL(sdt_gpu_unitigs_links, gpu, first, n, NULL, 0, &n_links, &n_dangling)) return 1;
		if (n_links > link_cap) {
			free(links);
			link_cap = n_links;
			if (!(links = (sdt_unitig_link *)malloc((size_t)link_cap * sizeof *links))) { fprintf(stderr, "sdt-kmers: out of memory for %llu links\n", (unsigned long long)link_cap); return 1; }
		}
		if (n_links && SDT_CALL(sdt_gpu_unitigs_links, gpu, first, n, links, link_cap, &n_links, &n_dangling)) return 1;
		if (sdt_unitig_gfa_links(gfa, links, n_links, opt->K, &tally) != 0) return cannot_write(gfa_path);
	}
	if (fclose(f) != 0) return cannot_write(path);
	if (fclose(fa) != 0) return cannot_write(fa_path);
	if (fclose(gfa) != 0) return cannot_write(gfa_path);
	sdt_unitig_summary(line, info, &tally, opt->K);
	free(keys); free(offs); free(rec); free(bases); free(links); free(tally.nodes);
	return 0;
}

static int run_unitigs(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)reads; (void)pairs;
	uint64_t info[8];
	char line[SDT_UNITIG_SUMMARY_MAX];
	if (unitigs_files(gpu, opt, info, line) != 0 || SDT_CALL(sdt_gpu_unitigs_end, gpu)) return 1;
	fputs(line, stdout);
	return 0;
}

/* ---- thread ------------------------------------------------------------------------------------------------------------------------------ */
/* `thread`: the unitig list and its files as `unitigs` writes them, the index, then the libraries once more through
 * sdt_gpu_unitigs_reads, batch by batch as they are parsed: the records by read ordinal, the segments in the order the batches came
 * with every read's place among them; then one walk over the ordinals writes the lines (threadsplit.c) */
typedef struct {
	sdt_ctx *gpu;
	uint64_t reads;                                                          /* the ordinals: what pass 1 streamed */
	sdt_read_path *rec;                                                      /* by ordinal; kmers 0xFFFFFFFF: no read */
	uint64_t *seg_at;                                                        /* by ordinal: its first segment in segs */
	sdt_path_seg *segs;
	uint64_t n_segs, cap_segs, seen;
	sdt_read_path *b_rec;                                                    /* of one batch */
	uint64_t *b_offs, b_cap;
} thread_state;

static int thread_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	thread_state *st = (thread_state *)user;
	if (!b->nreads) return 0;
	if (ord_base + (b->nreads - 1) * ord_stride >= st->reads) {
		fprintf(stderr, "sdt-kmers: the second pass over the libraries holds read %llu, the first held %llu reads\n",
		        (unsigned long long)(ord_base + (b->nreads - 1) * ord_stride) + 1, (unsigned long long)st->reads);
		return -1;
	}
	if (b->nreads > st->b_cap) {
		free(st->b_rec); free(st->b_offs);
		st->b_cap = b->nreads;
		st->b_rec = (sdt_read_path *)malloc((size_t)st->b_cap * sizeof *st->b_rec);
		st->b_offs = (uint64_t *)malloc(((size_t)st->b_cap + 1) * sizeof *st->b_offs);
		if (!st->b_rec || !st->b_offs) { fprintf(stderr, "sdt-kmers: out of memory for the paths of %llu reads\n", (unsigned long long)b->nreads); return -1; }
	}
	uint64_t n = 0;
	/* into the room behind the segments so far; where that is too small the call says how many there are, and runs once more */
	int rc = sdt_gpu_unitigs_reads(st->gpu, b->words, b->nwords, b->offsets, b->nreads, st->b_rec, st->b_offs, st->segs ? st->segs + st->n_segs : NULL,
	                               st->segs ? st->cap_segs - st->n_segs : 0, &n);
	if (rc == SDT_EFULL || (rc == SDT_OK && !st->segs && n)) {
		const uint64_t cap = 2 * (st->n_segs + n);
		sdt_path_seg *more = (sdt_path_seg *)realloc(st->segs, (size_t)cap * sizeof *more);
		if (!more) { fprintf(stderr, "sdt-kmers: out of memory for %llu path segments\n", (unsigned long long)cap); return -1; }
		st->segs = more;
		st->cap_segs = cap;
		rc = sdt_gpu_unitigs_reads(st->gpu, b->words, b->nwords, b->offsets, b->nreads, st->b_rec, st->b_offs, st->segs + st->n_segs, st->cap_segs - st->n_segs, &n);
	}
	if (rc != SDT_OK) { gpu_fail("sdt_gpu_unitigs_reads"); return -1; }
	for (uint64_t i = 0; i < b->nreads; i++) {
		const uint64_t ord = ord_base + i * ord_stride;
		st->rec[ord] = st->b_rec[i];
		st->seg_at[ord] = st->n_segs + st->b_offs[i];
	}
	st->n_segs += n;
	st->seen += b->nreads;
	return 0;
}

static int run_thread(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)pairs;
	uint64_t info[8], iinfo[4];
	char uline[SDT_UNITIG_SUMMARY_MAX], line[SDT_THREAD_SUMMARY_MAX], path[4200];
	if (unitigs_files(gpu, opt, info, uline) != 0 || SDT_CALL(sdt_gpu_unitigs_index, gpu, iinfo)) return 1;
	thread_state st = {gpu, reads, (sdt_read_path *)records_alloc(reads, sizeof(sdt_read_path), 0xFF), (uint64_t *)records_alloc(reads, sizeof(uint64_t), 0),
	                   NULL, 0, 0, 0, NULL, NULL, 0};
	sdt_thread_tally tally;
	if (!st.rec || !st.seg_at) return 1;
	if (sdt_thread_tally_init(&tally, info[2]) != 0) { fprintf(stderr, "sdt-kmers: out of memory for %llu unitigs\n", (unsigned long long)info[2]); return 1; }
	const sdt_cfg *cfg = opt->cfg;
	const int max_read_len = cfg->max_rd_len ? cfg->max_rd_len : 100;
	const size_t chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);
	const int parse_threads = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : opt->threads;
	if (sdt_stream_reads(cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, thread_batch, &st, NULL) != 0) return 1;
	if (!all_reads_came_back(reads, st.seen, "threaded")) return 1;
	if (SDT_CALL(sdt_gpu_unitigs_end, gpu)) return 1;
	FILE *f = stats_open(path, opt->outname, ".readPaths");
	if (!f) return cannot_write(path);
	for (uint64_t ord = 0; ord < reads; ord++) {
		if (st.rec[ord].kmers == 0xFFFFFFFFu) continue;                      /* (an ordinal that no read has) */
		const int rc = sdt_thread_read_write(f, st.rec + ord, st.segs ? st.segs + st.seg_at[ord] : NULL, &tally);
		if (rc == -2) { fprintf(stderr, "sdt-kmers: the path of read %llu does not add up\n", (unsigned long long)ord + 1); return 1; }
		if (rc != 0) return cannot_write(path);
	}
	if (fclose(f) != 0) return cannot_write(path);
	f = stats_open(path, opt->outname, ".unitigReads");
	if (!f || (sdt_thread_unitig_reads_write(f, &tally) != 0) | (fclose(f) != 0)) return cannot_write(path);
	sdt_thread_summary(line, &tally);
	fputs(line, stdout);
	sdt_thread_tally_free(&tally);
	free(st.rec); free(st.seg_at); free(st.segs); free(st.b_rec); free(st.b_offs);
	return 0;
}

/* ---- support ----------------------------------------------------------------------------------------------------------------------------- */
/* `support`: the unitig list and its files as `unitigs` writes them, the index, a cleared tally, then the libraries once more through
 * sdt_gpu_unitigs_support_add, batch by batch as they are parsed; then the tallies are fetched a piece at a time and written
 * (supportsplit.c).  Nothing per read or per segment comes to the host */
typedef struct { sdt_ctx *gpu; uint64_t seen; } support_state;

static int support_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	support_state *st = (support_state *)user;
	(void)ord_base; (void)ord_stride;
	if (!b->nreads) return 0;
	/* (single reads: the mates of two files are in different batches) */
	if (sdt_gpu_unitigs_support_add(st->gpu, b->words, b->nwords, b->offsets, b->nreads, 0) != SDT_OK) { gpu_fail("sdt_gpu_unitigs_support_add"); return -1; }
	st->seen += b->nreads;
	return 0;
}

static int run_support(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs)
{
	(void)pairs;
	enum { PIECE = 1 << 16 };
	uint64_t info[8], iinfo[4], totals[12], nj = 0, link_cap = 0;
	char uline[SDT_UNITIG_SUMMARY_MAX], line[SDT_SUPPORT_SUMMARY_MAX], path[4200];
	const sdt_support_params prm = {opt->max_junctions, 0, 0, 0};           /* (no mate links: see support_batch) */
	if (unitigs_files(gpu, opt, info, uline) != 0 || SDT_CALL(sdt_gpu_unitigs_index, gpu, iinfo) || SDT_CALL(sdt_gpu_unitigs_support_begin, gpu, &prm)) return 1;
	support_state st = {gpu, 0};
	const sdt_cfg *cfg = opt->cfg;
	const int max_read_len = cfg->max_rd_len ? cfg->max_rd_len : 100;
	const size_t chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);
	const int parse_threads = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : opt->threads;
	if (sdt_stream_reads(cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, support_batch, &st, NULL) != 0) return 1;
	if (!all_reads_came_back(reads, st.seen, "tallied")) return 1;
	sdt_unitig *rec = (sdt_unitig *)malloc((size_t)PIECE * sizeof *rec);
	sdt_unitig_support *us = (sdt_unitig_support *)malloc((size_t)PIECE * sizeof *us);
	sdt_unitig_link *links = NULL;
	sdt_link_support *ls = NULL;
	if (!rec || !us) { fprintf(stderr, "sdt-kmers: out of memory for the tallies\n"); return 1; }
	FILE *f = stats_open(path, opt->outname, ".unitigSupport");
	if (!f) return cannot_write(path);
	for (uint64_t first = 0; first < info[2]; first += PIECE) {
		const uint64_t n = info[2] - first < PIECE ? info[2] - first : PIECE;
		if (SDT_CALL(sdt_gpu_unitigs_fetch, gpu, first, n, NULL, rec) || SDT_CALL(sdt_gpu_unitigs_support_unitigs, gpu, first, n, us)) return 1;
		if (sdt_support_unitigs_write(f, rec, us, first, n) != 0) return cannot_write(path);
	}
	if (fclose(f) != 0) return cannot_write(path);
	f = stats_open(path, opt->outname, ".linkSupport");
	if (!f) return cannot_write(path);
	for (uint64_t first = 0; first < info[2]; first += PIECE) {
		const uint64_t n = info[2] - first < PIECE ? info[2] - first : PIECE;
		uint64_t n_links = 0;
		if (SDT_CALL(sdt_gpu_unitigs_links, gpu, first, n, NULL, 0, &n_links, NULL)) return 1;
		if (n_links > link_cap) {
			free(links); free(ls);
			link_cap = n_links;
			links = (sdt_unitig_link *)malloc((size_t)link_cap * sizeof *links);
			ls = (sdt_link_support *)malloc((size_t)link_cap * sizeof *ls);
			if (!links || !ls) { fprintf(stderr, "sdt-kmers: out of memory for %llu links\n", (unsigned long long)link_cap); return 1; }
		}
		if (!n_links) continue;
		if (SDT_CALL(sdt_gpu_unitigs_links, gpu, first, n, links, link_cap, &n_links, NULL) || SDT_CALL(sdt_gpu_unitigs_support_links, gpu, first, n, ls, link_cap, &n_links))
			return 1;
		if (sdt_support_links_write(f, links, ls, n_links) != 0) return cannot_write(path);
	}
	if (fclose(f) != 0) return cannot_write(path);
	/* the junctions; a set that is not kept (a capacity of 0) leaves an empty file */
	sdt_unitig_junction *jn = NULL;
	if (opt->max_junctions) {
		if (SDT_CALL(sdt_gpu_unitigs_support_junctions, gpu, NULL, 0, &nj)) return 1;
		if (!(jn = (sdt_unitig_junction *)malloc((size_t)(nj ? nj : 1) * sizeof *jn))) { fprintf(stderr, "sdt-kmers: out of memory for %llu junctions\n", (unsigned long long)nj); return 1; }
		if (SDT_CALL(sdt_gpu_unitigs_support_junctions, gpu, jn, nj, &nj)) return 1;
	}
	f = stats_open(path, opt->outname, ".junctions");
	if (!f || (sdt_support_junctions_write(f, jn, nj) != 0) | (fclose(f) != 0)) return cannot_write(path);
	if (SDT_CALL(sdt_gpu_unitigs_support_totals, gpu, totals) || SDT_CALL(sdt_gpu_unitigs_support_end, gpu) || SDT_CALL(sdt_gpu_unitigs_end, gpu)) return 1;
	sdt_support_summary(line, totals, nj);
	fputs(line, stdout);
	free(rec); free(us); free(links); free(ls); free(jn);
	return 0;
}

/* ---- the command line ------------------------------------------------------------------------------------------------------------------ */
enum { PROFILE, QUERY, CORRECT, NORMALIZE, TRIM, DEDUP, CLIP, OVERLAP, COMPLEXITY, QTRIM, SCREEN, MERGE, QC, EVALUATE, COMPARE, CLUSTER, BUBBLES, UNITIGS, THREAD, SUPPORT, N_SUBCOMMANDS };

static const struct {
	const char *name;
	int keep_reads, pairs;                  /* SDT_FLAG_KEEP_READS; the pair ranges are noted while the reads stream */
	unsigned long min_count;                /* where -c is not given */
	int (*run)(sdt_ctx *gpu, unsigned long long reads, options *opt, const sdt_pair_ranges *pairs);      /* after the count is finished */
} subcommands[N_SUBCOMMANDS] = {
	[PROFILE] = {"profile", 1, 0, 0, run_profile},       [QUERY] = {"query", 0, 0, 0, run_query},
	[CORRECT] = {"correct", 1, 0, 2, run_correct},       [NORMALIZE] = {"normalize", 1, 1, 0, run_normalize},
	[TRIM] = {"trim", 1, 1, 2, run_trim},                [DEDUP] = {"dedup", 1, 1, 0, run_dedup},
	[CLIP] = {"clip", 1, 1, 0, run_clip},                [OVERLAP] = {"overlap", 1, 1, 0, run_overlap},
	[COMPLEXITY] = {"complexity", 1, 1, 0, run_complexity}, [QTRIM] = {"qtrim", 1, 1, 0, run_qtrim},
	[SCREEN] = {"screen", 1, 1, 0, run_screen},             [MERGE] = {"merge", 1, 1, 0, run_merge},
	[QC] = {"qc", 0, 0, 0, NULL},                           /* (streams on its own and counts nothing: run_qc, from main) */
	[EVALUATE] = {"evaluate", 0, 0, 2, run_evaluate},
	[COMPARE] = {"compare", 0, 0, 2, NULL},                 /* (counts two sets of libraries into two contexts: run_compare, from main) */
	[CLUSTER] = {"cluster", 1, 1, 2, run_cluster},
	[BUBBLES] = {"bubbles", 0, 0, 2, run_bubbles},
	[UNITIGS] = {"unitigs", 0, 0, 2, run_unitigs},
	[THREAD] = {"thread", 0, 0, 2, run_thread},            /* (streams the libraries a second time on its own: no read is kept) */
	[SUPPORT] = {"support", 0, 0, 2, run_support},         /* (the same) */
};

enum { O_MAX_K = 1000, O_DEVICE, O_TARGET, O_MAX_CV, O_SEED, O_MIN_COV, O_MIN_LEN, O_CORRECT, O_MATE_SWAP, O_TAIL3, O_TAIL5, O_MIN_OVERLAP, O_ERROR_PCT,
       O_MIN_TAIL, O_TAIL_ERROR_PCT, O_MAX_ERR, O_MAX_SCORE, O_MAX_LOW, O_TRIM_LOW, O_PHRED, O_CUT_Q, O_LOW_Q, O_MAX_LOW_BASES, O_MAX_EE, O_SCREEN_K,
       O_MIN_HITS, O_MIN_HIT_PCT, O_KEEP_MATCHED, O_MIN_MERGED, O_MAX_MERGED, O_CYCLES, O_FROM_END, O_ASSEMBLY, O_ROWS, O_AGAINST, O_COLS, O_SELECT, O_MAX_LIST, O_MAX_COUNT, O_MIN_LINK, O_PICK, O_MAX_BRANCH, O_MAX_JUNCTIONS };

/* the options that belong to some subcommands only: the name as it is printed, who may be given it, what the refusal says after
 * "belongs to" (kept, not derived: --min-overlap names clip alone), and the most its value may be where it takes a whole number */
#define BIT(sub) (1u << (sub))
static const struct { int code; const char *name; unsigned owners; const char *belongs; unsigned long long most; } owned_options[] = {
	{O_TARGET, "--target", BIT(NORMALIZE), "normalize", UINT32_MAX}, {O_MAX_CV, "--max-cv", BIT(NORMALIZE), "normalize", UINT32_MAX},
	{O_SEED, "--seed", BIT(NORMALIZE), "normalize", UINT64_MAX},
	{O_MIN_COV, "--min-cov", BIT(TRIM), "trim", UINT32_MAX}, {O_CORRECT, "--correct", BIT(TRIM), "trim", 0},
	{O_MIN_LEN, "--min-len", BIT(TRIM) | BIT(CLIP) | BIT(OVERLAP) | BIT(COMPLEXITY) | BIT(QTRIM) | BIT(MERGE), "trim, clip, overlap, complexity and qtrim", UINT32_MAX},
	{'a', "-a", BIT(CLIP), "clip", 0}, {'g', "-g", BIT(CLIP), "clip", 0}, {O_TAIL3, "--tail3", BIT(CLIP), "clip", 0}, {O_TAIL5, "--tail5", BIT(CLIP), "clip", 0},
	{O_ERROR_PCT, "--error-pct", BIT(CLIP), "clip", 100}, {O_MIN_TAIL, "--min-tail", BIT(CLIP), "clip", UINT32_MAX},
	{O_TAIL_ERROR_PCT, "--tail-error-pct", BIT(CLIP), "clip", 100}, {O_MIN_OVERLAP, "--min-overlap", BIT(CLIP) | BIT(OVERLAP) | BIT(MERGE), "clip", UINT32_MAX},
	{O_MAX_ERR, "--max-err", BIT(OVERLAP) | BIT(MERGE), "overlap", 100},
	{O_MAX_SCORE, "--max-score", BIT(COMPLEXITY), "complexity", 100}, {O_MAX_LOW, "--max-low", BIT(COMPLEXITY), "complexity", 100},
	{O_TRIM_LOW, "--trim-low", BIT(COMPLEXITY), "complexity", 0},
	{O_PHRED, "--phred", BIT(QTRIM) | BIT(QC), "qtrim", 64}, {O_CUT_Q, "--cut-q", BIT(QTRIM), "qtrim", 93}, {O_LOW_Q, "--low-q", BIT(QTRIM), "qtrim", 93},
	{O_MAX_LOW_BASES, "--max-low-bases", BIT(QTRIM), "qtrim", 100}, {O_MAX_EE, "--max-ee", BIT(QTRIM), "qtrim", UINT32_MAX},
	{'r', "-r", BIT(SCREEN), "screen", 0}, {O_SCREEN_K, "--screen-k", BIT(SCREEN), "screen", 31}, {O_MIN_HITS, "--min-hits", BIT(SCREEN), "screen", UINT32_MAX},
	{O_MIN_HIT_PCT, "--min-hit-pct", BIT(SCREEN), "screen", 100}, {O_KEEP_MATCHED, "--keep-matched", BIT(SCREEN), "screen", 0},
	{O_MATE_SWAP, "--mate-swap", BIT(DEDUP), "dedup", 0},
	{O_MIN_MERGED, "--min-merged", BIT(MERGE), "merge", UINT32_MAX}, {O_MAX_MERGED, "--max-merged", BIT(MERGE), "merge", UINT32_MAX},
	{O_CYCLES, "--cycles", BIT(QC), "qc", SDT_QC_MAX_CYCLES}, {O_FROM_END, "--from-end", BIT(QC), "qc", 0},
	{O_ASSEMBLY, "--assembly", BIT(EVALUATE), "evaluate", 0}, {O_ROWS, "--rows", BIT(EVALUATE) | BIT(COMPARE), "evaluate", SDT_CMP_MAX_CELLS / 2},
	{O_AGAINST, "--against", BIT(COMPARE), "compare", 0}, {O_COLS, "--cols", BIT(COMPARE), "compare", SDT_CMP_MAX_CELLS / 2},
	{O_SELECT, "--select", BIT(COMPARE), "compare", 0}, {O_MAX_LIST, "--max-list", BIT(COMPARE), "compare", 1ULL << 31},
	{O_MAX_COUNT, "--max-count", BIT(CLUSTER) | BIT(BUBBLES) | BIT(UNITIGS) | BIT(THREAD) | BIT(SUPPORT), "cluster", UINT32_MAX},
	{O_MIN_LINK, "--min-link", BIT(CLUSTER) | BIT(BUBBLES) | BIT(UNITIGS) | BIT(THREAD) | BIT(SUPPORT), "cluster", 63},
	{O_PICK, "--pick", BIT(CLUSTER), "cluster", 0}, {O_MAX_BRANCH, "--max-branch", BIT(BUBBLES), "bubbles", SDT_BUBBLE_MAX_LEN},
	{O_MAX_JUNCTIONS, "--max-junctions", BIT(SUPPORT), "support", 1ULL << 36},
};

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

/* the options of subcommand `sub` into opt (the defaults are in it); 0, or the exit code after saying why */
static int parse_options(int argc, char **argv, int sub, options *opt)
{
	static struct option longopts[] = {{"max-k", required_argument, 0, O_MAX_K}, {"device", required_argument, 0, O_DEVICE},
	                                   {"target", required_argument, 0, O_TARGET}, {"max-cv", required_argument, 0, O_MAX_CV},
	                                   {"seed", required_argument, 0, O_SEED}, {"min-cov", required_argument, 0, O_MIN_COV},
	                                   {"min-len", required_argument, 0, O_MIN_LEN}, {"correct", no_argument, 0, O_CORRECT},
	                                   {"mate-swap", no_argument, 0, O_MATE_SWAP}, {"tail3", required_argument, 0, O_TAIL3},
	                                   {"tail5", required_argument, 0, O_TAIL5}, {"min-overlap", required_argument, 0, O_MIN_OVERLAP},
	                                   {"error-pct", required_argument, 0, O_ERROR_PCT}, {"min-tail", required_argument, 0, O_MIN_TAIL},
	                                   {"tail-error-pct", required_argument, 0, O_TAIL_ERROR_PCT}, {"max-err", required_argument, 0, O_MAX_ERR},
	                                   {"max-score", required_argument, 0, O_MAX_SCORE}, {"max-low", required_argument, 0, O_MAX_LOW},
	                                   {"trim-low", no_argument, 0, O_TRIM_LOW}, {"phred", required_argument, 0, O_PHRED},
	                                   {"cut-q", required_argument, 0, O_CUT_Q}, {"low-q", required_argument, 0, O_LOW_Q},
	                                   {"max-low-bases", required_argument, 0, O_MAX_LOW_BASES}, {"max-ee", required_argument, 0, O_MAX_EE},
	                                   {"screen-k", required_argument, 0, O_SCREEN_K}, {"min-hits", required_argument, 0, O_MIN_HITS},
	                                   {"min-hit-pct", required_argument, 0, O_MIN_HIT_PCT}, {"keep-matched", no_argument, 0, O_KEEP_MATCHED},
	                                   {"min-merged", required_argument, 0, O_MIN_MERGED}, {"max-merged", required_argument, 0, O_MAX_MERGED},
	                                   {"cycles", required_argument, 0, O_CYCLES}, {"from-end", no_argument, 0, O_FROM_END},
	                                   {"assembly", required_argument, 0, O_ASSEMBLY}, {"rows", required_argument, 0, O_ROWS},
	                                   {"against", required_argument, 0, O_AGAINST}, {"cols", required_argument, 0, O_COLS},
	                                   {"select", required_argument, 0, O_SELECT}, {"max-list", required_argument, 0, O_MAX_LIST},
	                                   {"max-count", required_argument, 0, O_MAX_COUNT}, {"min-link", required_argument, 0, O_MIN_LINK},
	                                   {"pick", required_argument, 0, O_PICK}, {"max-branch", required_argument, 0, O_MAX_BRANCH}, {"max-junctions", required_argument, 0, O_MAX_JUNCTIONS},
	                                   {0, 0, 0, 0}};
	int c;
	while ((c = getopt_long(argc, argv, "s:K:p:d:c:o:q:a:g:r:", longopts, NULL)) != -1) {
		const char *name = NULL;
		unsigned long long most = 0, v = 0;
		for (size_t i = 0; i < sizeof owned_options / sizeof owned_options[0] && !name; i++) {
			if (owned_options[i].code != c) continue;
			name = owned_options[i].name;
			most = owned_options[i].most;
			if (!(owned_options[i].owners & BIT(sub))) { fprintf(stderr, "sdt-kmers: %s belongs to %s\n", name, owned_options[i].belongs); usage(); return 255; }
		}
		if (most && parse_number(name, optarg, most, &v) != 0) return 255;
		switch (c) {
		case 's': snprintf(opt->cfgfile, sizeof opt->cfgfile, "%s", optarg); break;
		case 'o': snprintf(opt->outname, sizeof opt->outname, "%s", optarg); break;
		case 'q': snprintf(opt->qfile, sizeof opt->qfile, "%s", optarg); break;
		case 'K': opt->K = atoi(optarg); break;
		case 'p': opt->threads = atoi(optarg) > 0 ? atoi(optarg) : 1; break;
		case 'd': opt->d = atoi(optarg) >= 0 ? atoi(optarg) : 0; break;      /* pregraph.c:159 */
		case 'c': opt->min_count = strtoul(optarg, NULL, 10); break;
		case O_MAX_K: opt->max_k = atoi(optarg); break;
		case O_DEVICE: opt->device = atoi(optarg); break;
		case O_TARGET: opt->norm.target = (uint32_t)v; break;
		case O_MAX_CV: opt->norm.max_cv_pct = (uint32_t)v; break;
		case O_SEED: opt->norm.seed = v; break;
		case O_MIN_COV: opt->trim.min_cov = (uint32_t)v; break;
		case O_MIN_LEN: opt->trim.min_len = opt->clip.min_len = opt->overlap.min_len = opt->cx.min_len = opt->qual.min_len = (uint32_t)v; break;
		case O_CORRECT: opt->trim.flags |= SDT_TRIM_CORRECTED; break;
		case O_MATE_SWAP: opt->dedup.flags |= SDT_DEDUP_MATE_SWAP; break;
		case 'a': case 'g': snprintf(opt->afile[c == 'g'], sizeof opt->afile[0], "%s", optarg); break;
		case O_TAIL3: case O_TAIL5: {
			const int mask = tail_mask(name, optarg);
			if (mask < 0) return 255;
			if (c == O_TAIL3) opt->clip.tail3_bases = (uint32_t)mask; else opt->clip.tail5_bases = (uint32_t)mask;
			break;
		}
		case O_MIN_OVERLAP: case O_MIN_TAIL:
			if (v == 0) { fprintf(stderr, "sdt-kmers: %s must be at least 1\n", name); return 255; }
			if (c == O_MIN_OVERLAP) opt->clip.min_overlap = opt->overlap.min_overlap = (uint32_t)v; else opt->clip.min_tail = (uint32_t)v;
			break;
		case O_ERROR_PCT: opt->clip.max_err_pct = (uint32_t)v; break;
		case O_TAIL_ERROR_PCT: opt->clip.tail_err_pct = (uint32_t)v; break;
		case O_MAX_ERR: opt->overlap.max_err_pct = (uint32_t)v; break;
		case O_MAX_SCORE:
			if (v == 0) { fprintf(stderr, "sdt-kmers: --max-score must be at least 1: at 0 every window would be low\n"); return 255; }
			opt->cx.max_score_pct = (uint32_t)v;
			break;
		case O_MAX_LOW: opt->cx.max_low_pct = (uint32_t)v; opt->max_low_given = 1; break;
		case O_TRIM_LOW: opt->cx.flags |= SDT_COMPLEXITY_TRIM; break;
		case O_PHRED:
			if (v != 33 && v != 64) { fprintf(stderr, "sdt-kmers: --phred %llu: 33 or 64\n", v); return 255; }
			opt->qual.phred_offset = opt->qc.phred_offset = (uint32_t)v;
			break;
		case O_CUT_Q: opt->qual.cut_q = (uint32_t)v; break;
		case O_LOW_Q: opt->qual.low_q = (uint32_t)v; break;
		case O_MAX_LOW_BASES: opt->qual.max_low_pct = (uint32_t)v; break;
		case O_MAX_EE: opt->qual.max_ee_ppm = (uint32_t)v; break;
		case 'r':
			if (opt->n_rfiles == MAX_REF_FILES) { fprintf(stderr, "sdt-kmers: more than %d -r files\n", MAX_REF_FILES); return 255; }
			opt->rfile[opt->n_rfiles++] = optarg;
			break;
		case O_SCREEN_K:
			if (v < 11) { fprintf(stderr, "sdt-kmers: --screen-k %llu: 11 to 31\n", v); return 255; }
			opt->screen_k = (uint32_t)v;
			break;
		case O_MIN_HITS: opt->screen.min_hits = (uint32_t)v; break;
		case O_MIN_HIT_PCT: opt->screen.min_hit_pct = (uint32_t)v; break;
		case O_KEEP_MATCHED: opt->screen.flags |= SDT_SCREEN_KEEP_MATCHED; break;
		case O_MIN_MERGED: opt->merge.min_len = (uint32_t)v; break;
		case O_MAX_MERGED: opt->merge.max_len = (uint32_t)v; break;
		case O_CYCLES:
			if (v == 0) { fprintf(stderr, "sdt-kmers: --cycles must be at least 1\n"); return 255; }
			opt->qc.cycles = (uint32_t)v;
			break;
		case O_FROM_END: opt->qc.flags |= SDT_QC_FROM_END; break;
		case O_ASSEMBLY:
			if (opt->n_asmfiles == MAX_REF_FILES) { fprintf(stderr, "sdt-kmers: more than %d --assembly files\n", MAX_REF_FILES); return 255; }
			opt->asmfile[opt->n_asmfiles++] = optarg;
			break;
		case O_ROWS:
			if (v < 2 || (sub == EVALUATE && v > SDT_ASM_MAX_ROWS)) {
				fprintf(stderr, "sdt-kmers: --rows %llu: 2 to %d\n", v, sub == EVALUATE ? SDT_ASM_MAX_ROWS : SDT_CMP_MAX_CELLS / 2);
				return 255;
			}
			opt->rows = (uint32_t)v;
			break;
		case O_AGAINST: snprintf(opt->againstfile, sizeof opt->againstfile, "%s", optarg); break;
		case O_COLS:
			if (v < 2) { fprintf(stderr, "sdt-kmers: --cols %llu: 2 to %d\n", v, SDT_CMP_MAX_CELLS / 2); return 255; }
			opt->cols = (uint32_t)v;
			break;
		case O_SELECT:
			if (sdt_cmp_parse_select(optarg, opt->select) != 0) {
				fprintf(stderr, "sdt-kmers: --select %s: MINA:MAXA:MINB:MAXB is expected, four whole numbers below 2^32 with MINA <= MAXA and MINB <= MAXB\n", optarg);
				return 255;
			}
			opt->select_given = 1;
			break;
		case O_MAX_LIST: opt->max_list = v; break;
		case O_MAX_COUNT: opt->cluster.max_count = (uint32_t)v; break;
		case O_MIN_LINK:
			if (v == 0) { fprintf(stderr, "sdt-kmers: --min-link must be at least 1\n"); return 255; }
			opt->cluster.min_link = (uint32_t)v;
			break;
		case O_PICK:
			if (sdt_cluster_parse_pick(optarg, opt->pick) != 0) {
				fprintf(stderr, "sdt-kmers: --pick %s: LO:HI is expected, two cluster ids from 1 with LO <= HI\n", optarg);
				return 255;
			}
			opt->pick_given = 1;
			break;
		case O_MAX_BRANCH:
			if (v == 0) { fprintf(stderr, "sdt-kmers: --max-branch must be at least 1\n"); return 255; }
			opt->max_branch = (uint32_t)v;
			break;
		case O_MAX_JUNCTIONS: opt->max_junctions = v; break;
		default: usage(); return 255;
		}
	}
	if (!opt->cfgfile[0] || (sub == QUERY ? !opt->qfile[0] : !opt->outname[0])) { usage(); return 255; }
	if (sub == SCREEN && opt->n_rfiles == 0) { fprintf(stderr, "sdt-kmers: screen needs a reference file: -r refs.fa\n"); usage(); return 255; }
	if (sub == EVALUATE && opt->n_asmfiles == 0) { fprintf(stderr, "sdt-kmers: evaluate needs an assembly: --assembly contigs.fa\n"); usage(); return 255; }
	if (sub == EVALUATE && opt->rows <= opt->min_count) {
		fprintf(stderr, "sdt-kmers: --rows %u must exceed -c %lu: the last row takes every larger count, and the solid nodes are summed from the rows\n", opt->rows,
		        opt->min_count);
		return 255;
	}
	if (sub == COMPARE && !opt->againstfile[0]) { fprintf(stderr, "sdt-kmers: compare needs a second library config: --against b.cfg\n"); usage(); return 255; }
	if (sub == COMPARE && (unsigned long long)opt->rows * opt->cols > SDT_CMP_MAX_CELLS) {
		fprintf(stderr, "sdt-kmers: --rows %u x --cols %u = %llu cells: %d at most\n", opt->rows, opt->cols, (unsigned long long)opt->rows * opt->cols, SDT_CMP_MAX_CELLS);
		return 255;
	}
	if (sub == COMPARE && (opt->rows <= opt->min_count || opt->cols <= opt->min_count)) {
		fprintf(stderr, "sdt-kmers: --rows %u and --cols %u must exceed -c %lu: the last row and column take every larger count, and the solid k-mers are summed from them\n",
		        opt->rows, opt->cols, opt->min_count);
		return 255;
	}
	if (sub == MERGE && opt->merge.max_len != 0 && opt->merge.max_len < (opt->merge.min_len > 1 ? opt->merge.min_len : 1u)) {
		fprintf(stderr, "sdt-kmers: --max-merged %u is below --min-merged %u: no pair could merge (0: no limit)\n", opt->merge.max_len, opt->merge.min_len);
		return 255;
	}
	if ((sub == CLUSTER || sub == BUBBLES || sub == UNITIGS || sub == THREAD || sub == SUPPORT) && opt->cluster.max_count != 0 && opt->cluster.max_count < (opt->min_count > 1 ? opt->min_count : 1ul)) {
		fprintf(stderr, "sdt-kmers: --max-count %u is below -c %lu: no node could be live (0: no limit)\n", opt->cluster.max_count, opt->min_count);
		return 255;
	}
	if (sub == NORMALIZE && opt->norm.target == 0) { fprintf(stderr, "sdt-kmers: --target must be at least 1\n"); return 255; }
	if (opt->cx.flags & SDT_COMPLEXITY_TRIM) {
		if (opt->max_low_given && opt->cx.max_low_pct != 0) {
			fprintf(stderr, "sdt-kmers: --max-low %u with --trim-low: the longest clean stretch is kept, whatever fraction is low; give --max-low 0 or none\n",
			        opt->cx.max_low_pct);
			return 255;
		}
		opt->cx.max_low_pct = 0;
	}
	if (opt->max_k == 0) opt->max_k = opt->K <= 31 ? 31 : SDT_MAX_K;
	if (opt->d > 127) opt->d = (signed char)opt->d;                          /* deLowKmer is a char */
	/* pregraph.c:38-59 */
	if (opt->K % 2 == 0) { opt->K++; printf("K should be an odd number\n"); }
	if (opt->K < 13) { opt->K = 13; printf("K should not be less than 13\n"); }
	else if (opt->K > opt->max_k) opt->K = opt->max_k;
	return 0;
}

/* what the options name is read and checked before the device is touched: the adapter files (the 3' file first), the reference files
 * in the order given, the query file, the library config, and for qtrim that every library is FASTQ.  0, or the exit code */
static int load_inputs(int sub, options *opt, sdt_cfg *cfg)
{
	char err[4400];
	for (int e = 0; e < 2; e++)
		if (opt->afile[e][0] && sdt_adapters_load(&opt->ads, opt->afile[e], e, err, sizeof err) != 0) { fprintf(stderr, "sdt-kmers: %s\n", err); return 2; }
	for (uint32_t i = 0; i < opt->ads.n; i++)
		if (opt->ads.offsets[i + 1] - opt->ads.offsets[i] < opt->clip.min_overlap) {
			fprintf(stderr, "sdt-kmers: adapter %s has %llu bases, fewer than --min-overlap %u\n", opt->ads.names[i],
			        (unsigned long long)(opt->ads.offsets[i + 1] - opt->ads.offsets[i]), opt->clip.min_overlap);
			return 2;
		}
	for (int i = 0; i < opt->n_rfiles; i++)
		if (sdt_refs_load(&opt->refs, opt->rfile[i], err, sizeof err) != 0) { fprintf(stderr, "sdt-kmers: %s\n", err); return 2; }
	if (sub == SCREEN) {
		const sdt_ref_set *refs = &opt->refs;
		if (sdt_refs_pack(&opt->refs) != 0) { fprintf(stderr, "sdt-kmers: out of memory for the references\n"); return 2; }
		uint64_t positions = 0;
		for (uint64_t i = 0; i < refs->nseqs; i++)
			if (refs->offsets[i + 1] - refs->offsets[i] >= opt->screen_k) positions += refs->offsets[i + 1] - refs->offsets[i] - opt->screen_k + 1;
		if (positions == 0) { fprintf(stderr, "sdt-kmers: the references hold no stretch of %u letters ACGT: no k-mer to screen against\n", opt->screen_k); return 2; }
	}
	for (int i = 0; i < opt->n_asmfiles; i++)
		if (sdt_refs_load(&opt->refs, opt->asmfile[i], err, sizeof err) != 0) { fprintf(stderr, "sdt-kmers: %s\n", err); return 2; }
	if (sub == EVALUATE) {
		const sdt_ref_set *refs = &opt->refs;
		if (sdt_refs_pack(&opt->refs) != 0) { fprintf(stderr, "sdt-kmers: out of memory for the assembly\n"); return 2; }
		uint64_t longest = 0;
		for (uint64_t i = 0; i < refs->nseqs; i++)
			if (refs->offsets[i + 1] - refs->offsets[i] > longest) longest = refs->offsets[i + 1] - refs->offsets[i];
		if (longest < (uint64_t)opt->K) { fprintf(stderr, "sdt-kmers: the assembly holds no stretch of %d letters ACGT: no k-mer to score\n", opt->K); return 255; }
	}
	if (sub == QUERY) {
		const int rq = load_queries(opt->qfile, opt->K, opt->K <= 31 ? 1 : (opt->K <= 63 ? 2 : 4), &opt->qs);
		if (rq != 0) return rq;
	}
	if (sdt_cfg_load(opt->cfgfile, cfg) != 0) return 255;
	if (sub == COMPARE && sdt_cfg_load(opt->againstfile, &opt->against) != 0) return 255;
	/* qtrim: every read needs its qualities; refused before the device is touched and before anything is written */
	for (int i = 0; i < cfg->nlibs && sub == QTRIM; i++) {
		const sdt_lib *l = &cfg->libs[i];
		const char *fasta = l->nf ? l->f[0] : (l->nf1 ? l->f1[0] : (l->nf2 ? l->f2[0] : (l->np ? l->p[0] : (l->nb ? l->b[0] : NULL))));
		if (fasta) { fprintf(stderr, "sdt-kmers: qtrim needs base qualities: %s is not a FASTQ file (q1= / q2= / q=)\n", fasta); return 2; }
	}
	return 0;
}

/* the libraries through pass 1 (qtrim: every batch's qualities judged on the way); 0 with *reads, or 1 after the context was
 * destroyed or what failed was said.  says: in front of the lines it prints.  May be called again for another context (compare): the
 * parser pool is enabled and disabled per call, and the ring of pushes in flight, which a call that failed leaves as it was, starts
 * empty */
static int stream_and_count(sdt_ctx *gpu, int sub, options *opt, const sdt_cfg *cfg, sdt_pair_ranges *pairs, qtrim_state *qst, unsigned long long *reads,
                            const char *says)
{
	g_inflight.head = g_inflight.n = 0;
	const int max_read_len = cfg->max_rd_len ? cfg->max_rd_len : 100;       /* prlHashReads.c:361-364 */
	push_state st = {gpu, 0, subcommands[sub].pairs ? pairs : NULL};
	if (sub == QTRIM) {
		if (SDT_CALL(sdt_gpu_init, &qst->qgpu, opt->device, opt->K, 1, 0)) return 1;
		qst->push = st;
		qst->prm = &opt->qual;
		sdt_read_quals(1);
	}
	const size_t chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);
	const int parse_threads = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : opt->threads;
	sdt_pool_enable(sdt_gpu_host_alloc, sdt_gpu_host_free, parse_threads + PUSH_DEPTH + 8);
	int rc = sub == QTRIM ? sdt_stream_reads(cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, qtrim_batch, qst, NULL)
	                      : sdt_stream_reads(cfg, max_read_len, parse_threads > 0 ? parse_threads : 1, chunk, 0, push_batch, &st, NULL);
	if (sub == QTRIM) {
		st.reads = qst->push.reads;
		sdt_read_quals(0);
		sdt_gpu_destroy(qst->qgpu);
	}
	if (rc == 0 && inflight_retire(gpu, 0) != 0) rc = -1;
	sdt_pool_disable();
	if (rc != 0) { sdt_gpu_destroy(gpu); return 1; }
	uint64_t kmers = 0, nodes = 0, removed = 0;
	if (SDT_CALL(sdt_gpu_finish_count, gpu, &kmers, &nodes)) return 1;
	printf("%s%llu reads, %llu nodes allocated, %llu kmer in reads\n", says, st.reads, (unsigned long long)nodes, (unsigned long long)kmers);
	if (opt->d && SDT_CALL(sdt_gpu_delow, gpu, opt->d, &removed)) return 1;
	if (opt->d) printf("%s%llu kmer removed\n", says, (unsigned long long)removed);
	*reads = st.reads;
	return 0;
}

int main(int argc, char **argv)
{
	int sub = 0;
	while (sub < N_SUBCOMMANDS && (argc < 2 || strcmp(argv[1], subcommands[sub].name) != 0)) sub++;
	if (sub == N_SUBCOMMANDS) { usage(); return 255; }
	static options opt = {.K = 23, .threads = 8,
	                      .norm = {50, 10000, 0}, .clip = {5, 10, 0, 10, 20, 0, 0, 0}, .overlap = {30, 10, 0, 0}, .cx = {10, 50, 0, 0},
	                      .qual = {33, 20, 15, 40, 0, 0, 0, 0}, .screen = {1, 0, 0, 0}, .merge = {0, 0, 33, 0},
	                      .qc = {1024, 33, 0, 0, 0}, .screen_k = 31, .rows = 256, .cols = 64, .max_list = 1000000,
	                      .cluster = {2, 0, 1, 0}, .pick = {0, 0xFFFFFFFEu}, .max_branch = 1000, .max_junctions = 1u << 22};                                   /* bbduk's usual figure: a choice, not a measurement */
	opt.min_count = subcommands[sub].min_count;
	if (sub == COMPARE) opt.rows = 64;
	sdt_cfg cfg;
	int rc = parse_options(argc - 1, argv + 1, sub, &opt);
	if (rc == 0) rc = load_inputs(sub, &opt, &cfg);
	if (rc != 0) return rc;
	if (sub == QC) {
		rc = run_qc(&opt, &cfg);
		sdt_cfg_free(&cfg);
		return rc;
	}

	sdt_ctx *gpu = NULL;
	if (SDT_CALL(sdt_gpu_init, &gpu, opt.device, opt.K, 0, subcommands[sub].keep_reads ? SDT_FLAG_KEEP_READS : 0u)) return 1;
	sdt_pair_ranges pairs;
	memset(&pairs, 0, sizeof pairs);
	static qtrim_state qst;
	opt.qtrim = &qst;
	opt.cfg = &cfg;
	unsigned long long reads = 0;
	if (sub == COMPARE) {
		/* A is counted and drained before B's libraries stream; both contexts then live side by side on the device */
		sdt_ctx *gpu_b = NULL;
		if (stream_and_count(gpu, sub, &opt, &cfg, &pairs, &qst, &reads, "A: ") != 0) return 1;
		if (SDT_CALL(sdt_gpu_init, &gpu_b, opt.device, opt.K, 0, 0u)) { sdt_gpu_destroy(gpu); return 1; }
		if (stream_and_count(gpu_b, sub, &opt, &opt.against, &pairs, &qst, &reads, "B: ") != 0) { sdt_gpu_destroy(gpu); return 1; }
		rc = run_compare(gpu, gpu_b, &opt);
		sdt_gpu_destroy(gpu_b);
		sdt_gpu_destroy(gpu);
		sdt_cfg_free(&opt.against);
		sdt_cfg_free(&cfg);
		return rc;
	}
	if (stream_and_count(gpu, sub, &opt, &cfg, &pairs, &qst, &reads, "") != 0) return 1;
	if (subcommands[sub].run(gpu, reads, &opt, &pairs) != 0) return 1;
	sdt_pair_ranges_free(&pairs);
	sdt_adapters_free(&opt.ads);
	sdt_refs_free(&opt.refs);
	free(qst.rec); free(qst.dense);
	sdt_gpu_destroy(gpu);
	sdt_cfg_free(&cfg);
	return 0;
}
