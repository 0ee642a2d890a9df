/*
 * sdt_gpu.h -- C ABI of libsdt_gpu.so: the MI355X (gfx950) implementation of SOAPdenovo-Trans's
 * `pregraph` hashing path (read chopping -> canonical k-mer -> hash insert/count -> -d filter ->
 * linear marking + k-mer frequency histogram -> node export).
 *
 * The reference has no FFI layer: the path sits behind the C functions that call_pregraph() calls
 * (inc/extfunc.h:82,156-163) with state in globals.  Each entry point below names the reference
 * function / call site it replaces (paths relative to /root/reference/src).  A host written in C
 * (soapdenovo-trans_amd/csrc/host/sdt_pregraph.c), Python/ctypes (soapdenovo-trans_amd/__init__.py)
 * or the reference's own prlHashReads.c binds exactly these symbols.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative SDT_E* code and
 * leaves a message retrievable by sdt_gpu_last_error(); no exceptions cross the boundary; one host
 * thread per context; a context owns one GPU.  There is NO CPU fallback: without a usable gfx950
 * device sdt_gpu_init fails with SDT_ENODEV.
 *
 * Packed reads ("2-bit stream"): all reads of a batch concatenated, 2 bits per base with the
 * reference's coding A=0 C=1 T=2 G=3 (inc/def.h:39-42), 16 bases per little-endian uint32 word, FIRST
 * base in the MOST significant bit pair (so a k-mer is a funnel shift of consecutive words and equals
 * the reference's Kmer value, inc/def.h:45-59).  read i occupies bases [offsets[i], offsets[i+1]).
 * The word array must be readable for 4 words past the last base (pad with zeros).
 */
#ifndef SDT_GPU_H
#define SDT_GPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDT_ABI_VERSION 8

enum {
	SDT_OK       = 0,
	SDT_EINVAL   = -1,   /* bad argument */
	SDT_ENODEV   = -2,   /* no gfx950 device / HIP runtime error at init */
	SDT_ENOMEM   = -3,   /* device or host allocation failed */
	SDT_EHIP     = -4,   /* HIP runtime error (message in sdt_gpu_last_error) */
	SDT_EFULL    = -5,   /* node table cannot grow any further */
	SDT_ESTATE   = -6,   /* call out of order (e.g. export before finish); also: the pipeline's conservation check failed
	                      * (k-mers cut into records != k-mers counted, sdt_gpu_finish_count) -- never a silent loss */
	SDT_ELIMIT   = -7    /* a data-dependent limit of a device algorithm was passed (sdt_gpu_layout_on_device: rounds of a growth,
	                      * depth of an eviction chain); nothing was changed: the caller takes the other path */
};

typedef struct sdt_ctx sdt_ctx;

/* sdt_gpu_init flags: pick the pass-1 kernel family.  Both give identical tables.  Default (neither flag): the locality
 * pipeline wherever its geometry applies (reads of K+1 .. ~550 bases, one rank), the direct kernel otherwise. */
#define SDT_FLAG_DIRECT    1u   /* always one device atomic per k-mer occurrence (k_count_reads) */
#define SDT_FLAG_PARTITION 2u   /* locality pipeline (csrc/sdt_superkmer.cuh): minimizer buckets of super-k-mers, counted in LDS,
                                 * one merge per distinct key and batch */
/* Track, per node, the ordinal of its first occurrence in the read stream: (read ordinal << 16) | position.
 * The reference's table layout -- hence the visiting order of its cutting passes, the order of *.vertex and the
 * edge ids -- is a function of exactly this order; the host replays it (csrc/host/graph). */
#define SDT_FLAG_TRACK_FIRST 4u
/* Keep every pushed batch of packed reads resident in HBM so that the second pass over the reads
 * (prlRead2edge, sdt_gpu_map_reads) needs no re-parse: 0.25 B/base, 7.5 GB for 200 M x 150 bp. */
#define SDT_FLAG_KEEP_READS 8u
/* map stage: the table indexes the k-mers of the contigs (sdt_gpu_index_contigs; implies TRACK_FIRST) */
#define SDT_FLAG_CONTIG_INDEX 16u
/* (bits 32 and 64 were SDT_FLAG_FLAT_MERGE / SDT_FLAG_NODE_LOG until ABI 7: the count stage of the locality pipeline merges every
 * generation of its LDS table into the node table, the only form since ABI 8; the bits are ignored) */

/* ---- lifecycle ------------------------------------------------------------------------------ */

/* Replaces the allocation half of prlRead2HashTable (prlHashReads.c:355,402-423: createFilter +
 * init_kmerset x thrd_num).  K = overlaplen after call_pregraph's clamp (pregraph.c:38-59): odd, 13..127.
 * est_distinct sizes the device node table (it grows by rebuild when needed, the analogue of
 * encap_kmerset, newhash.c:293-409); 0 = default.  device = HIP device ordinal. */
int sdt_gpu_init(sdt_ctx **ctx, int device, int K, uint64_t est_distinct, uint32_t flags);
int sdt_gpu_destroy(sdt_ctx *ctx);                 /* free_Sets (pregraph.c:107) */
const char *sdt_gpu_last_error(void);
int sdt_gpu_abi_version(void);

/* forget all nodes, keep allocations (a fresh prlRead2HashTable run on the same context).  The clear of the node table is deferred: the
 * first read pushes carry it inside their level-1 scatter, any other call that needs the table clears what is left first
 * (INTEGRATION.md section 1); no call sees anything but an empty table. */
int sdt_gpu_reset(sdt_ctx *ctx);

/* ---- pass 1: chop + insert/count ------------------------------------------------------------- */

/* The longest read pass 1 counts.  Every batch may end up in the direct kernel, which stages 64 reads of the batch's longest
 * length in one LDS tile of at most 64 KiB: 584 + 16 L bytes.  (The 12-bit position of a super-k-mer record, 4 095, is never the
 * binding limit.)  A batch that holds a longer read is refused as a whole with SDT_EINVAL by the call that hands it over -- the
 * message names the length and this limit -- and nothing of it is counted, kept (SDT_FLAG_KEEP_READS) or numbered (read ordinals):
 * the context goes on as if the call had not been made.
 *
 * Below that limit the length of a batch's longest read decides the KERNEL FAMILY and never the result: reads of up to 256 k-mers
 * take the one-lane-per-read scatter of the locality pipeline, longer ones its strip kernel, and a batch whose scatter tile no
 * longer fits 160 KiB of LDS (about 1 130 bases while the window holds at most 49 m-mers, K = 31; about 600 bases with the second
 * hash array of longer windows, K >= 61) is counted by the direct kernel -- silently, under SDT_FLAG_PARTITION too, and in the
 * middle of a stream, as is a batch whose read ordinals would pass 2^34.  The tables are identical whichever way a batch went. */
#define SDT_PASS1_MAX_READ_LEN 4059

/* Replaces one `sendWorkSignal(2); sendWorkSignal(1);` pair (prlHashReads.c:523-526,600-606,615-620):
 * chopKmer4read over every read of the batch (:164-310) and put_kmerset of every record
 * (newhash.c:411-462).  Host buffers; the call stages them to the device asynchronously (double
 * buffered) and returns once the buffers may be reused.  Reads shorter than K+1 are skipped (:592).
 * Longest read: SDT_PASS1_MAX_READ_LEN bases, SDT_EINVAL beyond (see there); the length picks the kernel family, never the result. */
int sdt_gpu_push_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords,
                       const uint64_t *offsets, uint64_t nreads);

/* The same without the wait: the call returns as soon as the copies and kernels are enqueued (a ring of 48 device staging
 * buffers, up to 32 batches staged ahead of their kernels; the host blocks only when the ring is full).  The caller's buffers must
 * stay untouched until sdt_gpu_push_wait(ctx, *ticket) has returned -- a host that parses into a ring of its own waits for
 * the ticket of the buffer it is about to refill, not for every push (prlHashReads.c:493-620 double-buffers the same way:
 * one buffer is parsed while the threads work on the other).  Pinned host memory keeps the copy asynchronous.
 * hint_total_kmers: the caller expects this many k-mers in all, so the first small batch already takes the locality pipeline
 * (cleared by sdt_gpu_reset).
 * Longest read: SDT_PASS1_MAX_READ_LEN bases (see there); a batch with a longer read is SDT_EINVAL from THIS call, never from the
 * later call in which its kernels would have been launched; no new ticket is issued for it. */
int sdt_gpu_push_reads_async(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                             uint64_t *ticket);
/* a batch whose reads all have read_len bases (read i starts at base i * read_len): no offsets cross PCIe, the device makes them.
 * Longest read: read_len <= SDT_PASS1_MAX_READ_LEN (see there), SDT_EINVAL from this call beyond. */
int sdt_gpu_push_reads_fixed_async(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, uint64_t nreads, uint64_t read_len,
                                   uint64_t *ticket);
int sdt_gpu_push_wait(sdt_ctx *ctx, uint64_t ticket);
/* pinned host memory for the buffers of asynchronous pushes (the copy engine reads it directly; a push from pageable memory is
 * staged by the runtime at a fraction of the link and blocks the caller): stands where the reference mallocs its two read
 * buffers (prlHashReads.c:430-470).  NULL when no memory can be pinned.  Callable from any host thread. */
void *sdt_gpu_host_alloc(size_t bytes);
void sdt_gpu_host_free(void *p);
int sdt_gpu_hint_total_kmers(sdt_ctx *ctx, uint64_t kmers);

/* Read ordinals of the NEXT batch: read i of it gets ordinal base + i*stride; afterwards the base advances by
 * nreads*stride.  Only needed with SDT_FLAG_TRACK_FIRST when the stream is not consumed file after file: the
 * reference interleaves paired files read1, read2, read1, ... (prlHashReads.c:493-567) = stride 2, base 0 / 1. */
int sdt_gpu_set_read_ordinal(sdt_ctx *ctx, uint64_t base, uint64_t stride);

/* Same, for a batch that is already resident in device memory (device pointers; the bench and the
 * multi-GPU driver use this).  Asynchronous on the context's stream.  max_read_len bounds the longest
 * read of the batch (the reference's maxReadLen, prlHashReads.c:358-366); it sizes the LDS tile.
 * Longest read: max_read_len <= SDT_PASS1_MAX_READ_LEN, SDT_EINVAL beyond, before any launch and with nothing counted or numbered;
 * max_read_len picks the kernel family, never the result.  (A max_read_len smaller than the batch's longest read is not policed.) */
int sdt_gpu_count_reads_device(sdt_ctx *ctx, const void *d_packed_words, uint64_t nwords,
                               const void *d_offsets, uint64_t nreads, uint64_t max_read_len);

/* Drain: all pushed batches are in the table on return (end of the read loop, prlHashReads.c:615-623).
 * Outputs (may be NULL): k-mer occurrences processed ("kmer in reads", :662) and distinct nodes
 * ("nodes allocated" = sum of count_kmerset, :655-662).  SDT_EFULL if an insert ever found no slot; SDT_ESTATE if the
 * k-mers that went into the locality pipeline's records are not the k-mers that came out of its count stage. */
int sdt_gpu_finish_count(sdt_ctx *ctx, uint64_t *kmers_processed, uint64_t *nodes);

/* ---- multi-GPU, bucket sharding (the product path) ---------------------------------------------------------
 * The reference partitions records over threads by hash_kmer % thrd_num (prlHashReads.c:79-88).  Across the GPUs of a
 * node every rank owns a contiguous range of the 256 level-1 minimizer buckets (csrc/sdt_superkmer.cuh): all
 * occurrences of a canonical k-mer -- either strand, any read -- fall into one bucket, so they meet on one rank.
 * What travels is the super-k-mer record (~3 B per k-mer occurrence instead of a 16-B (key, meta) record), in
 * level-1 chunks: one grouped ncclSend / ncclRecv per peer and round over xGMI, on a stream of its own, while the
 * next round's reads are chopped and the previous round's records are split and counted.
 *   comm_id / comm_init      one process per GPU; rank 0 makes the id (ncclGetUniqueId) and hands it to the others
 *   comm_init_shm            same protocol over POSIX shared memory + host staging: validation where several ranks
 *                            share one GPU (RCCL refuses that), never for a reported number
 *   count_reads_sharded      COLLECTIVE: every rank calls it with ITS slice of the reads (device buffers as in
 *                            sdt_gpu_count_reads_device; nreads may be 0).  On return the k-mers of all slices are in
 *                            the tables of their owners (asynchronously: sdt_gpu_finish_count drains).
 *   push_reads_sharded       the same for host buffers
 *                            Longest read: what the level-1 scatter of the locality pipeline holds in 160 KiB of LDS -- about
 *                            1 130 bases at K = 31, about 600 from K = 61 on (the single-GPU calls hand such a batch to the direct
 *                            kernel; a rank cannot, the k-mers may be another rank's).  Beyond: SDT_EINVAL on every rank, "reads of
 *                            <n> bases do not fit the LDS tile of the sharded path", nothing counted or numbered, the contexts go
 *                            on.  A communicator of ONE rank counts through sdt_gpu_count_reads_device and has its limit instead.
 *   allreduce_i64            COLLECTIVE sum, for counters and the 257 kmerFreq bins (freqStat sums per-thread bins,
 *                            prlHashReads.c:1004-1014)
 *   comm_stats               bytes this rank sent / received in exchanges and the time they took on the exchange stream
 *   shard_ranges / sdt_kmer_bucket   who owns what: rank r owns the level-1 buckets [first_bucket[r], first_bucket[r + 1])
 *                            (nranks + 1 entries), cut on the FIRST sharded call so that the ranks' bucket weights -- taken
 *                            from a sample of every rank's reads -- are equal; sdt_kmer_bucket is the host copy of the device's
 *                            bucket function (canonical k-mer -> 0..255).  sdt_kmer_owner: the owner under EQUAL ranges. */
typedef struct { unsigned char bytes[128]; } sdt_comm_id;
int sdt_gpu_comm_id(sdt_comm_id *id);
int sdt_gpu_comm_init(sdt_ctx *ctx, const sdt_comm_id *id, int rank, int nranks);
int sdt_gpu_comm_init_shm(sdt_ctx *ctx, const char *name, int rank, int nranks);
int sdt_gpu_count_reads_sharded(sdt_ctx *ctx, const void *d_packed_words, uint64_t nwords, const void *d_offsets,
                                uint64_t nreads, uint64_t max_read_len);
int sdt_gpu_push_reads_sharded(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                               uint64_t nreads);
int sdt_gpu_allreduce_i64(sdt_ctx *ctx, int64_t *vals, int n);
int sdt_gpu_comm_stats(sdt_ctx *ctx, uint64_t *bytes_sent, uint64_t *bytes_recv, double *exchange_ms, uint64_t *exchanges);
int sdt_gpu_shard_ranges(const sdt_ctx *ctx, uint32_t *first_bucket);
int sdt_kmer_bucket(const uint64_t *key_words_msw_first, int K);

/* the FINAL minimizer bucket (0 .. 2^18 - 1) of a canonical k-mer: the unit the count stage of the locality pipeline works on (one
 * workgroup counts all occurrences of a bucket's keys in LDS) */
int sdt_kmer_final_bucket(const uint64_t *key_words_msw_first, int K);
/* the node table as it stands: info[1] slots, [2] nodes as of the last look at the device's counters; the other words are 0
 * (they described the node log of ABI 7) */
int sdt_gpu_table_info(sdt_ctx *ctx, uint64_t info[8]);
int sdt_kmer_owner(const uint64_t *key_words_msw_first, int K, int nranks);
/* After pass 1 the order-dependent graph phases (cutTipPreGraph.c, node2edge.c) run on ONE host over ALL nodes: rank 0
 * takes the other ranks' exported shards (sdt_gpu_export_nodes arrays; keys are disjoint by construction) into its own
 * table with import_nodes -- its device mirror then answers the dry runs and the second read pass for the whole
 * graph -- and keeps every read of the run resident with keep_reads (like SDT_FLAG_KEEP_READS, minus the counting;
 * ordinals from sdt_gpu_set_read_ordinal as for a push). */
int sdt_gpu_import_nodes(sdt_ctx *ctx, const uint64_t *keys, const uint32_t *l_links, const uint32_t *r_flags,
                         const uint32_t *count, const uint64_t *first, uint64_t n);
int sdt_gpu_keep_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads);
/* host-only self test of the shared-memory transport's control plane (no device needed; the CPU tests run it with
 * several processes) */
int sdt_comm_selftest_shm(const char *name, int rank, int nranks, int rounds);

/* The exchange plan as pure host functions of the count matrix (csrc/sdt_shard_plan.h; no device, no communicator): what
 * sdt_gpu_count_reads_sharded computes after its all-gather, exported so that the protocol can be driven -- and checked --
 * with any transport (tests/test_multirank_gloo.py: two gloo ranks on CPU).
 *   mat[r * 257 + b]   first position of level-1 bucket b in rank r's chunk list (b = 256: the list's length)
 *   cut_ranges         ranges[0..nranks]: rank d owns buckets [ranges[d], ranges[d + 1]), equal weights
 *   plan               sub-round t of the exchange as rank `me` sees it (*subrounds: how many there are -- the same on every
 *                      rank): for every peer p the piece [send_begin[p], + send_count[p]) of my chunk list, its place
 *                      send_at[p] in my send buffer (p == me: in my receive buffer), and the run recv_count[s] at recv_at[s]
 *                      of my receive buffer that arrives from rank s.  Arrays of nranks entries. */
int sdt_shard_cut_ranges(const uint32_t *mat, int nranks, uint32_t *ranges);
int sdt_shard_plan(const uint32_t *mat, int nranks, int me, const uint32_t *ranges, uint32_t recv_chunks, uint32_t t,
                   uint32_t *subrounds, uint32_t *send_begin, uint32_t *send_count, uint32_t *send_at, uint32_t *recv_count,
                   uint32_t *recv_at);

/* The work items and launches of the count stage as a pure host function of the level-2 chunk lists (csrc/sdt_count_plan.h; no
 * device): what the library computes between the level-2 scatter and k_sk_count, callable so that it can be tested on a CPU.
 *   off2[f], kpre2[f]   first chunk / first k-mer of final bucket f in the chunk list (f = nbuckets: the totals)
 *   items               4 words per work item: the run [c0, c1) of the list, top bit of c1 = the item holds whole buckets only;
 *                       its first and its last final bucket.
 *                       Buckets of <= 64 chunks share an item with their neighbours -- inside one level-1 bucket and a span of 64
 *                       final buckets --, buckets of > 1024 chunks are cut into pieces.
 *   first_item[l], launch_kmers[l]   first item and k-mers of launch l (first_item[*nlaunches] = *nitems); a launch is cut
 *                       between buckets at `limit` k-mers (`first_limit` for the first).
 * Stands where the reference hands a batch of k-mers to its threads (prlHashReads.c:312-336, sendWorkSignal). */
int sdt_sk_plan_count_items(const uint32_t *off2, const uint64_t *kpre2, uint32_t nbuckets, uint64_t first_limit, uint64_t limit,
                            uint32_t max_launches, uint32_t *items, uint32_t items_cap, uint32_t *first_item, uint64_t *launch_kmers,
                            uint32_t launches_cap, uint32_t *nitems, uint32_t *nlaunches);

/* ---- table scans ------------------------------------------------------------------------------ */

/* deLowCov / thread_delow (prlHashReads.c:844-909), `-d d`: zero links with 0 < v <= d, mark nodes
 * left without links deleted.  *removed = "%lld kmer removed". */
int sdt_gpu_delow(sdt_ctx *ctx, int d, uint64_t *removed);

/* Mark1in1outNode / thread_mark (prlHashReads.c:911-992): set `linear`, fill the 257-bin histogram
 * that freqStat (:994-1023) prints bins 1..255 of.  *linear = "%lld linear nodes". */
int sdt_gpu_mark_and_hist(sdt_ctx *ctx, int64_t hist[257], uint64_t *linear);

/* ---- hand the node table back to host graph phases (cutTipPreGraph.c, node2edge.c) ------------
 * Copies every node to caller-owned host arrays of capacity max_nodes (order unspecified):
 *   keys     : key_words() uint64 per node, MOST significant word first (the reference Kmer struct order)
 *   l_links  : kmer_t.l_links (4 x 6-bit, inc/newhash.h:38-43)
 *   r_flags  : the second 32-bit word of kmer_t (inc/newhash.h:69-75): r_links:24 | linear<<24 |
 *              deleted<<25 | checked<<26 | single<<27 | twin<<28 | inEdge<<30
 *   count    : kmer_t.count
 *   first    : first-occurrence ordinal (needs SDT_FLAG_TRACK_FIRST)
 * Any array may be NULL.  *n receives the node count. */
int sdt_gpu_export_nodes(sdt_ctx *ctx, uint64_t *keys, uint32_t *l_links, uint32_t *r_flags,
                         uint32_t *count, uint64_t *first, uint64_t max_nodes, uint64_t *n);

/* --gpus N, second read pass on every rank: the final graph as that pass needs it -- every node's key and path word -- out of the
 * table of the rank that built the edges (after sdt_gpu_load_paths), and into the table of a rank that holds its own share of the
 * reads (sdt_gpu_keep_reads / SDT_FLAG_KEEP_READS): its shard of pass 1 makes way, the kept reads stay; patch table and edge count
 * as in sdt_gpu_load_paths.  Then sdt_gpu_map_reads + sdt_gpu_export_arcs on every rank, and the arcs of all ranks add up
 * (prlRead2path.c:415-430 counts arcs per thread and adds them the same way). */
int sdt_gpu_export_paths(sdt_ctx *ctx, uint64_t *keys, uint64_t *path_words, uint64_t max_nodes, uint64_t *n);
int sdt_gpu_import_paths(sdt_ctx *ctx, const uint64_t *keys, const uint64_t *path_words, uint64_t n, const uint64_t *patch_keys,
                         const uint64_t *patch_info, uint64_t npatch, uint64_t num_ed);
/* A rank whose shard has been handed over (sdt_gpu_export_nodes) and that now waits for the graph: its node table, the
 * first-occurrence ordinals and the pools of the locality pipeline go back to the device; the reads kept for the second pass stay.
 * The context then holds no nodes until sdt_gpu_import_paths gives it the graph.  (The reference frees its sets only at the very
 * end, pregraph.c:107-108: one process, one address space.  Here the waiting ranks may share a device with rank 0's graph phases.) */
int sdt_gpu_release_table(sdt_ctx *ctx);
/* ---- pass 2: reads -> edge paths -> arcs (prlRead2edge, prlRead2path.c:817-1335) --------------------------
 * After the host graph phases (minor-out, tip cutting, kmer2edges) every node gets one path word
 *     bit 0 skip = deleted || (linear && !inEdge) (:650) | bit 1 linear | bits 2..3 twin | bits 32..63 l_links = edge id
 * and the (K+1)-mers of length-1 edges (KmerSetsPatch, node2edge.c:404-463) come as patch_keys (key_words()
 * words each, most significant first) with patch_info = edge id | twin << 32.  load_paths overwrites the
 * nodes' counters with the path words (export the table first); keys == NULL: path_words[i] belongs to node i of
 * sdt_gpu_set_node_index / sdt_gpu_layout_apply (no keys to send, no look-ups); path_words == NULL as well: the path words
 * sdt_gpu_build_edges left on the device.  map_reads then replays parse1read (:617-789),
 * search1kmerPlus (:575-615) and the arc counting (:190-241,415-430) over the kept reads; export_arcs returns
 * every arc with its multiplicity and the ordinal of its first appearance ((read ordinal << 16) | item index):
 * per from-edge the reference prints arcs most-recent-first-appearance first (:427-428,472-496) -- the arrays come in that order
 * (from ascending, first appearance descending) since round 5.
 * SDT_ESTATE from load_paths / import_paths: a key that is not in the table / a key twice (the message says how many).  The nodes
 * that were found have their path words by then, but the context is not poisoned: the same call with the right keys succeeds. */
int sdt_gpu_load_paths(sdt_ctx *ctx, const uint64_t *keys, const uint64_t *path_words, uint64_t n,
                       const uint64_t *patch_keys, const uint64_t *patch_info, uint64_t npatch, uint64_t num_ed);
int sdt_gpu_map_reads(sdt_ctx *ctx, uint64_t *reads_processed, uint64_t *arcs);
int sdt_gpu_export_arcs(sdt_ctx *ctx, uint32_t *from, uint32_t *to, uint32_t *mult, uint64_t *first,
                        uint64_t max_arcs, uint64_t *n);

/* ---- graph-cleaning dry runs (cutTipPreGraph.c) on the device mirror of the host graph ------------------
 * The passes after kmerFreq are order-dependent: the host commits their writes in the reference's
 * order.  What each sweep needs before that is read-only -- the walk from every dead end to the node it runs
 * into (clipTipFromNode, cutTipPreGraph.c:43-281) -- and that is table look-ups: the device table, kept equal to
 * the host graph, answers them for all nodes at once.
 *   set_node_index: keys in the host's visiting order (index i = position in `keys`); results are indexed by it.
 *   update_nodes:   links / linear / deleted of the nodes the host wrote since the last call (l_links, r_flags as
 *                   in export_nodes).
 *   tip_walks:      for every node i: end_idx[i] = index of the node the walk from i stops at, ~0 when there is
 *                   nothing to decide (not a dead end, chain longer than cut_len, deleted, linear; thin != 0:
 *                   removeSingleTips' rule, only `single` nodes start or continue a walk); info[i] = ch | sm << 2 |
 *                   thin_stop << 3: the base by which the end node sees the chain, the strand it was reached on,
 *                   and (thin) whether the walk stopped at a linear node that is not single (:163-166). */
int sdt_gpu_set_node_index(sdt_ctx *ctx, const uint64_t *keys, uint64_t n);
int sdt_gpu_update_nodes(sdt_ctx *ctx, const uint64_t *keys, const uint32_t *l_links, const uint32_t *r_flags, uint64_t n);
int sdt_gpu_tip_walks(sdt_ctx *ctx, int thin, int cut_len, uint64_t *end_idx, uint8_t *info, uint64_t n);
/*   tip_walks_compact: the same walks, only for the nodes that have one, in no particular order: records of 2 words,
 *                   [0] = node index | info << 56, [1] = end index.  SDT_EFULL: *n_records says how many there are. */
int sdt_gpu_tip_walks_compact(sdt_ctx *ctx, int thin, int cut_len, uint64_t *records, uint64_t max_records,
                              uint64_t *n_records);
/*   minor_out_dry:  removeMinorOut's read-only part (cutTipPreGraph.c:1012-1076): every junction whose ratio test
 *                   (count / largest count on that side < threshold = dd / 100.0, clipKmerFromNode :591-1010)
 *                   would cut at least one neighbour on the graph as it is now, and who the neighbours of those
 *                   junctions and of the neighbours to cut are.  records: 9 words each -- node index, then
 *                   (neighbour index << 1 | smaller) or ~0 for the four left and the four right links;
 *                   [0, n_junctions) are the junctions, [n_junctions, n_records) the neighbours to cut that are not
 *                   junctions themselves.  SDT_EFULL when records[] is too small: *n_records says what is needed. */
int sdt_gpu_minor_out_dry(sdt_ctx *ctx, double threshold, uint64_t *records, uint64_t max_records,
                          uint64_t *n_junctions, uint64_t *n_records);
/*   build_host_index: the host's k-mer -> node look-up table for the ordered commits (csrc/host/graph/graph.c:
 *                   open addressing over index_slots = 2^m >= 2n 32-bit words, home slot = mix_key(4-word k-mer) &
 *                   (slots-1), linear probing, value = node index + 1, 0 = empty), filled by the device from its node index. */
int sdt_gpu_build_host_index(sdt_ctx *ctx, uint32_t *index, uint64_t index_slots);
/*   build_host_index64: the same with 64-bit entries (value = node index + 1), for graphs past 2^32 - 2 nodes.
 * Node indices of the graph phases (set_node_index, layout_apply, layout_on_device number the nodes) take one of two forms,
 * fixed when the nodes are numbered: 32-bit below 2^32 - 16 nodes, 64-bit past that or when the caller asked for it.
 *   set_graph_index_bits: 0 = by node count (the default), 64 = the 64-bit form at the next numbering.
 *   graph_index_bits:     32 or 64, the form of the numbering in effect (before one: the form the next one takes). */
int sdt_gpu_build_host_index64(sdt_ctx *ctx, uint64_t *index, uint64_t index_slots);
int sdt_gpu_set_graph_index_bits(sdt_ctx *ctx, int bits);
int sdt_gpu_graph_index_bits(const sdt_ctx *ctx);
/*   edge_ports:     kmer2edges' walks (node2edge.c:46-191): for every node that is neither linear nor deleted one
 *                   record of 17 words -- node index, then for each of its 8 ports (right links 0..3 on the stored
 *                   strand, left links 0..3 on the reverse strand) the index of the first non-linear node the chain
 *                   of linear nodes leads to (~0: no link) and  length | far_port << 32 | bal_edge << 40  (the port
 *                   the chain arrives through; bal_edge = 0 when the chain is its own reverse complement,
 *                   check_iden_kmerList :563-588).  SDT_EFULL when records[] is too small (*n_records = needed). */
int sdt_gpu_edge_ports(sdt_ctx *ctx, uint64_t *records, uint64_t max_records, uint64_t *n_records);

/* ---- the reference's visiting order, and the dry runs labelled for commits that run side by side ----------------------
 * Every phase after kmerFreq walks the reference's tables "set 0..p-1, slot 0..size-1" (cutTipPreGraph.c:351-366,385-408,
 * 1049-1072, node2edge.c:46-56), and a node's place there is a function of hash_kmer(key) % p and of the order in which the
 * distinct keys of its set first occurred (put_kmerset / encap_kmerset, newhash.c:293-462).  The device knows both:
 *   layout_sorted_keys: sorts the nodes by (set, first-occurrence ordinal) -- set = hash_kmer (hashFunction.c:83-122) over the
 *                   bytes of the nw_variant-word Kmer of the emulated binary, % p -- and returns the KEYS in that order
 *                   (key_words() words each) with set_start[0..p]; keys == NULL: only *n.  Ends pass 1 (its pools are freed).
 *   layout_apply:   order[v] = rank (index into that key array) of the node at visiting position v, from the host's replay of
 *                   the probing (csrc/host/graph/graph.c: graph_replay_order).  Numbers the nodes: everything below that
 *                   speaks of a node index means v.  Replaces sdt_gpu_set_node_index (no keys cross the link).
 *   export_ordered: the nodes in visiting order, arrays as sdt_gpu_export_nodes (any may be NULL).
 *   update_nodes_by_index: sdt_gpu_update_nodes with node indices instead of keys.
 *   tip_walks_labelled / minor_out_labelled: the dry runs of sdt_gpu_tip_walks_compact / sdt_gpu_minor_out_dry with one more
 *                   word per record, the COMPONENT of the record's node: a visit of the ordered commit reads and writes only
 *                   its own node and nodes of the same component, so components commit side by side, each in the reference's
 *                   order (csrc/host/graph/cuttip.c).  Components = union-find over node indices on the device --
 *                   removeSingleTips (thin): tip + end node of every walk; removeMinorTips: non-linear nodes joined by chains
 *                   of <= cut_len linear nodes; removeMinorOut: every record's node + its eight neighbours.  Records:
 *                   walks 3 words (node | info << 56, end, label), all sorted by (label, node); junctions 14 words (node,
 *                   8 neighbours, their 8 occurrence counts two per word, label), the first *n_junctions sorted by
 *                   (label, node), then the neighbours to cut.
 *                   The records stay on the device until fetch_records copies them (nwords = records x words, exactly). */
int sdt_gpu_layout_sorted_keys(sdt_ctx *ctx, int p, int nw_variant, uint64_t *keys, uint64_t max_nodes, uint64_t *set_start, uint64_t *n);
int sdt_gpu_layout_apply(sdt_ctx *ctx, const uint64_t *order, uint64_t n);
/*   layout_on_device: layout_sorted_keys + the replay of put_kmerset / encap_kmerset (newhash.c:293-462) + layout_apply in one call,
 *                   nothing but set_start[0..p] crosses the link.  Between two growths a set is laid out by priority insertion
 *                   (first come first served in first-occurrence order, built in any order); a growth -- the in-place rehash of
 *                   :359-406, where an entry that gives way is carried on at once -- as a fixed point of insertion times, ten to
 *                   twenty rounds of priority insertion (csrc/sdt_graph_kernels.cuh; tools/replay_fixed_point.c checks the
 *                   formulation against the sequential emulation).  small_init != 0: the sets of the 63mer / 127mer variants
 *                   start at 3 slots (`-a`, prlHashReads.c:404-413).  SDT_EINVAL when a limit is passed (2^32 nodes, a set's table
 *                   of 2^32 slots, the packed table word): use the two-step form with the host's replay then.
 *                   Round 5: SDT_ELIMIT for those limits and for a growth that does not settle; the rounds are incremental (only the
 *                   stretch from a changed entry's home to the end of its cluster is laid out again); on success the first-occurrence
 *                   ordinals are dropped (8 bytes per table slot: layout_sorted_keys / export_nodes(first) return SDT_ESTATE after). */
int sdt_gpu_layout_on_device(sdt_ctx *ctx, int p, int nw_variant, int small_init, uint64_t *set_start, uint64_t *n);
int sdt_gpu_export_ordered(sdt_ctx *ctx, uint64_t *keys, uint32_t *l_links, uint32_t *r_flags, uint32_t *count, uint64_t n);
int sdt_gpu_update_nodes_by_index(sdt_ctx *ctx, const uint64_t *node, const uint32_t *l_links, const uint32_t *r_flags, uint64_t n);
int sdt_gpu_tip_walks_labelled(sdt_ctx *ctx, int thin, int cut_len, uint64_t *n_records);
int sdt_gpu_minor_out_labelled(sdt_ctx *ctx, double threshold, uint64_t *n_junctions, uint64_t *n_records);
int sdt_gpu_fetch_records(sdt_ctx *ctx, uint64_t *dst, uint64_t nwords);
/*   minor_out_commit: removeMinorOut's COMMIT (cutTipPreGraph.c:591-1010: the ratio test on the live links, `deleted`, the
 *                   neighbours' links cleared and their `linear` re-derived) on the records minor_out_labelled left on the device,
 *                   one lane per component, the visits of a component in the reference's order; then thread_mark's re-marking
 *                   over the nodes it wrote (:911-967).  *off = "kmers off", *linear = nodes newly marked linear, *n_written =
 *                   nodes whose links or flags changed -- fetch_written copies them out as (index, l_links, r_links | linear << 24 |
 *                   deleted << 25), the form update_nodes_by_index takes.  Components of more than max_component visits (*largest
 *                   = the largest there is) are left alone: one lane is no match for a host thread on a long chain of dependent
 *                   accesses.  fetch_skipped hands their records over (*n_skipped_records of 14 words: first their *n_skipped junction
 *                   records in order, then the records of the neighbours they may cut); the caller commits them (they touch no node
 *                   the device wrote) and sends what it wrote with update_nodes_by_index. */
int sdt_gpu_minor_out_commit(sdt_ctx *ctx, double threshold, uint64_t max_component, uint64_t *largest, uint64_t *off, uint64_t *linear, uint64_t *n_written,
                             uint64_t *n_skipped, uint64_t *n_skipped_records);
int sdt_gpu_fetch_skipped(sdt_ctx *ctx, uint64_t *dst, uint64_t n_records);
/*   minor_out_commit in two halves, so that the caller can commit the long components while the device walks the short ones:
 *                   _begin finds the components, gathers the records of the long ones (fetch_skipped may be called right after it)
 *                   and LAUNCHES the visits; _finish waits for them, re-marks and lists the written nodes (fetch_written). */
int sdt_gpu_minor_out_commit_begin(sdt_ctx *ctx, double threshold, uint64_t max_component, uint64_t *largest, uint64_t *n_skipped, uint64_t *n_skipped_records);
int sdt_gpu_minor_out_commit_finish(sdt_ctx *ctx, uint64_t *off, uint64_t *linear, uint64_t *n_written);
int sdt_gpu_fetch_written(sdt_ctx *ctx, uint64_t *node, uint32_t *l_links, uint32_t *r_flags, uint64_t n);
/* kmer2edges (node2edge.c:46-561) on the device mirror, after sdt_gpu_layout_apply: every chain of linear nodes between two
 * nodes that are neither linear nor deleted is one edge; it belongs to the first of its two (node, port) ends in visiting order
 * (ports: right links 0..3 on the stored strand, then left links 0..3 on the other), ids are handed out in that order (an edge
 * that is not its own reverse complement takes two), the interior nodes are stamped with id and twin (merge_linearV2, :351-561)
 * -- as PATH WORDS: sdt_gpu_load_paths(ctx, NULL, NULL, n, ...) then takes them from the device.  *n_edges records wait for
 * sdt_gpu_fetch_records (4 + 2 * key_words() words each, in id order: length | bal_edge << 32, cvg, id, offset of the edge's
 * bases, first and last oriented k-mer) and *n_bases letters for sdt_gpu_fetch_edge_bases (the last base of nodes 1..length of
 * every edge); *num_ed = ids handed out (EDGEs of *.preGraphBasic).  SDT_ESTATE with "does not lead back" in the message: a
 * chain is not symmetric -- nothing was stamped, build the edges sequentially (node2edge.c's own order). */
int sdt_gpu_build_edges(sdt_ctx *ctx, uint64_t *n_edges, uint64_t *num_ed, uint64_t *n_bases);
int sdt_gpu_fetch_edge_bases(sdt_ctx *ctx, char *dst, uint64_t nbytes);

/* ---- `map` stage: prlContig2nodes (prlHashCtg.c:287-425) and prlRead2Ctg (prlRead2Ctg.c:656-894) -------
 * A context created with SDT_FLAG_CONTIG_INDEX holds the k-mers of the contigs:
 *   index_contigs: contigs packed like reads (2 bit / base, offsets in bases, 4 pad words), ids[i] = the id the
 *                  reference takes from the record name (getID, prlHashCtg.c:276-285) -- the caller has applied
 *                  the length cut (:343-350).  May be called repeatedly; contig order = call order, array order.
 *                  The first occurrence of a k-mer (contig order, then position) owns contig id / position /
 *                  strand, every further one marks it deleted (singleKmer :110-139).
 *                  sdt_gpu_finish_count then reports "kmer in reads" and "nodes allocated" (:397).  The first
 *                  align call freezes the index (nodes are rewritten into their look-up form): SDT_ESTATE after.
 *   set_contig_table: contig_array[0..num_ctg] of basicContigInfo (prlRead2Ctg.c:610-648): length, and
 *                  twin[i] = getTwinCtg(i) (attachPEinfo.c:479-482).
 *   align_reads:   chopKmer4read + searchKmer + parse1read (prlRead2Ctg.c:129-353) for a batch of reads.
 *                  align_len: per-read ALIGNLEN (the value of the global when the read's batch is parsed,
 *                  :774-791), or NULL and align_len_all for every read.
 *                  read_info[r] = more_start (40 bits) | nhits << 40 | best << 48 | footprint << 56 | overflow << 57;
 *                  nhits = count_Contig (0: ctgIdArray[t] = 0).  ctg2read[t][0] = hits[r]; ctg2read[t][m], m >= 1,
 *                  = hits[more_start + m - 1] (the tail of hits[] past the first nreads entries, in the reference's
 *                  order); best = index m of the hit that sets ctgIdArray / posArray / orienArray (posArray =
 *                  contig_offset - read_offset + 1); overflow: more than 20 candidate contigs -- the reference
 *                  overruns pos_temp[20] there; such a read is reported unmapped.
 *                  max_hits >= nreads; *nhits = entries of hits[] in use (nreads + all further hits); SDT_EFULL
 *                  when hits[] is too small: *nhits says how many the batch needs.
 *   align_reads_device: the same on buffers already in device memory (outputs too).
 * Limits.  A contig has fewer than 2^24 bases (positions are 24-bit): index_contigs returns SDT_EINVAL before any device work, nothing
 * of the call is indexed.  A read of align_reads has at most 8 152 k-mers (8 151 + K bases: 8 bytes per k-mer and 40 hit slots per
 * wavefront in 64 KiB of LDS); a batch (align_reads_device: a max_read_len) beyond is SDT_EINVAL before any launch, the index is
 * not frozen by that call.  Below, the length only picks the launch geometry (4, 2, 1 wavefronts per workgroup, changing past 1 496
 * and 3 032 k-mers), never the result. */
typedef struct {
	uint32_t contig;             /* READSET.contigID */
	int32_t contig_offset;       /* READSET.contigOffset */
	uint32_t read_offset;        /* READSET.readOffset (1-based k-mer index) */
	uint32_t align_len_orien;    /* READSET.alignLength | (orien == '-' ? 1u << 31 : 0) */
} sdt_hit;
int sdt_gpu_index_contigs(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          const uint32_t *ids, uint64_t ncontigs);
int sdt_gpu_set_contig_table(sdt_ctx *ctx, const uint32_t *length, const uint32_t *twin, uint64_t num_ctg);
int sdt_gpu_align_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                        uint64_t nreads, const int32_t *align_len, int align_len_all, uint64_t *read_info,
                        sdt_hit *hits, uint64_t max_hits, uint64_t *nhits);
int sdt_gpu_align_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                               uint64_t max_read_len, const void *d_align_len, int align_len_all, void *d_read_info,
                               void *d_hits, uint64_t max_hits, uint64_t *nhits);

/* ---- read-only questions to the counted table ------------------------------------------------------------
 * search_kmerset (newhash.c:239-283) has no counterpart in pass 1 itself: the reference calls it from the later phases
 * (prlRead2path.c:363-394, cutTipPreGraph.c, node2edge.c), always with the smaller of a k-mer and its reverse complement.
 *   search_kmers:   a batch of n k-mers; keys = n x key_words() words, most significant first, the k-mer as the caller has
 *                   it (either strand, K bases right-aligned, the bits above them 0).  For query i:
 *                     status[i]   bit 0 found | bit 1 the query is the larger strand, i.e. the node is stored as its reverse
 *                                 complement (set whether or not the node exists)
 *                     count[i], l_links[i], r_flags[i]   the words sdt_gpu_export_nodes gives for the node -- kmer_t.count,
 *                                 l_links, r_links:24 | linear << 24 | deleted << 25 | single << 27 -- as the STORED node has
 *                                 them (never swapped to the query's strand); 0 when the node does not exist.
 *                   Any output array may be NULL.  Host pointers; blocks.  _device: device pointers, asynchronous on the
 *                   context's stream.
 *   profile_reads:  the k-mer coverage of every read of a batch (packed as for sdt_gpu_push_reads): out[i] for read i.
 *                     kmers   len - K + 1 for len >= K, else 0 and every other field 0.  (NOT pass 1's len >= K + 1 rule,
 *                             prlHashReads.c:592: a profile is about the read, not about what was inserted.)
 *                     found   k-mers whose node exists;  solid: k-mers with count >= min_count (min_count == 0: all of them)
 *                     min, median, max   over ALL kmers counts, a k-mer without a node counting 0; median = the lower median,
 *                             element (kmers - 1) / 2 in ascending order
 *                   _device: buffers already on the device; max_read_len bounds the longest read (it sizes the LDS strip).  A
 *                   longer read gets kmers = 0xFFFFFFFF (other fields 0) and the call returns SDT_EINVAL; the call waits for
 *                   the kernel to know.
 *   profile_kept_reads: the same for the reads kept in HBM (SDT_FLAG_KEEP_READS / sdt_gpu_keep_reads): out[] is indexed by
 *                   READ ORDINAL (sdt_gpu_set_read_ordinal: base + i * stride of each kept batch), so interleaved paired
 *                   files land in the reference's stream order (prlHashReads.c:493-567).  out_capacity records; *nreads =
 *                   reads profiled.  Records of ordinals that no kept read has are left untouched.  SDT_EFULL, nothing
 *                   written, when a kept read's ordinal is >= out_capacity.
 * Allowed once sdt_gpu_finish_count has returned and for as long as the counters exist: after delow, mark_and_hist, layout or
 * cutting calls the answers describe the table as it is then.  SDT_ESTATE: batches pushed or counted and not yet drained; after
 * sdt_gpu_load_paths / sdt_gpu_import_paths (the counters hold path words); after sdt_gpu_release_table; on a
 * SDT_FLAG_CONTIG_INDEX context; on a context with a communicator (a shard cannot tell "absent" from "another rank's
 * bucket").  n == 0 / nreads == 0: SDT_OK, nothing touched.  The calls never write the table.
 * Longest read of the profile, correct, select and trim calls, every form: 16 384 k-mers (16 383 + K bases: the read's counts sit in a
 * strip of LDS, 4 bytes per k-mer, 64 KiB per wavefront).  A host batch that holds a longer read, or a max_read_len beyond, is
 * SDT_EINVAL from a host-side check before any launch: "reads of <n> bases do not fit the per-wavefront LDS strip", no output
 * written.  Below, the length only picks the launch geometry (4, 2, 1 wavefronts per workgroup, changing past 4 096 and 8 192
 * k-mers), never the result.  (Pass 1 itself takes reads of at most SDT_PASS1_MAX_READ_LEN bases; sdt_gpu_keep_reads has no limit.)
 *
 * Substitution errors corrected against the table (k-mer-spectrum correction, the usual step in front of a de Bruijn assembler).
 * Added without a change of SDT_ABI_VERSION: the five calls and sdt_read_fix are additions, nothing that existed has changed.
 * The rule is deterministic and decides every read on its own.  A read has n = len - K + 1 k-mers (0 for len < K) with the counts
 * c[j] that profile_reads sees (absent = 0; the deleted flag is ignored).  k-mer j is WEAK iff c[j] < min_count; a RUN is a maximal
 * stretch [a, b] of weak k-mers, l = b - a + 1.  Every run is judged on the read as it came (a substitution at p changes only
 * k-mers of its own run):
 *     a == 0 && b == n - 1  (nothing solid in the read)   no candidate
 *     a > 0 && b < n - 1    (interior)                    candidate iff l == K;  p = b
 *     a == 0 && b < n - 1   (head)                        candidate iff l <= K;  p = b
 *     a > 0 && b == n - 1   (tail)                        candidate iff l <= K;  p = a + K - 1
 * For a candidate each base x != read[p] is tried: x is valid iff every k-mer j in [a, b] of the read with base p replaced by x
 * has a count >= min_count.  Exactly one valid x: base p becomes x.  None or several: the read stays as it is.  min_count == 0:
 * nothing is weak, nothing changes.
 *   correct_reads:  fix[i] for read i of a batch (packed as for sdt_gpu_push_reads): kmers as sdt_read_cov, weak k-mers before the
 *                   correction, runs, substitutions made.  out_words (may be NULL): nwords words, the stream with the substitutions
 *                   made (pad words as they came).  edits (may be NULL): one word per substitution,
 *                       read << 18 | pos << 2 | new_base      (pos 0-based, < 65536; read = index in the batch)
 *                   ascending, i.e. by read, then by position; *n_edits = substitutions made.  SDT_EFULL when there are more than
 *                   max_edits: *n_edits says how many, the first max_edits are stored, fix[] and out_words are complete.
 *                   (The host and kept forms do not know the number of edits of a piece beforehand: a piece with more edits than
 *                   its device list holds runs the kernel a second time with a list of the size the first run asked for.)
 *   correct_reads_device: buffers already on the device; d_out_words must not overlap the input; d_edits in no particular order.
 *                   max_read_len as for profile_reads_device: a longer read gets kmers = 0xFFFFFFFF (other fields 0), stays as it
 *                   is in d_out_words, and the call returns SDT_EINVAL.  The call waits for the kernel to know *n_edits.
 *   correct_kept_reads: the reads kept in HBM; fix[] by READ ORDINAL like profile_kept_reads (SDT_EFULL, nothing written, when a
 *                   kept read's ordinal is >= out_capacity), edits ascending with the read ordinal in the place of the index.  The
 *                   kept reads are NOT changed: fetch them and apply the edits.
 *   kept_batches / fetch_kept_batch: the kept batches back on the host, in the order they were kept: info = nwords, nreads,
 *                   ord_base, ord_stride; words / offsets NULL: info only.  Needs kept reads, not a table: SDT_ESTATE without
 *                   them, SDT_EINVAL for i out of range, SDT_EFULL when a capacity is too small, SDT_ESTATE (info
 *                   included) while pushed batches are not drained (sdt_gpu_finish_count): their copies may be in flight.
 * State rules and return codes are those of the profile calls.  Nothing here writes the table or the kept reads.
 *
 * In-silico read normalisation against the table: a read is kept with probability target / median k-mer coverage, measured against
 * the table of ALL reads, so every read is decided on its own and the result does not depend on the order of the reads or on the
 * launch geometry.  Added without a change of SDT_ABI_VERSION: the five calls and the two structs are additions.  The rule is in
 * integers only.  A read has n = len - K + 1 k-mers (0 for len < K) with the counts c[j] that profile_reads sees (absent = 0; the
 * deleted flag is ignored).
 *     median   the lower median of c[], element (n - 1) / 2 ascending, of the unsaturated 32-bit counts (sdt_read_cov.median)
 *     S1, S2   the sum and the sum of squares of c'[j] = min(c[j], 65535); n * S2 < 2^64 as n <= 65 536
 *     a read is ABERRANT iff max_cv_pct > 0 and 10000 * (n * S2 - S1 * S1) > max_cv_pct * max_cv_pct * S1 * S1, evaluated in 128
 *              bits: stdev / mean > max_cv_pct / 100.  S1 == 0: both sides are 0, not aberrant.
 * A UNIT is one read, or the two mates of a pair; its id u is the index of its first read (dense forms) or that read's ordinal (kept
 * form).  cov of a single read = its median; of a pair = (mL + mR + 1) / 2 in 64 bits, or the other mate's median when one mate has
 * n == 0.  A unit is aberrant iff a mate with n > 0 is.  The same verdict goes to both mates, the first line that applies:
 *     4  every read of the unit has n == 0                dropped, short
 *     3  the unit is aberrant                             dropped, aberrant
 *     0  cov <= target                                    kept
 *     1  draw(u) * cov < target * 2^32                    kept by draw
 *     2  otherwise                                        dropped by draw
 * draw(u) = mix64(seed ^ (u * 0x9E3779B97F4A7C15)) >> 32, the multiplication mod 2^64, mix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd;
 * x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33 (csrc/sdt_kmer.cuh).  cov and target are 32-bit: both products fit 64 bits.
 * target == 0 is SDT_EINVAL.
 *   select_reads:   pick[i] for read i of a batch (packed as for sdt_gpu_push_reads): kmers and median as sdt_read_cov, the unit's
 *                   cov, verdict = the class above | 1 << 4 iff THIS read is aberrant on its own.  paired != 0: reads 2t and 2t + 1
 *                   are mates (an odd nreads is SDT_EINVAL).  keep (may be NULL): keep[i] = 1 for verdicts 0 and 1, else 0.
 *                   *n_kept = reads kept.  The batch is staged in pieces as for profile_reads; a piece never splits a pair.
 *   select_reads_device: buffers already on the device (d_pick nreads records, d_keep nreads bytes or NULL); max_read_len as for
 *                   profile_reads_device: a longer read gets kmers = 0xFFFFFFFF, median = cov = 0, verdict 4, keep 0, counts as
 *                   n == 0 for its mate, and the call returns SDT_EINVAL with every other record complete.  The call waits for the
 *                   kernels to know *n_kept.
 *   select_kept_reads: the reads kept in HBM; pick[] by READ ORDINAL like profile_kept_reads (SDT_EFULL, nothing written, when a
 *                   kept read's ordinal is >= out_capacity; records of ordinals that no kept read has are left untouched).
 *                   pair_ranges[2i], pair_ranges[2i + 1] = [first, end) of ordinals that hold interleaved pairs, the first mate at
 *                   first + 2t; ascending, disjoint, of even length, else SDT_EINVAL.  Ordinals outside every range are single
 *                   reads.  A pair of which only one mate is kept in HBM is judged on that mate alone (its id stays the first
 *                   mate's ordinal).  *nreads = reads decided, *n_kept = reads kept.  Mates sit in different kept batches, so the
 *                   call holds the records of ALL ordinals on the device at once: 16 B x (highest kept ordinal + 1) of HBM beside
 *                   the table and the kept reads, SDT_ENOMEM (nothing written) when that does not fit.
 *   compact_reads:  the reads with keep[i] != 0 of a 2-bit stream, packed base-contiguous again in their order: out_offsets has
 *                   *n_out_reads + 1 entries (the caller provides nreads + 1), out_words *n_out_words words and 4 pad words of 0
 *                   after them; the last word is zero past the last base.  SDT_EFULL with *n_out_words (and *n_out_reads) set when
 *                   out_words_cap < *n_out_words + 4; nothing else is valid then.  The host form stages the whole stream at once.
 *                   It needs a context for its stream only: allowed in any state and on any kind of context.
 *   compact_reads_device: buffers on the device; d_out_words must not overlap the input.  The call waits for the kernels.  Its
 *                   outputs are what sdt_gpu_count_reads_device of another context takes (nwords = *n_out_words + 4).
 * The select calls follow the state rules and return codes of the profile calls (nreads == 0: SDT_OK, nothing touched).  Nothing
 * here writes the table or the kept reads.
 *
 * Reads trimmed to their longest solid stretch against the table: what correct_reads cannot fix (two errors closer than K, a
 * candidate with no or several valid alternatives, indels, chimeric junctions) is cut away, so that those k-mers do not go back into
 * pass 1.  Added without a change of SDT_ABI_VERSION: the five calls, the two structs and the flag are additions.  The rule is
 * deterministic, in integers only, decides every read on its own and only reads the table.  A read of L bases has n = L - K + 1
 * k-mers (0 for L < K) with the counts c[j] that profile_reads sees (32-bit, unsaturated, absent = 0; the deleted flag is ignored).
 *     k-mer j is WEAK iff c[j] < min_count (min_count == 0: nothing is weak), SOLID otherwise
 *     median   the lower median of c[], as sdt_read_cov.median;  weak = the weak k-mers of the read as it came
 *     SDT_TRIM_CORRECTED (bit 0 of flags): every run of weak k-mers that sdt_gpu_correct_reads would fix with the same min_count (a
 *              candidate run with exactly one valid alternative) counts as solid from then on.  A substitution at p changes exactly
 *              the k-mers of its own run: the corrected read's weak mask is the original mask with the fixed runs cleared, nothing
 *              more is looked up.  weak and median still describe the read as it came; start and len are in the read's own
 *              coordinates, which a substitution does not shift.
 *     a STRETCH is a maximal run [a, a + s) of solid k-mers; it covers bases [a, a + s + K - 1)
 * The first line that applies decides the read; (start, len) are the kept bases:
 *     4  short     n == 0                                                                          0, 0
 *     0  whole     no weak k-mer is left                                                           0, L
 *     1  gated     min_cov > 0 and median < min_cov (a thin transcript's weak k-mers are not
 *                  evidence of error)                                                              0, L
 *     3  dropped   there is no stretch, or the longest covers fewer than min_len bases             0, 0
 *     2  trimmed   otherwise: the longest stretch, the first among equals                          a, s + K - 1
 * A stretch covers at least K bases: a min_len of K or less never binds.  An unknown bit in flags is SDT_EINVAL.
 *   trim_reads:     trim[i] for read i of a batch (packed as for sdt_gpu_push_reads); keep (may be NULL): keep[i] = len > 0;
 *                   *n_kept = reads with len > 0.  The batch is staged in pieces as for profile_reads.
 *   trim_reads_device: buffers already on the device (d_trim nreads records, d_keep nreads bytes or NULL); max_read_len as for
 *                   profile_reads_device: a longer read gets kmers = 0xFFFFFFFF, the other fields 0, verdict 4, keep 0, and the
 *                   call returns SDT_EINVAL with every other record complete.  The call waits for the kernel to know *n_kept.
 *   trim_kept_reads: the reads kept in HBM, batch by batch; trim[] by READ ORDINAL like profile_kept_reads (SDT_EFULL, nothing
 *                   written, when a kept read's ordinal is >= out_capacity; records of ordinals that no kept read has are left
 *                   untouched).  No pair logic: mates are trimmed independently.  The kept reads are NOT changed.
 *   compact_trimmed: compact_reads with a range per read: read r contributes bases [offsets[r] + start, + len) of trim[r], len == 0
 *                   leaves it out.  Pad, zero tail, SDT_EFULL and the sizes of the outputs as for compact_reads.  start + len
 *                   beyond the read is SDT_EINVAL before anything is staged.  Any state, any kind of context.
 *   compact_trimmed_device: buffers on the device; d_out_words must not overlap the input.  It cannot refuse a range: start and len
 *                   are clamped to the read, nothing outside the stream is read.  Its outputs are what sdt_gpu_count_reads_device
 *                   of another context takes (nwords = *n_out_words + 4).  Both forms read start and len of a record only, and
 *                   sdt_read_clip has them where sdt_read_trim has them: they take an array of sdt_read_clip through a pointer cast.
 * The trim calls follow the state rules and return codes of the profile calls (nreads == 0: SDT_OK, nothing touched).
 *
 * Exact copies of a read or of a read pair dropped (PCR and optical duplicates: they add no k-mer and inflate the counts that -d,
 * min_count and the normalisation's median key on).  Needs NO counted table: it runs before pass 1, and dedup -> compact_reads_device
 * -> count_reads_device goes without a copy to the host.  Added without a change of SDT_ABI_VERSION: the three calls, the two structs
 * and the flag are additions.  The rule is exact, deterministic and independent of any hash function and of the launch geometry.
 *     A UNIT is one read, or the two mates of a pair; its id is the index of its first read (dense forms) or that read's ordinal
 *     (kept form), as for select_reads.  Two reads are EQUAL iff they have the same length and the same bases (two reads of length 0
 *     are equal).  Two units are EQUAL iff they hold the same number of reads and those are equal mate by mate; with
 *     SDT_DEDUP_MATE_SWAP (bit 0 of flags) pairs (a, b) and (c, d) are also equal when a = d and b = c: the same fragment read from
 *     the other strand of an unstranded library.  A single read never equals a pair.  Reverse complements of single reads are NOT
 *     considered (out of scope).  An unknown bit in flags is SDT_EINVAL; reserved is ignored.
 *     Equality partitions the units into CLASSES; the unit with the smallest id of a class is kept, the others are dropped.  Every
 *     read of a unit gets the same record:
 *         first    the smallest unit id of the class (the kept unit's own id)
 *         copies   the units of the class, the same in every record of the class, saturating at 2^32 - 1
 *         verdict  0 kept, 1 dropped
 *   dedup_reads:    dup[i] for read i of a batch (packed as for sdt_gpu_push_reads).  paired != 0: reads 2t and 2t + 1 are mates (an
 *                   odd nreads is SDT_EINVAL).  keep (may be NULL): keep[i] = 1 for verdict 0, else 0; *n_kept = reads kept.  Reads
 *                   depend on each other: the whole stream is staged at once, like compact_reads.
 *   dedup_reads_device: buffers already on the device (d_dup nreads records of 16 bytes, d_keep nreads bytes or NULL).  The call waits
 *                   for the kernels to know *n_kept.  d_keep is what sdt_gpu_compact_reads_device takes.
 *   dedup_kept_reads: the reads kept in HBM, over ALL kept batches at once (mates and copies sit in different batches); dup[] by READ
 *                   ORDINAL like select_kept_reads (SDT_EFULL, nothing written, when a kept read's ordinal is >= out_capacity;
 *                   records of ordinals that no kept read has are left untouched); pair_ranges with the meaning and the checks of
 *                   select_kept_reads.  A pair of which only one mate is kept in HBM is a single-read unit (its id stays the first
 *                   mate's ordinal).  *nreads = reads decided, *n_kept = reads kept.  The kept reads are NOT changed.
 * State: the dense forms need a context for its stream only: any state, any kind of context, like compact_reads.  The kept form
 * needs kept reads, not a table: the rules of sdt_gpu_kept_batches (SDT_ESTATE without kept reads or while pushed batches are not
 * drained).  nreads == 0: SDT_OK, nothing touched.  There is NO limit on the read length: no per-wavefront strip is involved.
 * How: a 64-bit fingerprint per read, of its bases wherever they start in a word; then rounds over the unresolved units: the unit
 * fingerprints go into a hash set, the smallest unit of a slot is its representative, and every other unit of the slot is compared
 * with it base by base: equal: dropped; different (a collision of fingerprints): it meets its own class in the next round, under
 * another salt.  Every round resolves the class of every slot's smallest unit; in practice there is one round.  SDT_ELIMIT, no host
 * output written, past 64 rounds (the device forms' d_dup and d_keep then hold records of resolved units only).
 * Device memory held during the call, beside the reads, SDT_ENOMEM (nothing written) when it does not fit:
 *     the hash set      24 B per slot (fingerprint, representative, copies); slots = the power of two >= 2 x units, < 4 x units
 *     dense forms       8 B per read (its fingerprint); the host form also the stream, 16 B + 1 B per read of records and keep
 *     kept form         per ordinal up to the highest kept one: 24 B (fingerprint, length, where the read's bases start) and the
 *                       16 B record
 *
 * Sequencing adapters and poly-A/T tails clipped from reads: what the library preparation added and no other stage removes.  Adapter
 * k-mers are solid (the same bases recur in many reads), so correct_reads and trim_reads leave them in and they join unrelated
 * transcripts; poly-A k-mers make the giant minimizer bucket; a read-through adapter hides a duplicate from dedup_reads.  Needs NO
 * counted table and no base qualities; clip -> compact_trimmed_device -> dedup -> compact -> count goes without a copy to the host.
 * Added without a change of SDT_ABI_VERSION: the three calls and the three structs are additions.  The rule is deterministic, in
 * integers only, decides every read on its own, reads nothing but the read and the adapter set, and does not depend on the launch
 * geometry or on where a read starts in its word.  Bases are the stream's codes (A 0, C 1, T 2, G 3); a read has L bases r[0, L).
 *     The ADAPTER SET holds n adapters, 0 <= n <= SDT_CLIP_MAX_ADAPTERS, each of 1 .. SDT_CLIP_MAX_ADAPTER_LEN bases, packed like
 *     reads (16 bases per word, the first in the most significant pair) with offsets[n + 1] in bases; ends[i] = 0: a 3' adapter,
 *     1: a 5' adapter.
 *     A 3' adapter a of m bases, at a position p in [0, L): the overlap is o = min(m, L - p), h the number of i < o with
 *              r[p + i] != a[i]; p is a HIT iff o >= min_overlap and 100 h <= max_err_pct o.  The adapter's hit is the smallest such
 *              p: the adapter may continue past the read's end, never past its start.
 *     A 5' adapter, the mirror image, at an end e in (0, L]: o = min(m, e), h the number of i < o with r[e - o + i] != a[m - o + i];
 *              the adapter's hit is the largest e that passes the same two conditions.
 *     Every adapter is judged on the read as it came, independently of the others.  e0 = the smallest 3' hit over all 3' adapters (L
 *              if there is none), s0 = the largest 5' hit over all 5' adapters (0 if none); the adapter that set a bound is the one
 *              of lowest index among equals.  Hamming distance only: no indels, no IUPAC letters.
 *     TAILS are judged on what the adapters left, and only if s0 < e0 (a poly-A tail sits in front of a read-through adapter).  For
 *              a segment [s, e) and a base b the 3' tail of length t is the suffix [e - t, e), x_t the bases != b in it, its score
 *              t - 3 x_t (+1 a match, -2 a mismatch).  t is ADMISSIBLE iff r[e - t] == b and t >= min_tail and
 *              100 x_t <= tail_err_pct t.  The tail is the admissible t of greatest score, the smallest t among equal scores; none
 *              admissible: t = 0.  tail3_bases is a mask, bit b makes base b eligible; over the eligible bases the longest tail
 *              wins: t3, on [s0, e0).  The 5' tail is the mirror image (prefixes, r[s + t - 1] == b), judged on [s0, e0 - t3) with
 *              tail5_bases: t5.
 *     start = s0 + t5, len = max(0, e0 - t3 - start).  The first line that applies:
 *         3  dropped   len < max(min_len, 1)                        record: start = len = 0
 *         0  whole     len == L                                             start = 0, len = L
 *         2  clipped   otherwise                                            start, len as computed
 *     (1 and 4 stay unused: 0, 2 and 3 mean what they mean in sdt_read_trim.)  The record of a dropped read still says what was
 *     found: adapters = (1 + index of the 3' adapter that set e0, or 0) | (1 + index of the 5' adapter that set s0, or 0) << 16;
 *     tail3, tail5 = the bases the tail rules removed.
 *     Defaults of the command line: min_overlap 5, max_err_pct 10, min_tail 10, tail_err_pct 20.  Short overlaps hit by chance: of
 *     20 000 random reads of 150 bases, 251 were touched under three adapters, min_overlap 5, 10 %, tails A at 3' and T at 5',
 *     min_tail 6 and 20 %.  That is a property of the parameters, not a fault; raise min_overlap or min_tail to lose fewer bases.
 *   clip_reads:     clip[i] for read i of a batch (packed as for sdt_gpu_push_reads); keep (may be NULL): keep[i] = len > 0;
 *                   *n_kept = reads with len > 0.  The batch is staged in pieces as for profile_reads.
 *   clip_reads_device: buffers already on the device (d_clip nreads records of 24 bytes, d_keep nreads bytes or NULL).  The adapter
 *                   set is given through HOST pointers here too: it is small, and the call copies it to the device.  The call waits
 *                   for the kernel to know *n_kept.  d_clip is what sdt_gpu_compact_trimmed_device takes.
 *   clip_kept_reads: the reads kept in HBM, batch by batch; clip[] by READ ORDINAL like trim_kept_reads (SDT_EFULL, nothing written,
 *                   when a kept read's ordinal is >= out_capacity; records of ordinals that no kept read has are left untouched).
 *                   No pair logic: mates are clipped independently.  The kept reads are NOT changed.
 * State: the dense forms need a context for its stream only: any state, any kind of context, like dedup_reads.  The kept form
 * follows the rules of sdt_gpu_kept_batches.  nreads == 0: SDT_OK, nothing touched.  There is NO limit on the read length: no
 * per-wavefront strip is involved (start and len are 32-bit, as in sdt_read_trim).  NULL adapters means n = 0.
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: flags != 0;
 * min_overlap == 0; max_err_pct or tail_err_pct > 100; a tail mask > 15; min_tail == 0 while a tail mask is set; n > 256; an
 * adapter of 0 or of more than 128 bases; an adapter shorter than min_overlap (it could never hit); adapter offsets that are not
 * monotonic; ends[i] > 1; NULL params.
 * Out of scope: base qualities and quality trimming (the streams have none); indels in the adapter alignment; IUPAC letters;
 * adapter detection from mate overlap (that is overlap_pairs, below: it runs in front of clip and needs no adapter list);
 * reverse-complement variants of an adapter (the user lists them as adapters of their own); clipping inside pass 1 itself.
 *
 * The overlap of the two mates of a pair, and read-through pairs clipped without an adapter list.  When a fragment is shorter than
 * the read, both mates run through into adapter; with the wrong adapter file, or a custom kit, clip_reads leaves those bases in.
 * The two mates carry the proof themselves: mate 2 reverse-complemented lies on mate 1, and everything past the fragment's end is
 * not transcript.  A pair that overlaps also gives the library's fragment length (avg_ins of the library config).  Needs NO counted
 * table, no adapter list and no base qualities; overlap -> compact_trimmed_device -> clip -> ... -> count goes without a copy to the
 * host.  Added without a change of SDT_ABI_VERSION: the three calls and the two structs are additions.
 *     Integers only.  Every pair is decided on its own.  Nothing is read but the two mates.  The result does not depend on the launch
 *     geometry or on where a read starts in its word.
 *     Bases are the stream's codes (A 0, C 1, T 2, G 3), so the complement of code x is x ^ 2.
 *     A pair is (a, b): a of La bases, b of Lb bases.  b' is the reverse complement of b: b'[q] = b[Lb - 1 - q] ^ 2.
 *     SHIFT.   Putting b'[0] under a[d] is the shift d, -Lb < d < La.  Its insert (the fragment length it implies) is F = d + Lb >= 1.
 *              Its columns are i in [max(0, d), min(La, d + Lb)).  o is their number.  h is the number of columns with
 *              a[i] != b'[i - d].
 *     ADMISSIBLE.  d is ADMISSIBLE iff o >= min_overlap and 100 h <= max_err_pct o.
 *     THE PAIR'S OVERLAP is the admissible shift of greatest score o - 3 h (+1 a match, -2 a mismatch, the scoring of clip's tails).
 *              Among equal scores the greatest F wins (the one that clips least).  If no shift is admissible, there is no overlap.
 *     KEPT BASES.  With an overlap of insert F, every mate keeps start = 0, len = min(L, F).  Whatever a read holds past the
 *              fragment's end is adapter, on either mate and for unequal mate lengths alike.  Without an overlap, len = L.
 *     VERDICT, with the numbers of sdt_read_trim; the first line that applies:
 *         3  dropped   len < max(min_len, 1)                        record: start = len = 0
 *         0  whole     len == L
 *         2  clipped   otherwise
 *     RECORD.  Both mates get overlap = o, mismatches = h, insert = F of the chosen shift (all 0 without one).  A dropped read's
 *              record still says what was found.  Mates are judged for min_len independently, as in clip.
 *     SINGLE READS.  The kept form's ordinals outside every pair range, and a pair of which one mate is not kept in HBM, get the
 *              record of a pair without overlap.
 *     Defaults of the command line: min_overlap 30, max_err_pct 10, min_len 0.  Chance hits, by brute force on the CPU: of 3 000
 *     pairs of random 150-base reads, none had an admissible shift at min_overlap 12, 16, 20 or 30 under 10 %.
 *   overlap_pairs:  ov[i] for read i of a batch (packed as for sdt_gpu_push_reads) in which reads 2t and 2t + 1 are mates; keep (may
 *                   be NULL): keep[i] = len > 0; *n_kept = reads with len > 0.  The batch is staged in pieces of whole pairs.
 *   overlap_pairs_device: buffers already on the device (d_ov nreads records of 24 bytes, d_keep nreads bytes or NULL).  The call
 *                   waits for the kernel to know *n_kept.  d_ov is what sdt_gpu_compact_trimmed_device takes: start, len and verdict
 *                   sit where sdt_read_trim has them, so both compaction calls take an array of sdt_read_overlap through a pointer cast.
 *   overlap_kept_pairs: the reads kept in HBM, over ALL kept batches at once (mates sit in different batches); ov[] by READ ORDINAL
 *                   like dedup_kept_reads (SDT_EFULL, nothing written, when a kept read's ordinal is >= out_capacity; records of
 *                   ordinals that no kept read has are left untouched); pair_ranges with the meaning and the checks of
 *                   select_kept_reads.  *nreads = reads decided, *n_kept = reads with len > 0.  The kept reads are NOT changed.
 * State: the dense forms need a context for its stream only: any state, any kind of context, like dedup_reads.  The kept form
 * follows the rules of sdt_gpu_kept_batches.  nreads == 0: SDT_OK, nothing touched.  There is NO limit on the read length: a
 * wavefront walks the shifts 64 at a time (start, len and insert are 32-bit, as in sdt_read_trim).
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: flags != 0;
 * min_overlap == 0; max_err_pct > 100; NULL params; an odd nreads in the dense forms; pair ranges that select_kept_reads refuses.
 * Device memory held during the call, beside the reads, SDT_ENOMEM (nothing written) when it does not fit:
 *     device form       8 B (the counter of the reads kept)
 *     host form         the piece of the stream that is staged, and 24 B + 1 B per read of it for records and keep
 *     kept form         per ordinal up to the highest kept one: 24 B (where the read's bases start and its length: the entry of
 *                       dedup_kept_reads) and the 24 B record; 24 B per stretch of units (at most 2 x n_ranges + 1)
 * Out of scope: merging the mates into one read; correcting mismatching bases in the overlap (needs qualities); indels; overlaps in
 * which mate 2 is not reverse-complemented; any change to clip.
 *
 * Low-complexity reads flagged, dropped or trimmed: reads, or parts of reads, that are homopolymers, di- or tri-nucleotide repeats, or
 * runs of N (the 2-bit stream cannot show N: the host codes it as G, so a run of N arrives as poly-G, and nothing downstream can tell
 * a called G-run from an N-run).  clip_reads removes tails at the ends only; internal poly-A, (AC)n and poly-G runs still reach the
 * table, where their k-mers make the giant minimizer buckets of pass 1, and, being solid (they recur across transcripts),
 * correct_reads and trim_reads leave them in and they join unrelated transcripts in the graph.  Needs NO counted table, no base
 * qualities and no pair logic; overlap -> compact_trimmed -> clip -> compact_trimmed -> complexity -> compact_trimmed -> dedup ->
 * compact -> count goes without a copy to the host.  Added without a change of SDT_ABI_VERSION: the three calls and the two structs
 * are additions.
 *     Integers only.  Every read is decided on its own.  Nothing is read but the read.  The result does not depend on the launch
 *     geometry or on where a read starts in its word.  Bases are the stream's codes (A 0, C 1, T 2, G 3); a read has L bases r[0, L).
 *     WINDOWS.  W = 0 for L = 0, else W = max(1, ceil(L / 32) - 1).  Window j is [32 j, min(32 j + 64, L)), with m_j bases and
 *              l_j = max(0, m_j - 2) triplets (r[i], r[i + 1], r[i + 2]).  So L = 150 gives [0,64) [32,96) [64,128) [96,150), L = 64
 *              one window, L = 65 two, and the last window always has more than 32 bases unless it is the only one.  With c_t the
 *              number of the window's triplets of kind t (64 kinds), D_j = sum over t of c_t (c_t - 1): the number of ordered pairs
 *              of equal triplets, 0 <= D_j <= l_j (l_j - 1).
 *     LOW.     Window j is LOW iff l_j >= 2 and 100 D_j >= max_score_pct l_j (l_j - 1).
 *     SCORE.   The read's score is the maximum over the windows with l_j >= 2 of floor(100 D_j / (l_j (l_j - 1))); without such a
 *              window it is 0.  A homopolymer scores 100.
 *     LOW BASES.  A base is low iff a LOW window covers it; B is the number of low bases.  The clean stretch is the longest run of
 *              bases that are not low, the first among equals: (s, n), n = 0 if all are low.
 *     KEPT RANGE.  flags = 0 (filter): start = 0, len = L, unless 100 B > max_low_pct L, in which case len = 0.
 *              SDT_COMPLEXITY_TRIM: start = s, len = n; max_low_pct must be 0.
 *     VERDICT, with the numbers of sdt_read_trim; the first line that applies:
 *         3  dropped   len < max(min_len, 1)                        record: start = len = 0
 *         0  whole     len == L
 *         2  clipped   otherwise
 *     RECORD.  windows = W, low = the number of LOW windows, score; start, len and verdict sit where sdt_read_trim has them.  A
 *              dropped read's record still says what was found.
 *     What the score does, on the CPU (numpy, seed 1): repeats of period 1 / 2 / 3 / 4 / 6 fill a 64-base window with scores
 *     100 / 49 / 32 / 23 / 15.  A random window has mean score 1.56 at every length; of 200 000 random 64-base windows none reached
 *     7 (the maximum was 5.6); of 200 000 random 33-base windows 46 (0.02 %) reached 7 and 6 (0.003 %) reached 10.  Of 20 000
 *     random reads, those with a LOW window at max_score_pct 10 / 7 / 5: L = 150: 0 / 0 / 6; L = 100: 0 / 3 / 28; L = 97: 0 / 3 / 35
 *     (the short last window is where chance hits).  A run planted at base 60 of 200 random 150-base reads, at 10: poly-A of 20
 *     bases alone scores 8 (18 triplets of 62: 306 of 3 782) and passes; with what chance adds the median score was 9 and 77 reads
 *     had a low window.  Poly-A of 25 bases: median 15, one window low in 92 reads and two in 108.  Poly-A of 30 bases: median 21,
 *     both covering windows low in all 200.  (AC)n of 30 bases: median 11, a low window in 182 reads.  A run that falls into a short
 *     last window weighs more: 20 bases of poly-A in a window of 54 score 11.
 *     Hence the defaults of the command line: max_score_pct 10, max_low_pct 50, min_len 0.  The 50 is a choice, not a measurement:
 *     a 150-base read with one 30-base internal run has 96 of its 150 bases low and is dropped under it.  Known coarseness: a low
 *     window is low as a whole, so under SDT_COMPLEXITY_TRIM it removes all 64 of its bases.
 *   complexity_reads: cx[i] for read i of a batch (packed as for sdt_gpu_push_reads); keep (may be NULL): keep[i] = len > 0;
 *                   *n_kept = reads with len > 0.  The batch is staged in pieces as for profile_reads.
 *   complexity_reads_device: buffers already on the device (d_cx nreads records of 24 bytes, d_keep nreads bytes or NULL).  The call
 *                   waits for the kernel to know *n_kept.  d_cx is what sdt_gpu_compact_trimmed_device takes: both compaction calls
 *                   take an array of sdt_read_complexity through a pointer cast.
 *   complexity_kept_reads: the reads kept in HBM, batch by batch; cx[] by READ ORDINAL like trim_kept_reads (SDT_EFULL, nothing
 *                   written, when a kept read's ordinal is >= out_capacity; records of ordinals that no kept read has are left
 *                   untouched).  SDT_ESTATE when batches were pushed and sdt_gpu_finish_count has not drained them, whether
 *                   their copies are still queued or they are counted and not yet synchronised.  *nreads = reads decided.  Mates are judged
 *                   independently.  The kept reads are NOT changed.
 * State: the dense forms need a context for its stream only: any state, any kind of context, like dedup_reads.  The kept form
 * follows the rules of sdt_gpu_kept_batches and is stricter in one: it alone of the kept forms that need no table also refuses
 * batches that are counted and not yet synchronised (above), as the forms on the counted table do; the others (fetch_kept_batch,
 * dedup_, clip_, overlap_, merge_, screen_) refuse only batches whose launch is still queued.  nreads == 0: SDT_OK, nothing
 * touched.  There is NO limit on the read length: a wavefront walks a read one window at a time (windows, low, start and len are 32-bit, as in sdt_read_trim).
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: NULL params; flag bits
 * other than SDT_COMPLEXITY_TRIM; max_score_pct 0 (every window would be low) or > 100; max_low_pct > 100; max_low_pct != 0 under
 * SDT_COMPLEXITY_TRIM.
 * Device memory held during the call, beside the reads, SDT_ENOMEM (nothing written) when it does not fit:
 *     device form       8 B (the counter of the reads kept)
 *     host form         the piece of the stream that is staged, and 24 B + 1 B per read of it for records and keep
 *     kept form         the 24 B records of the largest kept batch
 * Out of scope: entropy or other scores; masking bases inside a kept read (the stream has no N); more than one kept stretch per read;
 * a window other than 64 bases every 32; pair-aware decisions (mates are judged independently, as in clip; the command line routes
 * the survivors); any change to clip, overlap or pass 1.
 *
 * Reads trimmed and filtered by their base qualities: the first stage of the chain and the only one that reads qualities.  The bases a
 * sequencer was unsure of are where the error k-mers come from; correct_reads and trim_reads can deal with those only after a whole
 * count.  It is also the only stage that can see an N: the 2-bit stream codes N as G, but sequencers give N a quality of 2, so a run
 * of N is cut at the ends of a read and counted as low bases inside it.  Needs NO counted table and does NOT look at the bases.
 * Qualities are only valid while the offsets are those of the input, so the stage goes first:
 * quality -> compact_trimmed_device (on the 2-bit words, same offsets) -> overlap -> ...; NO later stage carries qualities along.
 * Added without a change of SDT_ABI_VERSION: the two calls and the two structs are additions.
 *     Integers only.  Every read is decided on its own.  Nothing is read but the read's own quality bytes.  The result does not
 *     depend on the launch geometry or on where a read starts in memory.
 *     INPUT.   quals: one byte per base, under the same offsets[nreads + 1] (in bases, here: in bytes) as the read's 2-bit stream.
 *              Read r has L = offsets[r + 1] - offsets[r] bytes c[0, L).  The quality of base i is q_i = 0 if c_i < phred_offset,
 *              else min(c_i - phred_offset, 93).
 *     SEGMENT (Mott's rule, as `seqtk trimfq` and `phred` use it).  s_i = q_i - cut_q; P_0 = 0, P_j = s_0 + ... + s_(j-1).  The kept
 *              segment is the [a, b), 0 <= a <= b <= L, with the greatest P_b - P_a; among equal sums the smallest a wins, among
 *              those the greatest b.  So all s_i < 0 gives a = b = 0; cut_q = 0 keeps the whole read (trimming is off); a base
 *              with q_i = cut_q at the edge of the segment is kept.  Equivalent form, the one a scan computes: for every b,
 *              M_b = min over a <= b of P_a and a_b the smallest a that attains it; take the b that is greatest under the key
 *              (P_b - M_b descending, a_b ascending, b descending).
 *     MEASURES of the segment, n = b - a.  low = the bases of [a, b) with q_i < low_q.  E = the sum over [a, b) of e[q_i], in
 *              millionths of an expected error: e[q] = 10^6 * 10^(-q / 10) rounded to the nearest integer (94 entries; e[0] =
 *              1 000 000, e[1] = 794 328, e[3] = 501 187, e[20] = 10 000, e[30] = 1 000, e[60..63] = 1, e[64..93] = 0; no entry is
 *              a tie), summed in 64 bits.  ee_ppm = floor(E / n), 0 for n = 0: expected errors per million bases, 10^6 at most.
 *     VERDICT, with the numbers of sdt_read_trim; the first line that applies:
 *         3  dropped   n < max(min_len, 1)                          record: start = len = 0
 *         3  dropped   100 low > max_low_pct n                      record: start = len = 0
 *         3  dropped   max_ee_ppm != 0 and ee_ppm > max_ee_ppm      record: start = len = 0
 *         0  whole     n == L                                       record: start = 0, len = L
 *         2  clipped   otherwise                                    record: start = a, len = n
 *     RECORD.  sdt_read_quality: span = n, low, ee_ppm; start, len and verdict sit where sdt_read_trim has them.  A dropped read's
 *              record still says what was found: from span, low, ee_ppm and the parameters anyone can tell which line dropped it.
 *     PARAMETERS.  max_low_pct = 100 or low_q = 0: the low-base filter is off.  max_ee_ppm = 0: the expected-error filter is off.
 *     The defaults of the command line are phred_offset 33, cut_q 20, low_q 15, max_low_pct 40, max_ee_ppm 0, min_len 0: the usual
 *     figures of `fastp` and `cutadapt`.  They are a choice, not a measurement.
 *   quality_reads:  out[i] for read i of a host batch of nbytes quality bytes; keep (may be NULL): keep[i] = len > 0; *n_kept = reads
 *                   with len > 0.  The batch is staged in pieces as for profile_reads, each from a 4-byte-aligned byte of the stream.
 *   quality_reads_device: buffers already on the device: d_quals 4-byte aligned and readable up to offsets[nreads] rounded up to 4
 *                   (bytes outside the reads never change a result), d_out nreads records of 24 bytes, d_keep nreads bytes or NULL.
 *                   The call waits for the kernel to know *n_kept.  d_out is what sdt_gpu_compact_trimmed_device takes: both
 *                   compaction calls take an array of sdt_read_quality through a pointer cast.
 * State: a context is needed for its stream only: any state, any kind of context, like dedup_reads.  nreads == 0: SDT_OK, nothing
 * touched, whatever the rest says.  There is NO limit on the read length: a wavefront walks a read 256 bases at a time (span, start
 * and len are 32-bit, as in sdt_read_trim).
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: NULL params;
 * phred_offset other than 0, 33 or 64; cut_q > 93; low_q > 93; max_low_pct > 100; flags != 0; reserved != 0.  The host form also:
 * offsets that are not monotonic, nbytes < offsets[nreads].  The device form also: d_quals not 4-byte aligned.
 * Device memory held during the call, beside the qualities, SDT_ENOMEM (nothing written) when it does not fit:
 *     device form       8 B (the counter of the reads kept)
 *     host form         the piece of the stream that is staged with its offsets, and 24 B + 1 B per read of it for records and keep
 * Out of scope: sliding-window cuts; per-end thresholds; masking bases; qualities carried through later stages or written out (the
 * outputs stay FASTA like every other stage's); a kept form (the reads kept in HBM carry no qualities, and sdt_gpu_keep_reads is
 * not changed); pair-aware decisions (mates are judged independently; the command line routes the survivors); any change to another
 * stage.
 *
 * Reads screened against reference sequences one already knows: ribosomal RNA, the PhiX spike-in, a mitochondrial genome, vectors or a
 * host.  Their k-mers are the most abundant solid k-mers of the table, so correct_reads and trim_reads leave them alone, select_reads
 * spends its budget on them and they make the deepest buckets of pass 1.  The stage drops the reads that hit a reference, or, as a
 * bait, keeps only those.  It needs NO counted table and has a k of its own: a small hash set on the device, canonical k-mer ->
 * reference, loaded once and kept by the context.  ... -> clip -> compact -> screen -> compact -> complexity -> dedup -> count goes
 * without a copy to the host.  Added without a change of SDT_ABI_VERSION: the seven calls and the two structs are additions.
 *     Integers only.  Every unit is decided on its own.  The result does not depend on the launch geometry, on any hash function or on
 *     where a read starts in its word.  Bases are the stream's codes (A 0, C 1, T 2, G 3), the complement is x ^ 2, and the canonical
 *     form of a k-mer is the smaller of itself and its reverse complement as a right-aligned integer.  11 <= k <= 31, even k included.
 *     SET.     nseqs sequences packed like reads (16 bases per word, the first in the most significant pair, offsets[nseqs + 1] in
 *              bases, the pad words of sdt_gpu_push_reads behind them), sequence i with ref_of_seq[i] < n_refs.  Several sequences may
 *              carry one reference: the caller cuts a reference at every letter that is not A, C, G or T, so that no k-mer spans one.
 *              A sequence of fewer than k bases contributes nothing; a sequence has NO length limit.  The set is the set of the
 *              canonical k-mers of all sequences; ref(x) of a k-mer x of the set is the SMALLEST ref_of_seq among the sequences that
 *              hold x or its reverse complement: references listed first win.  The set is a pure function of the input, not of the
 *              order of the sequences.
 *     READ.    L bases: kmers = max(L - k + 1, 0); hits = the positions whose canonical k-mer is in the set; ref = the smallest ref(x)
 *              over the hits, 0xFFFFFFFF without one.  MATCHED iff hits >= max(min_hits, 1) and 100 hits >= min_hit_pct kmers (in 64
 *              bits).  A read and its reverse complement get the same kmers, hits, ref and state.
 *     UNIT.    A read, or under paired != 0 the mates 2t and 2t + 1 (an odd nreads is SDT_EINVAL).  A unit is matched iff one of its
 *              reads is.  flags = 0: a matched unit is dropped; SDT_SCREEN_KEEP_MATCHED: an unmatched unit is dropped.  Every read of
 *              a unit gets the unit's verdict, 0 kept or 1 dropped, and keeps its own kmers, hits and ref.
 *     RECORD.  sdt_read_screen: kmers, hits, ref; start = 0, len = L if kept, else 0; start, len and verdict sit where sdt_read_trim
 *              has them, so both compaction calls take the records through a pointer cast, and keep[i] = (verdict == 0) is what
 *              sdt_gpu_compact_reads_device takes.
 *     An N inside a read is a G in the stream, as everywhere else.  The default of the command line, k = 31, is bbduk's usual figure:
 *     a choice, not a measurement.
 *   screen_load:    builds the set on the device and waits for it; *n_kmers (may be NULL) = its distinct k-mers.  The set belongs to
 *                   the context, of any kind and in any state (it needs the stream only): sdt_gpu_destroy frees it, sdt_gpu_reset and
 *                   the counting calls do not touch it.  A second load replaces it, but only once the new one is complete.  SDT_EINVAL
 *                   with the previous set kept: k outside 11 .. 31; n_refs = 0 or a ref_of_seq >= n_refs; offsets that are not
 *                   monotonic or packed_words too short (as for reads); a set without a single k-mer.  SDT_ENOMEM also leaves the
 *                   previous set.
 *   screen_unload:  frees the set (SDT_OK without one).
 *   screen_info:    info = { k, n_refs, distinct k-mers, slots of the table }, all 0 without a set.
 *   screen_lookup:  refs[i] = ref(keys[i]) for right-aligned k-mers of either strand, 0xFFFFFFFF: absent (also for a key of more than
 *                   2 k bits).  n == 0: SDT_OK.
 *   screen_reads:   out[i] for read i of a host batch; keep (may be NULL); *n_kept = reads kept.  The batch is staged in pieces as for
 *                   profile_reads, mates in one piece.
 *   screen_reads_device: buffers already on the device (d_out nreads records of 24 bytes, d_keep nreads bytes or NULL).  The call
 *                   waits for the kernel to know *n_kept.
 *   screen_kept_reads: the reads kept in HBM, in every respect like sdt_gpu_dedup_kept_reads: records by READ ORDINAL, pair_ranges
 *                   with the meaning and the checks of select_kept_reads, mates may sit in different kept batches, a pair with one
 *                   mate kept is a single-read unit, SDT_EFULL (nothing written) when a kept read's ordinal is >= out_capacity,
 *                   SDT_ESTATE without kept reads or while pushed batches are not drained.  Records of ordinals that no kept read has
 *                   are left untouched.  The kept reads are NOT changed.
 * State: screening or looking up without a set is SDT_ESTATE.  nreads == 0: SDT_OK, nothing touched, whatever the rest says.  There is
 * NO limit on the read length in any form: a wavefront walks a unit 64 k-mer positions at a time (kmers, hits and len are 32-bit).
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: NULL params;
 * min_hit_pct > 100; a flag other than SDT_SCREEN_KEEP_MATCHED; reserved != 0; an odd nreads under paired.
 * Device memory: the set is 16 B per slot, slots = the power of two >= 2 x the k-mer positions of the set (1 024 at least); during a
 * load also the staged sequences, their offsets and 4 B per sequence, and the previous set until the new one is complete.  A call:
 *     device form       8 B (the counter of the reads kept)
 *     host form         the piece of the stream that is staged, and 24 B + 1 B per read of it for records and keep
 *     kept form         the 24 B records of the largest kept batch (the unit verdicts are taken on the host)
 * Out of scope: Hamming-distance or IUPAC matching; masking the matching bases instead of dropping the read; attribution by majority
 * vote; k above 31; sets larger than device memory; any change to another stage.
 *
 * The two mates of an overlapping pair merged into one fragment read, and base qualities carried through one compaction.  These are
 * the two things that the overlap stage and the quality stage list as out of scope ("merging the mates into one read; correcting
 * mismatching bases in the overlap (needs qualities)", "NO later stage carries qualities along"): they went here.  An overlapping
 * pair puts every base of its overlap into pass 1 twice, once per strand, with independent errors, which inflates the counts of short
 * fragments only; and the second read pass links edges within one read, so a merged fragment crosses junctions that neither mate
 * crosses.  Needs NO counted table.  quality -> compact_trimmed_device + compact_quals_trimmed_device -> overlap -> merge (with the
 * qualities) -> compact_trimmed_device of the merge records for the rest goes without a copy to the host.  Added without a change of
 * SDT_ABI_VERSION: the five calls, the two structs and SDT_MERGE_MERGED are additions.
 *     Integers only.  Every pair is decided on its own.  Nothing is read but the two mates, their two overlap records and, if given,
 *     their quality bytes.  The result does not depend on the launch geometry, on where a read starts in its word, or on where the
 *     merged read starts in the output's word.  Bases are the stream's codes (A 0, C 1, T 2, G 3).  b' is the reverse complement of
 *     b: b'[q] = b[Lb - 1 - q] ^ 2.
 *     INPUT.   The 2-bit stream and its offsets as for overlap_pairs; ov, the sdt_read_overlap records of the same reads as
 *              overlap_pairs wrote them; optionally quals, one byte per base under the same offsets, exactly the input of
 *              sdt_gpu_quality_reads, or NULL.  The stage does not search for an overlap: it acts on the record, as compact_trimmed
 *              acts on a trim record.
 *     MERGEABLE.  Pair t has mates a = read 2t of La bases and b = read 2t + 1 of Lb bases, Fa = ov[2t].insert, Fb = ov[2t + 1].insert.
 *              With F = Fa the pair is MERGED iff all of these hold:
 *                  Fa == Fb
 *                  1 <= F < La + Lb       (every shift d = F - Lb with -Lb < d < La: at least one column exists unless a mate has
 *                                          no bases, and every position of [0, F) is covered by a or by b'; checked on the CPU for
 *                                          more than 825 combinations of La, Lb, F)
 *                  max(min_len, 1) <= F
 *                  max_len == 0 or F <= max_len
 *              A pair without overlap (Fa == Fb == 0) is not merged.  Any other record pair that violates one of the first two lines
 *              is INCONSISTENT: the host form and the kept form refuse the whole call with SDT_EINVAL before anything is staged,
 *              with a message that names the pair and the two inserts; the device form cannot read the records on the host, treats
 *              such a pair as not merged and never reads outside the two mates.  A mate that its overlap record dropped for min_len
 *              still takes part: the record's insert decides, not its len.
 *     MERGED READ.  m[0, F), with d = F - Lb.  For position p:
 *                  p < La only (p < d)                       m[p] = a[p]
 *                  p - d in [0, Lb) only (p >= La)           m[p] = b'[p - d]
 *                  both, a[p] == b'[p - d]                   that base
 *                  both, they differ: a MISMATCH COLUMN      without quals: a[p].  With quals: qa is the quality of a's base p, qb
 *                                                            that of b's base Lb - 1 - (p - d), both read as the quality stage reads
 *                                                            them (c < phred_offset gives 0, else min(c - phred_offset, 93)).  If
 *                                                            qb > qa the base is b'[p - d] and the column counts in from_b; otherwise
 *                                                            it is a[p].  A tie goes to mate 1.
 *     RECORD.  One sdt_read_merge per READ; both mates get the same first three fields.  merged = F if merged, else 0.  mismatches =
 *              the mismatch columns, recounted by this stage, 0 if not merged.  from_b as above.  start, len and verdict sit where
 *              sdt_read_trim has them and say what is left of this read in the stream of UNMERGED reads: for a merged pair
 *              start = len = 0 and verdict = 5 (SDT_MERGE_MERGED); for every other read the start, len and verdict of its overlap
 *              record, copied.  So the records go to sdt_gpu_compact_trimmed / _device as they are, and what comes out is the stream
 *              of the pairs that did not merge.
 *     MERGED STREAM.  Output read j is the j-th merged pair in ascending pair index (kept form: ascending ordinal of the first mate),
 *              packed like any stream: 16 bases per word, the first base in the most significant pair, out_offsets[n_merged + 1] from
 *              0, the tail bits zero and the pad words of sdt_gpu_push_reads (zero) behind.  It is what sdt_gpu_count_reads_device of
 *              another context, dedup_reads_device(paired = 0) and the other dense forms take.  (offsets[nreads] - offsets[0] + 15) /
 *              16 + 4 words always suffice for out_words, nreads / 2 + 1 entries for out_offsets.
 *     SINGLE READS.  The kept form's ordinals outside every pair range, and a pair of which one mate is not kept in HBM, get their
 *              overlap record's start, len and verdict copied and are never merged.
 *     Defaults of the command line: min_len 0, max_len 0 (no limit), phred_offset 33.
 *   merge_pairs:    mg[i] for read i of a host batch in which reads 2t and 2t + 1 are mates; quals (may be NULL) holds offsets[nreads]
 *                   bytes.  The whole stream is staged at once, like compact_reads, because the output of pieces would meet in the
 *                   middle of words.  SDT_EFULL with *n_merged and *n_out_words set, and nothing written or staged, when
 *                   out_words_cap < *n_out_words + 4.
 *   merge_pairs_device: buffers already on the device: d_ov and d_mg nreads records of 24 bytes, d_quals NULL or 4-byte aligned,
 *                   d_out_offsets nreads / 2 + 1 words; d_out_words must not overlap the input.  SDT_EFULL as above, nothing written.
 *                   The call waits for the kernels.  d_mg is what sdt_gpu_compact_trimmed_device takes.
 *   merge_kept_pairs: the reads kept in HBM, over ALL kept batches at once like overlap_kept_pairs: ov[] and mg[] by READ ORDINAL
 *                   (SDT_EFULL, nothing written, when a kept read's ordinal is >= out_capacity; records of ordinals that no kept read
 *                   has are neither read nor written); pair_ranges with the meaning and the checks of select_kept_reads.  No
 *                   qualities (the kept reads carry none): a mismatch column takes mate 1's base, phred_offset is ignored.  out_words
 *                   and out_offsets are host arrays of out_words_cap words and out_reads_cap + 1 entries; SDT_EFULL with *n_merged and
 *                   *n_out_words set, and nothing written, when either is short.  *nreads = reads decided.  The kept reads are NOT
 *                   changed.
 *   compact_quals_trimmed: the bytes [offsets[r] + start, + len) of every read r, by the records that compact_trimmed takes (any of
 *                   the 24-byte records of the stages), go to where compact_trimmed, on the same records, puts the read's bases: one
 *                   after the other in read order.  The output offsets are those that compact_trimmed writes and are not written
 *                   again.  *n_out_bytes = the bytes kept; the output is zero-padded to a multiple of 4 bytes, and SDT_EFULL (with
 *                   *n_out_bytes set, nothing written) when out_cap is less than that.  start + len beyond the read is SDT_EINVAL
 *                   before anything is staged, as are offsets that are not monotonic and nbytes < offsets[nreads].
 *   compact_quals_trimmed_device: buffers on the device; d_out_quals 4-byte aligned (SDT_EINVAL otherwise) and not overlapping the
 *                   input: what quality_reads_device and merge_pairs_device require of d_quals.  It cannot refuse a range: start
 *                   and len are clamped to the read, as in compact_trimmed_device.
 * State: the dense forms need a context for its stream only: any state, any kind of context, like dedup_reads.  The kept form
 * follows the rules of sdt_gpu_kept_batches.  nreads == 0: SDT_OK, *n_merged = 0 and out_offsets[0] = 0 if given, nothing else
 * touched.  There is NO limit on the read length: a wavefront walks a fragment 2 048 bases at a time (merged, start and len are
 * 32-bit, as in sdt_read_trim).
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: NULL params; flags != 0;
 * max_len != 0 and max_len < max(min_len, 1); phred_offset other than 0, 33 or 64 when quals are given (ignored when quals is NULL);
 * an odd nreads in the dense forms; the device form: d_quals not 4-byte aligned; pair ranges that select_kept_reads refuses.
 * Device memory held during the call, beside the reads, the records and the output, SDT_ENOMEM (nothing written) when it does not fit:
 *     merge, device form   per pair 4 B (its merged length) and 3 x 8 B (the scans: output offset, rank, place in the scratch), the
 *                          scans' temporary storage, and the scratch stream: 8 B per 32 bases of every merged read, each rounded up,
 *                          with 8 B per merged pair for its place in it
 *     merge, host form     that, the whole staged stream with its offsets, 24 B + 24 B per read for the two kinds of records, the
 *                          qualities if given, and the output
 *     merge, kept form     per ordinal up to the highest kept one: the 24 B entry of dedup_kept_reads and 24 B + 24 B for the two
 *                          kinds of records; 24 B per stretch of units; the device form's scratch per unit; the output
 *     compact_quals_trimmed  8 B per read (the scan) and its temporary storage; the host form also the staged bytes, offsets,
 *                          records and the output
 * Out of scope: qualities of the merged read (the outputs stay FASTA); indels; merging without an overlap record; a kept form with
 * qualities (the kept reads carry none); any change to overlap, quality or the compaction calls.
 *
 * A per-cycle QC report of a read batch: base composition, qualities, lengths, GC and mean quality.  Every stage above is driven by
 * parameters (cut_q, low_q, the tails, the adapters, min_len, the Phred offset); this is the view of the data they act on, before and
 * after a stage: it takes the 24-byte records of any stage as ranges, so the "after" view needs no compaction.  It is the one read
 * stage that is a reduction over the whole batch and not a record per read.  Needs NO counted table.  Added without a change of
 * SDT_ABI_VERSION: the three calls, the struct and the two constants are additions.
 *     Integers only.  Every count is exact.  The result does not depend on the launch geometry, on where a read starts in its word or
 *     byte, or on how a host batch is cut into pieces.
 *     INPUT.   The 2-bit stream and offsets[nreads + 1] in bases as for every read batch (16 bases per word, the first in the most
 *              significant pair, A 0, C 1, T 2, G 3); optionally quals, one byte per base under the same offsets; optionally ranges,
 *              nreads records of 24 bytes of which only start and len, where sdt_read_trim has them, are read; optionally classes,
 *              one byte per read.
 *     COUNTED. Read r is COUNTED iff classes is NULL or classes[r] == class_sel, else PASSED OVER.  It has L = offsets[r + 1] -
 *              offsets[r] bases; its counted bases are [s, s + n): s = 0 and n = L without ranges, s = start and n = len with them.
 *              The device form clamps s and n to the read as sdt_gpu_compact_trimmed_device does, and a read whose range had to be
 *              clamped adds 1 to totals[4]; the host form refuses such a range.  Base i, 0 <= i < n, is the stream's base s + i.
 *     QUALITY of base i, as in sdt_gpu_quality_reads: q = 0 if its byte < phred_offset, else min(byte - phred_offset, 93).
 *     ROW of base i.  C = cycles, R = C + 1 rows.  row = min(i, C); under SDT_QC_FROM_END row = min(n - 1 - i, C).  Row C takes
 *              everything past the C-th cycle.
 *     REPORT.  A flat array of uint64_t of sdt_gpu_qc_report_words(C) = 203 + 99 R words, the sections in this order:
 *                  totals      8       [0] reads counted  [1] of those the empty ones (n = 0; they enter no histogram but len[0])
 *                                      [2] bases counted  [3] reads passed over  [4] ranges clamped (device form only)  [5..7] 0
 *                  base[R][4]  4 R     counted bases by row and code
 *                  qual[R][94] 94 R    counted bases by row and q; untouched when quals is NULL
 *                  len[R]      R       counted reads by min(n, C)
 *                  gc[101]     101     counted reads with n >= 1 by floor(100 (#C + #G) / n)
 *                  meanq[94]   94      counted reads with n >= 1 by floor(sum of q / n); untouched when quals is NULL
 *              For any input: sum base = totals[2]; sum qual = totals[2] with qualities; sum len = totals[0]; sum gc = totals[0] -
 *              totals[1]; for a forward row c < C the sum of base[c][.] is the number of counted reads with n > c.
 *     THE CALL ADDS TO THE REPORT.  The caller zeroes it once; batches, pieces and classes then accumulate, and report(A ++ B) =
 *     report(A) + report(B).
 *   qc_report_words: 203 + 99 (cycles + 1); 0 for cycles = 0 or > SDT_QC_MAX_CYCLES.
 *   qc_reads:       a host batch, staged in pieces as for profile_reads; the qualities of a piece from a 4-byte-aligned byte of the
 *                   stream, with the piece's ranges and classes.  The pieces add into a report on the device, which is added to
 *                   report[] once, after the last piece: on any error report[] is untouched.
 *   qc_reads_device: buffers already on the device: d_quals NULL or 4-byte aligned and readable up to offsets[nreads] rounded up to
 *                   4, d_ranges NULL or nreads records of 24 bytes, d_classes NULL or nreads bytes, d_report 8-byte aligned.  No
 *                   word of the stream and no quality word without a counted base is read.
 *   Both forms wait for their kernels.
 * State: a context is needed for its stream only: any state, any kind of context, like dedup_reads.  nreads == 0: SDT_OK, nothing
 * touched, whatever the rest says.  There is NO limit on the read length: a workgroup walks a read 256 bases at a time per wavefront,
 * and what lies past cycle C is counted in 64 bits.
 * SDT_EINVAL, from a check on the host before any launch, with a message that names the field and its value: NULL params; cycles = 0
 * or > SDT_QC_MAX_CYCLES; phred_offset other than 0, 33 or 64 (also without quals: the check is a pure function of the params); a
 * flag other than SDT_QC_FROM_END; class_sel > 255; reserved != 0.  The host form also: offsets that are not monotonic; nwords or
 * nbytes too short (as for reads and qualities); a range with start + len > L (the message names the read); report_words <
 * sdt_gpu_qc_report_words(cycles).  The device form also: d_quals not 4-byte aligned; d_report not 8-byte aligned.
 * Device memory held during the call, beside the reads, SDT_ENOMEM (nothing written) when it does not fit:
 *     device form       none
 *     host form         the piece of the stream that is staged with its offsets, its quality bytes, 24 B + 1 B per read of it for
 *                       ranges and classes where given, and a report-sized buffer (8 B x (203 + 99 R), 3.2 MB at most)
 * Out of scope: a kept form (the reads kept in HBM carry no qualities); duplication levels (dedup has them); adapter content (clip has
 * it); over-represented sequences; per-tile statistics; HTML or plots; any change to another stage or to the parser.
 *
 * An assembly scored against the counted table.  search_kmers answers k-mer -> count and profile_reads reads -> coverage; this is the
 * other direction: which nodes of the table does a set of sequences (contigs, transcripts, scaffolds cut at their N runs) cover, and
 * how often -- what KAT comp / spectra-cn and Merqury compute: how much of the reads' solid k-mer content the assembly holds
 * (completeness), how much of the assembly has no read support (errors, chimeric junctions, a consensus QV), and how many times the
 * assembly holds each read k-mer (collapsed or duplicated isoforms).  Needs the counted table, and writes nothing to it.  Added
 * without a change of SDT_ABI_VERSION: the five calls, the two structs and the two constants are additions.
 *     Integers only.  Everything is exact and does not depend on the order of the sequences, on how they are split over adds or
 *     pieces, on where a sequence starts in its word, or on the launch geometry.
 *     An ASSEMBLY is a set of sequences packed as for sdt_gpu_push_reads (words, offsets[nseqs + 1] in bases), of any length.
 *     A sequence of L bases has n = L - K + 1 k-mers (0 for L < K).  k-mer j has the count c[j] that profile_reads sees: the
 *     canonical k-mer looked up, the 32-bit count with its high half, absent = 0, the deleted flag ignored.  k-mer j is WEAK iff
 *     c[j] < max(min_count, 1).  A GAP is a maximal run of weak k-mers.
 *     RECORD, per sequence (sdt_seq_support, 32 bytes):
 *         kmers  n                            found   the j with a node               solid  the j that are not weak
 *         sum    the sum of c[j], 64 bits     gaps    the number of gaps
 *         longest_gap  the length of the longest gap, 0 if none
 *         longest_at   its first k-mer, the first among equals; kmers if there is none
 *     L < K: kmers = 0, longest_at = 0, every other field 0.
 *     COPY NUMBER.  Per node of the table cn is kept: the k-mer occurrences in all sequences added since asm_begin whose canonical
 *     form is that node, saturating at 255.  Both strands feed the same node; a palindrome of even K counts once per occurrence.
 *     SPECTRUM.  A matrix of rows x SDT_ASM_CN_COLS uint64_t: m[r][c] = the occupied slots with min(count, rows - 1) = r and
 *     min(cn, 7) = c.  Row 0 holds whatever nodes have a count of 0; none is special-cased, and deleted nodes are counted like others.
 *     TOTALS, uint64_t[4], kept on the device over all adds: sequences, k-mers, found, solid.
 *   asm_begin:      allocates one byte per table slot (rounded up to 4), owned by the context, and zeroes it and the totals; params
 *                   are kept for the adds and the spectrum.  A second begin starts over.
 *   asm_add:        a host batch, staged in pieces as for profile_reads; out NULL: tally only, else nseqs records.  Waits.
 *   asm_add_device: buffers already on the device; d_out NULL or nseqs records of 32 bytes, 8-byte aligned.  Asynchronous on the
 *                   context's stream.  A sequence has fewer than 2^32 bases (the host form checks it).
 *   asm_spectrum:   any number of times between adds; matrix (rows x 8, as given to asm_begin) and totals, either may be NULL, not
 *                   both.  Waits.
 *   asm_end:        frees the tally (sdt_gpu_destroy does too).  Without a begin: SDT_OK.
 * There is NO limit on the length of a sequence in either form: a wavefront walks a sequence 64 k-mer positions at a time and keeps
 * no count of it but the record's sums, where profile_reads holds a sequence's counts in LDS (16 384 k-mers at most).
 * nseqs == 0: SDT_OK, nothing touched, whatever the rest says.
 * SDT_ESTATE: asm_begin under the state rules of search_kmers, with its messages (a SDT_FLAG_CONTIG_INDEX context, a shard, after
 * load_paths / import_paths, a released table, batches pushed and not drained); asm_add and asm_spectrum without a begin, after
 * asm_end, and once the table has changed since asm_begin (counted into, grown, reset, imported, released, path words loaded):
 * "the table changed since sdt_gpu_asm_begin" -- a tally is by slot and is never read against another table.
 * SDT_EINVAL, before any launch: NULL params; rows < 2 or > SDT_ASM_MAX_ROWS; flags or reserved not 0; offsets not monotonic or
 * nwords too short (as for reads); a sequence of 2^32 bases or more (host form); d_out not 8-byte aligned (device form).
 * Device memory: from asm_begin to asm_end one byte per table slot and 64 KiB for totals and matrix, SDT_ENOMEM when it does not fit;
 * the host form of asm_add also the staged piece with its offsets and 32 B per sequence of it.
 * Out of scope: distinct counting of assembly-only k-mers (they show as kmers - found, by occurrence); a k other than the table's K;
 * sharded contexts (refused); a kept-read form; plots; any change to profile_reads or its limit.
 *
 * Two counted tables compared.  The table can be asked by k-mer, by read and by assembly; these two calls ask it against ANOTHER
 * table: how many solid k-mers of the raw library does the trimmed, normalised or deduplicated one still hold, how many did it
 * lose, how many did correction invent; are two samples the same tissue (Jaccard, Bray-Curtis over k-mers: what Mash and KAT comp
 * give); which k-mers are solid here and absent there.  Two contexts with counted tables of the same K on one device; nothing is
 * written to either.  Added without a change of SDT_ABI_VERSION: the two calls, the two structs and the constant are additions.
 *     Integers only.  Everything is exact and does not depend on the slot layout of either table (their sizes, how often they were
 *     grown), on the launch geometry, or on how the high halves of the counts are read.
 *     COUNTS.  For a canonical k-mer x, cA(x) is the count profile_reads sees in A: 32 bits with the high half, absent = 0, the
 *     deleted flag ignored; cB(x) the same in B.  x is IN A iff it has a node in A (whatever its count).
 *     MATRIX.  rows x cols uint64_t: m[r][c] = the distinct canonical k-mers of A u B with min(cA, rows - 1) = r and
 *     min(cB, cols - 1) = c.  Nothing is special-cased: a node whose count is 0 lands in row or column 0 like an absent k-mer.
 *     TOTALS, uint64_t[8]:  [0] nodes in A   [1] nodes in B   [2] nodes in both   [3] the sum of cA over A   [4] the sum of cB over B
 *         [5] the sum of min(cA, cB) over the shared nodes (the minimum is taken per node, before summing)
 *         [6] the sum of cA over the shared nodes   [7] the sum of cB over the shared nodes
 *     Jaccard, the two containments and Bray-Curtis are functions of the totals; the caller computes them.
 *     SELECTION.  The k-mers IN A with min_a <= cA <= max_a and min_b <= cB <= max_b (cB = 0 for a k-mer that is not in B): keys in
 *     the layout of sdt_gpu_export_nodes (sdt_gpu_key_words words per k-mer, most significant first) with both counts, in no
 *     particular order.  The k-mers only in B: the same call with the contexts swapped.
 *     SYMMETRIES.  compare(B, A) is the transpose of compare(A, B) with totals [0]/[1], [3]/[4], [6]/[7] swapped; compare(A, A) is
 *     diagonal with [0] = [1] = [2].  a == b is allowed.
 *   compare_tables: matrix (rows x cols) and totals, either may be NULL, not both.  Waits.
 *   compare_select: any of keys, count_a, count_b may be NULL.  *n = the number of matching k-mers, whatever capacity is; at most
 *                   capacity of them are written, and which ones when there are more is not specified.  capacity = 0 with NULL
 *                   arrays asks for the size.  Waits.
 * The work runs on A's stream, after B's stream has been drained; the time of a pass is booked on the context whose table it walks
 * (sdt_gpu_kernel_time: the first pass and the selection on A, the second pass on B).  Neither context's assembly tally is touched
 * or made stale; the high halves of each context come through its own cache, which is filled if it was not.
 * SDT_ESTATE: each context under the state rules of search_kmers, with its messages (a SDT_FLAG_CONTIG_INDEX context, a shard, after
 * load_paths / import_paths, a released table, batches pushed and not drained); the message begins with the call's name and says
 * which context failed: "sdt_gpu_compare_tables: context B: ...".
 * SDT_EINVAL, before any launch, with the field and its value: a NULL context, NULL params or range; different K (both named);
 * different devices; rows or cols < 2; rows x cols > SDT_CMP_MAX_CELLS; flags or reserved not 0; matrix and totals both NULL;
 * min_a > max_a or min_b > max_b; capacity > 0 with every array NULL; capacity > 2^31 (the list of one call: narrow the ranges).
 * Device memory held during the call, SDT_ENOMEM (nothing written) when it does not fit:
 *     compare_tables    totals and matrix: 64 B + 8 B x rows x cols, 128 KiB + 64 B at most
 *     compare_select    16 B; with capacity > 0 also the list in chunks of 256 records of 8 B x (key words + 1) --
 *                       capacity / 192 + 1 chunks and one per wavefront of the grid -- 8 B per chunk, and the dense copy of what
 *                       was written
 * Out of scope: more than two tables; tables of different K; sharded contexts (refused); sketches; statistics on the counts;
 * scaling by library size (the matrix is raw); a read filter by the selection; a device-pointer form of the selection.
 *
 * Reads clustered by connected component of the counted k-mer graph.  Every node of the table carries eight link counters, four
 * to the left and four to the right: the table is a de Bruijn graph, and its connected components split the read set into the
 * groups that can be assembled, normalised or inspected on their own (what Trinity's Chrysalis and khmer's partition-graph /
 * annotate-partitions give).  Needs the counted table, and writes nothing to it, to the kept reads or to any cache of the context.
 * Added without a change of SDT_ABI_VERSION: the seven calls, the three structs and the constant are additions.
 *     Integers only.  Everything is exact and does not depend on the table's size or layout, on the order in which pass 1 placed
 *     colliding keys, on the pass-1 kernel family, or on the launch geometry.
 *     PARAMETERS (sdt_cluster_params): flags must be 0; min_link 1 .. 63; max_count 0 (no upper bound) or >= max(min_count, 1).
 *     LIVE NODES.  A node is live iff it exists and its deleted flag is clear, its 32-bit count (the one profile_reads sees, with
 *     the high half) is >= max(min_count, 1), and max_count is 0 or the count is <= max_count.
 *     EDGES.  For a live node u, a side (0 left, 1 right) and a base b, the link counter is bits 24 * side + 6 * b of the node's
 *     link word (l_links | r_links << 24, as export_nodes gives them).  If it is >= min_link: the neighbour word is u's k-mer
 *     shifted right by one base with b in front (left), or shifted left with b behind (right); its canonical strand is looked up;
 *     if that node v exists and is live, {u, v} is an edge.  One qualifying end is enough; a neighbour that is missing or not live
 *     gives no edge; u = v is allowed and joins nothing.
 *     CLUSTERS are the connected components of the live nodes under these edges, numbered 0 .. C - 1 in ascending order of their
 *     smallest canonical k-mer (numeric on the key words, most significant first).  SDT_CLUSTER_NONE = no cluster.
 *     READS.  A read of len bases has n = len - K + 1 k-mers (0 for len < K); a k-mer is live iff its canonical node is.  RECORD,
 *     per read (sdt_read_cluster, 24 bytes):
 *         kmers  n            live   its live k-mers
 *         cluster  the id of its first live k-mer, or SDT_CLUSTER_NONE
 *         split    its live k-mers that lie in another cluster than that one
 *         unit     a unit is one read or, with paired, reads 2t and 2t + 1: mate 1's cluster unless that is NONE, else mate 2's
 *         verdict  the first that applies: 4 every read of the unit has n == 0 (short); 3 no read of the unit has a live k-mer
 *                  (unassigned); 2 this read has no live k-mer, its mate has (assigned through the mate); 1 split > 0 or
 *                  cluster != unit (assigned, not whole); 0 assigned and whole
 *     keep[i] = 1 iff pick_lo <= unit <= pick_hi and unit is not SDT_CLUSTER_NONE.
 *   cluster_begin:      builds the clustering and waits.  info[8]: [0] live nodes  [1] link ends: the triples (u, side, b) that
 *                       qualified and found a live neighbour  [2] clusters  [3] nodes of the largest cluster  [4] its id (the
 *                       smallest among equals; 0 without a cluster)  [5] nodes that exist and are not live  [6], [7] 0.  info may be
 *                       NULL.  A second begin replaces the first.  A table of 2^32 - 1 slots or more is SDT_EINVAL ("the labels
 *                       are 32-bit"): a 64-bit form does not exist yet.
 *   cluster_components: per cluster in id order its smallest k-mer (sdt_gpu_key_words words, most significant first) and
 *                       sdt_cluster_comp { count_sum: the sum of its nodes' counts; nodes }.  Either array may be NULL; *n = C
 *                       always; SDT_EFULL when C > capacity, with the first capacity written.
 *   cluster_lookup:     the cluster of n k-mers, keys as for search_kmers, either strand; absent or not live: SDT_CLUSTER_NONE.
 *   cluster_reads:      a host batch, staged in pieces (a piece never splits a pair); rec nreads records, keep nreads bytes or
 *                       NULL; *n_kept = reads with keep 1.  Waits.
 *   cluster_reads_device: buffers already on the device; d_keep may be NULL.  Asynchronous on the context's stream when n_kept is
 *                       NULL; with n_kept it waits for the count.
 *   cluster_kept_reads: the reads kept in HBM, records by read ordinal as for select_kept_reads: pair_ranges as there, a pair with
 *                       only one mate kept is judged on that mate alone, records of ordinals that no kept read has are untouched,
 *                       SDT_EFULL (nothing written) when a kept read's ordinal is >= out_capacity.  *nreads = the kept reads seen.
 *   cluster_end:        frees the labels (sdt_gpu_destroy does too).  Without a begin: SDT_OK.
 * There is NO limit on the length of a read: a wavefront walks a unit 64 k-mer positions at a time and keeps no strip of it.
 * nreads == 0 (n == 0 for lookup): SDT_OK, nothing touched, whatever the rest says.
 * SDT_ESTATE: cluster_begin under the state rules of search_kmers, with its messages (a SDT_FLAG_CONTIG_INDEX context, a shard or any
 * context with a communicator, after load_paths / import_paths, a released table, batches pushed and not drained); every other call
 * without a begin, after cluster_end, and once the table has changed since cluster_begin (counted into, grown, reset, delow,
 * imported, released, any call of the graph phases): "the table changed since sdt_gpu_cluster_begin" -- labels are by slot and never read against another table.
 * SDT_EINVAL, before any launch: NULL params; flags not 0; min_link outside 1 .. 63; max_count below max(min_count, 1) and not 0;
 * a table of 2^32 - 1 slots or more; an odd nreads with paired; offsets not monotonic or nwords too short (as for reads); a read of
 * 2^32 bases or more (host form); pair ranges as for select_kept_reads.
 * Device memory: from cluster_begin to cluster_end 4 B per table slot; during cluster_begin 4 B per slot more and, per cluster,
 * 8 B x (key words + 2) + 8 B and the sort's scratch; SDT_ENOMEM with nothing left allocated when that does not fit.  The forms
 * over reads hold what select_reads holds, with records of 24 B.
 * Out of scope: tables of 2^32 - 1 slots and more; sharded contexts; joining clusters through mate pairs; removing knots beyond
 * what max_count does.
 *
 * The bubbles of the counted k-mer graph: two non-branching paths that leave one k-mer and meet again.  A substitution (a SNP, a
 * recurring error) is a bubble with K nodes on each side, an indel one with unequal sides, a skipped exon a short side against a
 * long one (what KisSplice and DiscoSNP report from a de Bruijn graph) -- the structures that tip cutting and the removal of minor
 * branches flatten.  Needs the counted table, and writes nothing to it, to the kept reads or to any cache or tally of the context.
 * Added without a change of SDT_ABI_VERSION: the four calls, the two structs and the constant are additions.
 *     Integers only.  Everything is exact and does not depend on the table's size or layout, on the pass-1 kernel family, or on
 *     the launch geometry.
 *     PARAMETERS (sdt_bubble_params): flags and reserved must be 0; min_link 1 .. 63; max_count 0 (no upper bound) or
 *     >= max(min_count, 1); max_len 1 .. SDT_BUBBLE_MAX_LEN (2^20).
 *     LIVE NODES are those of cluster_begin: the node exists, its deleted flag is clear, its 32-bit count (with the high half) is
 *     >= max(min_count, 1), and max_count is 0 or the count is <= max_count.
 *     ORIENTED WORDS.  The rule speaks of k-mer words x: K bases, either strand.  The node of x is its canonical strand; x is live
 *     iff that node is; count(x) is the node's count.  The OUT SIDE of x comes from the node's own link word (l_links |
 *     r_links << 24): if x is the stored canonical key, the four right counters, base b at bits 24 + 6 b; otherwise the four left
 *     counters of the canonical key, base b read at bits 6 (b ^ 2).  A palindrome (even K) is its own canonical key, uses the
 *     right counters, and is one oriented word, not two.
 *     SUCCESSORS.  succ(x) is the list, in ascending b, of (b, y, link) with link = the out counter of x for b >= min_link,
 *     y = next(x, b) -- x shifted left by one base, b behind, masked to K bases -- and y live.  outdeg(x) = |succ(x)|,
 *     indeg(x) = |succ(revcomp(x))|.  Every degree comes from the examined node's own counters and the liveness of the neighbour
 *     they name; in a table that pass 1 counted both ends of a link carry the same counter.
 *     BRANCH.  For a source word s with outdeg(s) >= 2 and one (b, y, link) of succ(s): cur = y, len = 0, and repeat:
 *         1. if indeg(cur) >= 2 the branch REACHES THE SINK cur; stop
 *         2. else if outdeg(cur) != 1 or len == max_len the branch fails; stop
 *         3. else cur is an inner node: len += 1, min = min(min, count(cur)), sum += count(cur), cur = its only successor.
 *     A branch with len == 0 has min = 0 and sum = 0; a branch never has more than max_len inner nodes.  Nothing else is special:
 *     s may be the sink.
 *     BUBBLE.  Two branches of the same s, with bases base_a < base_b, that reach the same sink word t.  Three branches that
 *     meet are three bubbles.  The bubble is REPORTED iff s <= revcomp(t), numeric on the key words, most significant first: a
 *     bubble of a counted table is found from both of its ends, and this keeps one of them.
 *     ID.  The reported bubbles are numbered 0 .. N - 1 in ascending order of (s, base_a, base_b).
 *     RECORD (sdt_bubble, 48 bytes): sum_a, sum_b, len_a, len_b, min_a, min_b of the two branches; src_count = count(s),
 *     snk_count = count(t); info = base_a | base_b << 2 | link_a << 8 | link_b << 16; reserved 0.  With each record go two
 *     words, 2 x sdt_gpu_key_words uint64: s, then t, as oriented words, most significant word first.
 *     PATHS.  Branch a of a bubble is len_a + 1 base codes (A 0, C 1, T 2, G 3, one byte each): the bases appended from s up to
 *     and including the step that gives t; the first is base_a.  The allele sequence is s followed by them; its last K bases are t.
 *   bubbles_begin: finds, sorts and numbers the bubbles, keeps the list on the device, and waits.  info[8]: [0] live nodes
 *                  [1] fork sides: the oriented words with outdeg >= 2  [2] branches walked: the sum of outdeg over the fork sides
 *                  [3] branches that reached a sink  [4] bubbles N  [5] the sum of len_a + len_b + 2 over the bubbles = the bytes
 *                  of all paths  [6] the longest branch (len) of a reported bubble  [7] 0.  info may be NULL.  A second begin
 *                  replaces the first.
 *   bubbles_fetch: bubbles first .. first + n - 1 in id order: keys n x 2 x sdt_gpu_key_words words, rec n records; either may be
 *                  NULL.  first + n > N: SDT_EINVAL.
 *   bubbles_paths: offsets[2 n + 1] = the prefix sums of len + 1 in the order a0, b0, a1, b1, ...; the bytes of branch j at
 *                  bases[offsets[j]].  SDT_EFULL, with the offsets written and no base written, when offsets[2 n] > capacity.
 *                  bases == NULL with capacity == 0 asks for the offsets only.  The branches are walked again in the table: no
 *                  path is stored at begin.
 *   bubbles_end:   frees the list (sdt_gpu_destroy does too).  Without a begin: SDT_OK.
 * There is no limit on the length of a branch other than max_len.  n == 0: SDT_OK, nothing touched, whatever the rest says.
 * SDT_ESTATE: bubbles_begin under the state rules of search_kmers, with its messages (a shard or any context with a communicator
 * among them); every other call without a begin, after bubbles_end, and once the table has changed since bubbles_begin (counted
 * into, grown, reset, delow, imported, released, any call of the graph phases): "the table changed since sdt_gpu_bubbles_begin".
 * SDT_EINVAL, before any launch: NULL params; flags or reserved not 0; min_link outside 1 .. 63; max_count below
 * max(min_count, 1) and not 0; max_len outside 1 .. 2^20 -- each with the field and its value; a range past N.
 * Device memory: from bubbles_begin to bubbles_end 48 B + 16 B x key words per bubble.  During bubbles_begin the fork list, 8 B per
 * fork side in chunks of 256 (a first guess of one per 64 table slots, the exact need on a second scan when that was too small),
 * the bubbles as they are found, six per fork side at the most at 48 B + 16 B x key words, and per bubble 24 B of sort keys and
 * order with the sort's scratch.  Nothing is per table slot.  SDT_ENOMEM leaves nothing allocated.  bubbles_paths holds the
 * offsets and the bytes it returns.
 * Out of scope: nested or overlapping bubbles (inner nodes are 1-in 1-out); popping or editing anything; allele counts from a
 * second table; phasing by reads or mates; sharded contexts; 2^32 bubbles and more.
 *
 * The unitigs of the counted k-mer graph and their links: the compacted de Bruijn graph, before any cleaning -- the maximal
 * non-branching paths with their abundances and what joins them (what BCALM writes, what an assembler dumps as its graph, what
 * Bandage draws).  Needs the counted table, and writes nothing to it, to the kept reads or to any cache or tally of the context.
 * Added without a change of SDT_ABI_VERSION: the five calls and the three structs are additions.
 *     Integers only.  Everything is exact and does not depend on the table's size or layout, on the pass-1 kernel family, or on
 *     the launch geometry.
 *     PARAMETERS (sdt_unitig_params): flags must be 0; min_link 1 .. 63; max_count 0 (no upper bound) or >= max(min_count, 1).
 *     LIVE NODES, ORIENTED WORDS, SUCCESSORS (succ, outdeg, indeg, next, revcomp) are those of the bubble rule above, word for word.
 *     JOIN.  For live oriented words x and y, JOIN(x, y) holds iff succ(x) has exactly one element and it is y; succ(revcomp(y))
 *     has exactly one element and it is revcomp(x); the nodes of x and y differ (this excludes y = x and y = revcomp(x)); and
 *     neither x nor y is its own reverse complement.  JOIN(x, y) <=> JOIN(revcomp(y), revcomp(x)) by construction, also where the
 *     two ends of a link carry different counters, which imported tables can.  A word has at most one right and one left join,
 *     so the oriented words fall into paths and cycles; each has a mirror image that shares no word with it (a shared word would
 *     need a palindrome or a hairpin join, and both are excluded).
 *     UNITIG.  A maximal chain x0 .. x(n-1) with JOIN(xi, xi+1).  A linear one is REPORTED in the orientation with
 *     x0 <= revcomp(x(n-1)), numeric on the key words, most significant first; a palindromic single word is reported once.  A
 *     cycle (every word has both joins) is reported as circular: of the two mirror cycles the one that holds the smallest word of
 *     both; that word is a stored canonical key, and it is x0.  Every live node lies in exactly one reported unitig.
 *     ID.  Ids run 0 .. N - 1 in ascending order of x0 (every word is in one unitig: no ties).
 *     RECORD (sdt_unitig, 24 bytes): sum, min, max over the counts of the n nodes; nodes = n; info = circular | indeg(x0) << 4 |
 *     outdeg(x(n-1)) << 8.  With each record go two words, 2 x sdt_gpu_key_words uint64: x0, then x(n-1), most significant word
 *     first.
 *     SEQUENCE.  The K bases of x0, then the last base of x1 .. x(n-1): nodes + K - 1 base codes (A 0, C 1, T 2, G 3, one byte
 *     each).  A circular unitig is written the same way from x0; its last K - 1 bases are NOT its first K - 1: the closing link
 *     says that it closes.
 *     LINKS.  For a reported unitig u and an orientation o, the out word w is x(n-1) for o = 0 (+) and revcomp(x0) for o = 1 (-).
 *     For every (b, y, link) of succ(w), in ascending b: if y is the first word of an oriented unitig (v, o') -- y = x0 of v for
 *     o' = 0, y = revcomp(x(n-1)) of v for o' = 1 -- one record (sdt_unitig_link, 16 bytes): from = u, to = v, info = o | o' << 1
 *     | b << 2 | link << 8, reserved 0.  The order is ascending (from, o, b).  A circular unitig gets its closing link
 *     (u, +) -> (u, +) and the mirror from the same rule.  In a table that pass 1 counted every successor of an out word is such
 *     a first word and every link appears from both sides; where the two ends of a link disagree, a target that is no first word
 *     is left out and counted (*n_dangling).
 *   unitigs_begin: finds, sorts and numbers the unitigs, keeps the list on the device, and waits.  info[8]: [0] live nodes
 *                  [1] start words found (= 2 x the linear unitigs: a chain is walked from both ends)  [2] unitigs N  [3] circular
 *                  ones  [4] the sum of nodes over the list: it equals [0], or the call fails with SDT_ESTATE and says so  [5] the
 *                  bytes of all sequences  [6] the longest unitig, in nodes  [7] 0.  info may be NULL.  A second begin replaces the
 *                  first.
 *   unitigs_fetch: unitigs first .. first + n - 1 in id order: keys n x 2 x sdt_gpu_key_words words, rec n records; either may be
 *                  NULL.  first + n > N: SDT_EINVAL.
 *   unitigs_seqs:  offsets[n + 1] = the prefix sums of nodes + K - 1; the bytes of unitig first + i at bases[offsets[i]].
 *                  SDT_EFULL, with the offsets written and no base written, when offsets[n] > capacity.  bases == NULL with
 *                  capacity == 0 asks for the offsets only.  The chains are walked again in the table: no sequence is stored at
 *                  begin; a chain that walks otherwise than at begin is counted and the call fails with SDT_ESTATE.
 *   unitigs_links: the links of the unitigs of the range, *n_links of them; *n_dangling (may be NULL) as above.  SDT_EFULL, with
 *                  *n_links set and nothing written, when *n_links > capacity.  links == NULL with capacity == 0 asks for the size.
 *   unitigs_end:   frees the list (sdt_gpu_destroy does too).  Without a begin: SDT_OK.
 * n == 0: SDT_OK, nothing touched, whatever the rest says.
 * SDT_ESTATE: unitigs_begin under the state rules of search_kmers, with its messages (a shard or any context with a communicator
 * among them); every other call without a begin, after unitigs_end, and once the table has changed since unitigs_begin (counted
 * into, grown, reset, delow, imported, released, any call of the graph phases): "the table changed since sdt_gpu_unitigs_begin".
 * A clustering, a bubble list and an assembly tally stay valid across these calls, and the list across theirs.
 * SDT_EINVAL, before any launch: NULL params; flags not 0; min_link outside 1 .. 63; max_count below max(min_count, 1) and not 0
 * -- each with the field and its value; a range past N.  SDT_ELIMIT: 2^32 unitigs or more (the sort's indices and the ids of a
 * link are 32-bit); a unitig of 2^32 nodes or more.
 * Device memory: from unitigs_begin to unitigs_end 24 B + 16 B x key words per unitig, and the index that unitigs_links searches,
 * 4 B + 8 B x key words per unitig (the reverse complements of the last words, sorted, with their ids; the first words are the
 * list itself).  During unitigs_begin the list of start words, 8 B each in chunks of 256 (a first guess of one per 16 table slots,
 * the exact need on a second scan when that was too small), the unitigs as they are found, one per start word at the most at
 * 24 B + 16 B x key words, and per unitig 24 B + 8 B x key words of sort keys and order with the sort's scratch.  Only if the
 * chains do not cover the live nodes -- the graph has a cycle without a branch -- also ONE BIT PER TABLE SLOT and a second copy of
 * the found unitigs; every node on such a cycle then walks it until it meets a smaller key, which is quadratic in the length of
 * one cycle in the worst case (real ones are a PhiX or a mitochondrion).  SDT_ENOMEM leaves nothing allocated.  unitigs_seqs
 * and unitigs_links hold the offsets and the bytes they return.
 * One lane walks one unitig, so a wavefront waits for its longest: accepted for transcripts, whose unitigs are thousands of nodes
 * long.  Out of scope: a list-ranking formulation for genome-length unitigs (single ones of millions of nodes); mate threading
 * (the k-mer -> unitig look-up and read threading are the block below); removing tips or popping bubbles; sharded contexts; tables
 * of even K; 2^32 unitigs and more.
 *
 * Reads threaded through the unitig list: a k-mer -> unitig index over the list of unitigs_begin, and every read laid on the list as
 * a path of segments -- what quantifies unitigs by reads, phases a bubble by the reads that cross both of its ends, shows which
 * links one read traverses in a row, and what a GAF line says on the GFA of the list.  Needs the counted table and a list begun with
 * sdt_gpu_unitigs_begin, and writes nothing to the table, to the kept reads or to any cache or tally of the context.  Added without
 * a change of SDT_ABI_VERSION: the four calls, the three structs and the constant are additions.
 *     Integers only.  Everything is exact and does not depend on the table's size or layout, on the pass-1 kernel family, on the
 *     launch geometry, or on how a host batch is cut into pieces.
 *     LIVE NODES, ORIENTED WORDS, SUCCESSORS, JOIN, UNITIG and ID are those of the unitig rule above, word for word.
 *     LABEL.  Every live node with stored canonical key c lies in one reported unitig u at one position i, counted from 0 in the
 *     reported orientation x0 .. x(n-1): s = 0 if x_i = c, s = 1 if x_i = revcomp(c).
 *     PLACEMENT.  A k-mer word w, as given, whose node is live has place(w) = (u, i, o): o = 0 when w = x_i -- the read runs along
 *     the reported orientation -- and o = 1 when w = revcomp(x_i).
 *     READS.  A read of len bases has n = max(len - K + 1, 0) k-mers w_0 .. w_(n-1), forward as read.  Position p CONTINUES p - 1
 *     iff both k-mers are live, they lie in the same unitig with the same o, and i_p = i_(p-1) + 1 for o = 0 or i_p = i_(p-1) - 1
 *     for o = 1.  There is no modular arithmetic: going round a circular unitig is NOT a continuation, it is the closing link.  A
 *     SEGMENT is a maximal run of live positions in which each position continues the one before.  The join of a segment that
 *     starts at p: 0 if p = 0 or w_(p-1) is not live (the first segment, or one after a gap); 1 if the out counter of w_(p-1)
 *     towards the last base of w_p is >= min_link -- the out side of the bubble rule, read from w_(p-1)'s own node: the transition
 *     is LINKED; 2 otherwise: the k-mers are adjacent in the read, and that is no edge of this graph.
 *     SEGMENT RECORD (sdt_path_seg, 24 bytes): unitig; info = o | join << 1; read_pos = p; unitig_pos = i of its FIRST k-mer;
 *     kmers; reserved 0.  For o = 1 the segment covers positions unitig_pos down to unitig_pos - kmers + 1.
 *     READ RECORD (sdt_read_path, 24 bytes): kmers = n; live = the live k-mers of the read; segs = its segments; breaks = the
 *     segments after the first whose join != 1; first, last = the unitig of the first and of the last segment, or SDT_UNITIG_NONE.
 *     What follows: the kmers of a read's segments sum to live.  In a table that pass 1 counted, a segment with join 1 starts at
 *     the in end of its oriented unitig (v, o') -- unitig_pos 0 for o' = 0, nodes - 1 for o' = 1 -- the segment before it ends at
 *     the out end of (u, o), and (u, o, v, o', the last base of w_p) is a record of sdt_gpu_unitigs_links.
 *   unitigs_index:  labels the table slot of every live node, 8 bytes per slot (the unitig; pos << 1 | s; all ones elsewhere), and
 *                   waits.  info[4]: [0] nodes labelled  [1] unitigs  [2] bytes held  [3] 0; info may be NULL.  The labelled nodes
 *                   are the live nodes of begin, or the call fails with SDT_ESTATE as unitigs_seqs does.  A second index rebuilds.
 *                   The index goes with the list: unitigs_end, a second unitigs_begin and sdt_gpu_destroy free it, and what makes
 *                   the list stale makes it stale.  No limit of 2^32 slots.
 *   unitigs_lookup: the place of n k-mers, keys as for search_kmers, either strand: sdt_unitig_pos { unitig, pos, info = o of the
 *                   word AS GIVEN, reserved 0 }; absent or not live: unitig SDT_UNITIG_NONE, the rest 0.
 *   unitigs_reads:  a host batch, staged in pieces like cluster_reads: rec nreads records; seg_offsets[nreads + 1] the prefix sums
 *                   of rec[].segs; the segments of read r at segs[seg_offsets[r]] in ascending read_pos; *n_segs the total.
 *                   segs == NULL with capacity == 0 asks for the records and the offsets only.  SDT_EFULL when the total exceeds
 *                   capacity: rec, seg_offsets and *n_segs are complete, what segs holds is unspecified.  Waits.
 *   unitigs_reads_device: the same with every buffer on the device (d_segs may be NULL with capacity 0); waits for the total.
 * There is NO limit on the length of a read: a wavefront walks a read 64 k-mer positions at a time and keeps no strip of it (a
 * segment that is open at the end of a step is carried in registers).  nreads == 0 (n == 0 for lookup): SDT_OK, nothing touched.
 * SDT_ESTATE: under the state rules of search_kmers with their messages; without a list, after unitigs_end and once the table has
 * changed, with the messages of the unitig calls; lookup and the reads forms without an index: "no sdt_gpu_unitigs_index of this
 * unitig list".  SDT_EINVAL, before any launch: NULL arguments; offsets not monotonic or nwords too short (as for reads); a read
 * of 2^32 bases or more (host form).  SDT_ELIMIT: a unitig of 2^31 nodes or more (a position and its strand share 32 bits).
 * Device memory: from unitigs_index to unitigs_end 8 B per table slot; SDT_ENOMEM leaves nothing of it allocated and the list as
 * it was.  The forms over reads hold 8 B per read of segment counts and the scan's scratch, and the host form what cluster_reads
 * holds with records of 24 B, 8 B per read of offsets and the segments of one piece.  Every read is walked twice, first for its
 * record and the number of its segments, then, after an exclusive scan on the device, for the segments at their offsets.  A
 * clustering, a bubble list and an assembly tally stay valid across these calls.
 * Out of scope: a form over the reads kept in HBM (there is no kept form and there are no keep bytes); aligning through the
 * stretches that are not live; sharded contexts; even K.  (What the reads support of the list is the block below.)
 *
 * Read support tallied on the unitig list: how many segments and k-mers of the added reads lie in every unitig, how many reads
 * traverse every link, which way into a unitig goes with which way out (junctions), and mate links between unitigs: which unitigs a
 * read pair bridges -- what picks paths through the graph, separates isoforms at a shared exon and joins unitigs that no single read
 * joins, without taking the segments of sdt_gpu_unitigs_reads to the host.  Needs the counted table, a list begun with
 * sdt_gpu_unitigs_begin and its sdt_gpu_unitigs_index, and writes nothing to the table, to the kept reads, to the index or to any
 * other cache or tally of the context.  Added without a change of SDT_ABI_VERSION: the nine calls and the five structs are additions.
 *     Integers only.  Everything is exact and does not depend on the order of the reads, on their split over add calls, on how a
 *     host batch is cut into pieces (pairs stay together), on the launch geometry, or on the table's size or layout.
 *     LIVE NODES, ORIENTED WORDS, SUCCESSORS, JOIN, UNITIG, ID, LABEL, PLACEMENT, READS, CONTINUES, SEGMENT and join are those of
 *     the threading rule above, word for word.
 *     ORIENTED UNITIG.  The 32-bit number ou = unitig << 1 | o; its mirror is ou ^ 1.
 *     PER UNITIG (sdt_unitig_support, 16 bytes): segs = the segments of all added reads in the unitig; kmers = the sum of their
 *     kmers.  (The number of DISTINCT READS per unitig stays on the host, in `sdt-kmers thread`: an exact set of reads per unitig
 *     has no bounded form on the device.)
 *     PER LINK (sdt_link_support, 16 bytes), parallel to the records of sdt_gpu_unitigs_links for the same range, record by record.
 *     A segment with join 1 that starts at position p is one TRAVERSAL of (the ou of the segment before it, b = the last base of
 *     w_p).  along of a record (from, o, b) = the traversals of (from << 1 | o, b).  against = the along of the record's MIRROR, the
 *     one record that leaves (to, o' ^ 1) for (from, o ^ 1) -- it may be the record itself; its base is the complement of the first
 *     base of the record's out word.  The closing link of a circular unitig is a link like any other.  A traversal that matches no
 *     record of the list is counted in the totals only (imported tables whose link ends disagree).
 *     JUNCTIONS (sdt_unitig_junction, 24 bytes: from, via, to oriented unitigs; reserved 0; count).  Two consecutive segments of one
 *     read that both have join 1 pass through the unitig of the first of them: with f the ou of the segment before it, v its own and
 *     t that of the second, one PASSAGE (f, v, t).  A passage and its mirror (t ^ 1, v ^ 1, f ^ 1) are the same junction, reported
 *     in the form whose via has o = 0.  The list is ascending by (via, from, to) and holds the junctions with count > 0.  (The set
 *     is keyed by the unitig of via and the two bases with which via is left at either end; in a table whose link ends disagree,
 *     passages that share those share a junction, reported with the ends of the first of them that came.)
 *     MATE LINKS (sdt_mate_link, 16 bytes: from, to oriented unitigs; pairs).  paired: reads 2r and 2r + 1 are mates, as for
 *     cluster_reads; forward/reverse libraries only.  If both mates have a segment, with (a, oa) the LAST segment of mate 1 and
 *     (b, ob) the LAST segment of mate 2 -- mate 2 is read against the fragment, so its last segment is the one nearest mate 1 --
 *     the link is from = a << 1 | oa, to = b << 1 | (ob ^ 1).  from == to: the pair lies within one unitig, counted in the totals
 *     only.  Otherwise (from, to) and (to ^ 1, from ^ 1) are one link, reported in the form with the smaller (from, to); the list
 *     is ascending by (from, to).
 *     TOTALS, uint64_t[12]: [0] reads  [1] reads with a segment  [2] segments  [3] live k-mers  [4] traversals  [5] traversals
 *     without a record  [6] passages  [7] pairs  [8] pairs with both mates placed  [9] pairs within one unitig  [10] pairs tallied
 *     as mate links  [11] entries dropped for want of room.
 *   unitigs_support_begin:     a cleared tally for the list, kept on the device; a second begin replaces the first.  params:
 *                              junction_capacity and mate_capacity = the DISTINCT junctions / mate links the two sets may hold, 0 =
 *                              that list is not kept (its passages and pairs are still counted in the totals) and its fetch gives
 *                              SDT_EINVAL; flags and reserved 0.
 *   unitigs_support_add:       a host batch, staged in pieces like cluster_reads (a piece of a paired batch holds whole pairs);
 *                              ADDS to the tally and waits.
 *   unitigs_support_add_device: the same for a batch on the device.
 *   unitigs_support_unitigs:   the tallies of unitigs first .. first + n - 1.
 *   unitigs_support_links:     the tallies of the link records of that range, *n_links of them, in the order of unitigs_links;
 *                              SDT_EFULL with *n_links set when capacity is too small; out == NULL with capacity == 0: the size.
 *   unitigs_support_junctions, unitigs_support_mates: the list, *n entries; SDT_EFULL with *n set when capacity is too small; out ==
 *                              NULL with capacity == 0: the size only.  The lists are put in order on the host.
 *   unitigs_support_totals:    the twelve totals.  [5] is made here from the link records of the whole list.
 *   unitigs_support_end:       frees the tally; without a begin SDT_OK.  The tally is part of the list's state: unitigs_end, a second
 *                              unitigs_begin and sdt_gpu_destroy free it; what makes the list or the index stale makes it stale; a
 *                              second unitigs_index leaves it valid, because the labels are a function of the list.
 * WHEN A SET FILLS UP -- more distinct entries than its capacity -- the add call returns SDT_EFULL, and so does every add after it
 * and every fetch of that set; totals[11] counts the entries that found no room (their number, unlike all else, depends on the
 * order of arrival).  The tallies per unitig and per link, the other set and the other totals stay exact.  The slots of a set are
 * the next power of two of twice its capacity, 64 at the least.
 * There is no limit on the length of a read.  nreads == 0 (n == 0): SDT_OK, nothing touched.
 * SDT_ESTATE: under the state rules of search_kmers with their messages; without a list, once the table has changed and without an
 * index with the messages of the threading calls; every call but begin and end without a begin:
 * "no sdt_gpu_unitigs_support_begin of this unitig list".  SDT_EINVAL, before any launch and with nothing added: NULL arguments;
 * non-zero flags or reserved; a capacity above 2^36; paired with an odd nreads; offsets not monotonic or nwords too short; a read of
 * 2^32 bases or more (host form); a range past N.  SDT_ELIMIT at begin: 2^31 - 1 unitigs or more (an oriented unitig is 32 bits,
 * and all ones is no unitig).
 * Device memory, from support_begin to support_end / unitigs_end: 16 B per unitig of tallies, 8 x 8 B per unitig of link slots
 * (two orientations x four bases), 24 B per slot of the junction set and 16 B per slot of the mate-link set, and 384 B of
 * counters; SDT_ENOMEM leaves nothing of it allocated.  unitigs_support_links holds the records and the tallies of its range,
 * 32 B per link; the host form of add holds what cluster_reads stages.  ON THE HOST a fetch of a list holds a copy of that set's
 * whole slot array (24 B or 16 B per slot, whatever it holds), and unitigs_support_totals the link records of the whole list and the
 * link slots, 8 x 8 B per unitig: ask for them once, after the last add.  One wavefront walks one read or one pair, once; every
 * count is a 64-bit atomic add at the memory side, the totals are summed per wavefront first.  A clustering, a bubble list and an
 * assembly tally stay valid across these calls.
 * Out of scope: the distinct reads per unitig on the device; gap or insert-size estimates on mate links; reverse/forward or
 * same-strand libraries; a form over the reads kept in HBM; sharded contexts; even K. */
typedef struct { uint32_t kmers, found, solid, min, median, max; } sdt_read_cov;
typedef struct { uint32_t kmers, weak, runs, fixed; } sdt_read_fix;
typedef struct { uint32_t kmers, median, cov, verdict; } sdt_read_pick;
typedef struct { uint32_t target, max_cv_pct; uint64_t seed; } sdt_norm_params;
typedef struct { uint32_t kmers, weak, median, start, len, verdict; } sdt_read_trim;
typedef struct { uint32_t min_count, min_cov, min_len, flags; } sdt_trim_params;
#define SDT_TRIM_CORRECTED 1u   /* sdt_trim_params.flags: runs that sdt_gpu_correct_reads would fix count as solid */
typedef struct { uint64_t first; uint32_t copies, verdict; } sdt_read_dup;   /* 16 bytes */
typedef struct { uint32_t flags, reserved; } sdt_dedup_params;
#define SDT_DEDUP_MATE_SWAP 1u  /* sdt_dedup_params.flags: pairs (a, b) and (b, a) are copies of each other */
#define SDT_CLIP_MAX_ADAPTERS    256
#define SDT_CLIP_MAX_ADAPTER_LEN 128
typedef struct { uint32_t adapters, tail3, tail5, start, len, verdict; } sdt_read_clip;   /* 24 bytes */
typedef struct { uint32_t min_overlap, max_err_pct, min_len, min_tail,
                          tail_err_pct, tail3_bases, tail5_bases, flags; } sdt_clip_params;
typedef struct { const uint32_t *words; const uint64_t *offsets; const uint8_t *ends;
                 uint32_t n, reserved; } sdt_adapter_set;
typedef struct { uint32_t overlap, mismatches, insert, start, len, verdict; } sdt_read_overlap;   /* 24 bytes */
typedef struct { uint32_t min_overlap, max_err_pct, min_len, flags; } sdt_overlap_params;
typedef struct { uint32_t windows, low, score, start, len, verdict; } sdt_read_complexity;   /* 24 bytes */
typedef struct { uint32_t max_score_pct, max_low_pct, min_len, flags; } sdt_complexity_params;
#define SDT_COMPLEXITY_TRIM 1u  /* sdt_complexity_params.flags: keep the longest clean stretch instead of judging the whole read */
typedef struct { uint32_t span, low, ee_ppm, start, len, verdict; } sdt_read_quality;   /* 24 bytes */
typedef struct { uint32_t phred_offset, cut_q, low_q, max_low_pct, max_ee_ppm, min_len, flags, reserved; } sdt_quality_params;
typedef struct { uint32_t kmers, hits, ref, start, len, verdict; } sdt_read_screen;   /* 24 bytes */
typedef struct { uint32_t min_hits, min_hit_pct, flags, reserved; } sdt_screen_params;
#define SDT_SCREEN_KEEP_MATCHED 1u  /* sdt_screen_params.flags: bait mode, the unmatched units are dropped */
#define SDT_SCREEN_NO_REF 0xFFFFFFFFu /* sdt_read_screen.ref / screen_lookup: no reference */
typedef struct { uint32_t merged, mismatches, from_b, start, len, verdict; } sdt_read_merge;   /* 24 bytes */
typedef struct { uint32_t min_len, max_len, phred_offset, flags; } sdt_merge_params;
#define SDT_MERGE_MERGED 5u     /* sdt_read_merge.verdict: the pair was merged, nothing of this read is left in the unmerged stream */
#define SDT_QC_MAX_CYCLES 4096
#define SDT_QC_FROM_END   1u    /* sdt_qc_params.flags: rows count from the last counted base of a read */
typedef struct { uint32_t cycles, phred_offset, flags, class_sel, reserved; } sdt_qc_params;
#define SDT_ASM_CN_COLS  8      /* columns of the spectrum: assembly copy number 0 .. 6, and 7 and more */
#define SDT_ASM_MAX_ROWS 1024
typedef struct { uint64_t sum; uint32_t kmers, found, solid, gaps, longest_gap, longest_at; } sdt_seq_support;   /* 32 bytes */
typedef struct { uint32_t min_count, rows, flags, reserved; } sdt_asm_params;   /* flags, reserved: 0 */
#define SDT_CMP_MAX_CELLS 16384 /* rows * cols: the matrix of a workgroup is 32-bit counters in 64 KiB of LDS */
typedef struct { uint32_t rows, cols, flags, reserved; } sdt_cmp_params;   /* rows, cols >= 2; flags, reserved: 0 */
typedef struct { uint32_t min_a, max_a, min_b, max_b; } sdt_cmp_range;
#define SDT_CLUSTER_NONE 0xFFFFFFFFu /* sdt_read_cluster.cluster / unit, cluster_lookup: no cluster */
typedef struct { uint32_t min_count, max_count, min_link, flags; } sdt_cluster_params;   /* flags: 0 */
typedef struct { uint64_t count_sum; uint32_t nodes, reserved; } sdt_cluster_comp;   /* 16 bytes */
typedef struct { uint32_t kmers, live, split, cluster, unit, verdict; } sdt_read_cluster;   /* 24 bytes */
#define SDT_BUBBLE_MAX_LEN (1u << 20) /* sdt_bubble_params.max_len: inner nodes of a branch at the most */
typedef struct { uint32_t min_count, max_count, min_link, max_len, flags, reserved; } sdt_bubble_params;   /* flags, reserved: 0 */
typedef struct { uint64_t sum_a, sum_b; uint32_t len_a, len_b, min_a, min_b, src_count, snk_count, info, reserved; } sdt_bubble;   /* 48 bytes */
typedef struct { uint32_t min_count, max_count, min_link, flags; } sdt_unitig_params;   /* flags: 0 */
typedef struct { uint64_t sum; uint32_t nodes, min, max, info; } sdt_unitig;   /* 24 bytes */
typedef struct { uint32_t from, to, info, reserved; } sdt_unitig_link;   /* 16 bytes */
#define SDT_UNITIG_NONE 0xFFFFFFFFu  /* sdt_unitig_pos.unitig, sdt_read_path.first / last: no unitig */
typedef struct { uint32_t unitig, pos, info, reserved; } sdt_unitig_pos;   /* 16 bytes */
typedef struct { uint32_t kmers, live, segs, breaks, first, last; } sdt_read_path;   /* 24 bytes */
typedef struct { uint32_t unitig, info, read_pos, unitig_pos, kmers, reserved; } sdt_path_seg;   /* 24 bytes */
typedef struct { uint64_t junction_capacity, mate_capacity; uint32_t flags, reserved; } sdt_support_params;   /* flags, reserved: 0 */
typedef struct { uint64_t segs, kmers; } sdt_unitig_support;   /* 16 bytes */
typedef struct { uint64_t along, against; } sdt_link_support;   /* 16 bytes */
typedef struct { uint32_t from, via, to, reserved; uint64_t count; } sdt_unitig_junction;   /* 24 bytes */
typedef struct { uint32_t from, to; uint64_t pairs; } sdt_mate_link;   /* 16 bytes */
int sdt_gpu_search_kmers(sdt_ctx *ctx, const uint64_t *keys, uint64_t n,
                         uint32_t *count, uint32_t *l_links, uint32_t *r_flags, uint8_t *status);
int sdt_gpu_search_kmers_device(sdt_ctx *ctx, const void *d_keys, uint64_t n,
                                void *d_count, void *d_l_links, void *d_r_flags, void *d_status);
int sdt_gpu_profile_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, uint32_t min_count, sdt_read_cov *out);
int sdt_gpu_profile_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                 uint64_t max_read_len, uint32_t min_count, void *d_out);
int sdt_gpu_profile_kept_reads(sdt_ctx *ctx, uint32_t min_count, sdt_read_cov *out, uint64_t out_capacity,
                               uint64_t *nreads);
int sdt_gpu_correct_reads_device(sdt_ctx *ctx, const void *d_packed_words, uint64_t nwords, const void *d_offsets,
                                 uint64_t nreads, uint64_t max_read_len, uint32_t min_count, void *d_fix,
                                 void *d_out_words, void *d_edits, uint64_t max_edits, uint64_t *n_edits);
int sdt_gpu_correct_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, uint32_t min_count, sdt_read_fix *fix, uint32_t *out_words,
                          uint64_t *edits, uint64_t max_edits, uint64_t *n_edits);
int sdt_gpu_correct_kept_reads(sdt_ctx *ctx, uint32_t min_count, sdt_read_fix *fix, uint64_t out_capacity,
                               uint64_t *nreads, uint64_t *edits, uint64_t max_edits, uint64_t *n_edits);
int sdt_gpu_kept_batches(const sdt_ctx *ctx, uint64_t *n);
int sdt_gpu_fetch_kept_batch(sdt_ctx *ctx, uint64_t i, uint64_t info[4], uint32_t *words, uint64_t words_cap,
                             uint64_t *offsets, uint64_t offsets_cap);
int sdt_gpu_select_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                         uint64_t nreads, int paired, const sdt_norm_params *params, sdt_read_pick *pick, uint8_t *keep,
                         uint64_t *n_kept);
int sdt_gpu_select_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                uint64_t max_read_len, int paired, const sdt_norm_params *params, void *d_pick, void *d_keep,
                                uint64_t *n_kept);
int sdt_gpu_select_kept_reads(sdt_ctx *ctx, const sdt_norm_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                              sdt_read_pick *pick, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_compact_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, const uint8_t *keep, uint32_t *out_words, uint64_t out_words_cap,
                          uint64_t *out_offsets, uint64_t *n_out_reads, uint64_t *n_out_words);
int sdt_gpu_compact_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                 const void *d_keep, void *d_out_words, uint64_t out_words_cap, void *d_out_offsets,
                                 uint64_t *n_out_reads, uint64_t *n_out_words);
int sdt_gpu_trim_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                       uint64_t nreads, const sdt_trim_params *params, sdt_read_trim *trim, uint8_t *keep,
                       uint64_t *n_kept);
int sdt_gpu_trim_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                              uint64_t max_read_len, const sdt_trim_params *params, void *d_trim, void *d_keep,
                              uint64_t *n_kept);
int sdt_gpu_trim_kept_reads(sdt_ctx *ctx, const sdt_trim_params *params, sdt_read_trim *trim, uint64_t out_capacity,
                            uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_compact_trimmed(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                            uint64_t nreads, const sdt_read_trim *trim, uint32_t *out_words, uint64_t out_words_cap,
                            uint64_t *out_offsets, uint64_t *n_out_reads, uint64_t *n_out_words);
int sdt_gpu_compact_trimmed_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                   const void *d_trim, void *d_out_words, uint64_t out_words_cap, void *d_out_offsets,
                                   uint64_t *n_out_reads, uint64_t *n_out_words);
int sdt_gpu_dedup_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                        uint64_t nreads, int paired, const sdt_dedup_params *params, sdt_read_dup *dup, uint8_t *keep,
                        uint64_t *n_kept);
int sdt_gpu_dedup_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                               int paired, const sdt_dedup_params *params, void *d_dup, void *d_keep, uint64_t *n_kept);
int sdt_gpu_dedup_kept_reads(sdt_ctx *ctx, const sdt_dedup_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                             sdt_read_dup *dup, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_clip_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                       uint64_t nreads, const sdt_clip_params *params, const sdt_adapter_set *adapters,
                       sdt_read_clip *clip, uint8_t *keep, uint64_t *n_kept);
int sdt_gpu_clip_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                              const sdt_clip_params *params, const sdt_adapter_set *adapters, void *d_clip, void *d_keep,
                              uint64_t *n_kept);
int sdt_gpu_clip_kept_reads(sdt_ctx *ctx, const sdt_clip_params *params, const sdt_adapter_set *adapters,
                            sdt_read_clip *clip, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_overlap_pairs(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, const sdt_overlap_params *params, sdt_read_overlap *ov, uint8_t *keep,
                          uint64_t *n_kept);
int sdt_gpu_overlap_pairs_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                 const sdt_overlap_params *params, void *d_ov, void *d_keep, uint64_t *n_kept);
int sdt_gpu_overlap_kept_pairs(sdt_ctx *ctx, const sdt_overlap_params *params, const uint64_t *pair_ranges,
                               uint64_t n_ranges, sdt_read_overlap *ov, uint64_t out_capacity, uint64_t *nreads,
                               uint64_t *n_kept);
int sdt_gpu_complexity_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                             uint64_t nreads, const sdt_complexity_params *params, sdt_read_complexity *cx, uint8_t *keep,
                             uint64_t *n_kept);
int sdt_gpu_complexity_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                    const sdt_complexity_params *params, void *d_cx, void *d_keep, uint64_t *n_kept);
int sdt_gpu_complexity_kept_reads(sdt_ctx *ctx, const sdt_complexity_params *params, sdt_read_complexity *cx,
                                  uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_quality_reads(sdt_ctx *ctx, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets, uint64_t nreads,
                          const sdt_quality_params *params, sdt_read_quality *out, uint8_t *keep, uint64_t *n_kept);
int sdt_gpu_quality_reads_device(sdt_ctx *ctx, const void *d_quals, const void *d_offsets, uint64_t nreads,
                                 const sdt_quality_params *params, void *d_out, void *d_keep, uint64_t *n_kept);
int sdt_gpu_screen_load(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nseqs,
                        const uint32_t *ref_of_seq, uint32_t n_refs, uint32_t k, uint64_t *n_kmers);
int sdt_gpu_screen_unload(sdt_ctx *ctx);
int sdt_gpu_screen_info(const sdt_ctx *ctx, uint64_t info[4]);
int sdt_gpu_screen_lookup(sdt_ctx *ctx, const uint64_t *keys, uint64_t n, uint32_t *refs);
int sdt_gpu_screen_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                         uint64_t nreads, int paired, const sdt_screen_params *params, sdt_read_screen *out, uint8_t *keep,
                         uint64_t *n_kept);
int sdt_gpu_screen_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired,
                                const sdt_screen_params *params, void *d_out, void *d_keep, uint64_t *n_kept);
int sdt_gpu_screen_kept_reads(sdt_ctx *ctx, const sdt_screen_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                              sdt_read_screen *out, uint64_t out_capacity, uint64_t *nreads, uint64_t *n_kept);
int sdt_gpu_merge_pairs(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads,
                        const sdt_read_overlap *ov, const uint8_t *quals, const sdt_merge_params *params, sdt_read_merge *mg,
                        uint32_t *out_words, uint64_t out_words_cap, uint64_t *out_offsets, uint64_t *n_merged,
                        uint64_t *n_out_words);
int sdt_gpu_merge_pairs_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                               const void *d_ov, const void *d_quals, const sdt_merge_params *params, void *d_mg,
                               void *d_out_words, uint64_t out_words_cap, void *d_out_offsets, uint64_t *n_merged,
                               uint64_t *n_out_words);
int sdt_gpu_merge_kept_pairs(sdt_ctx *ctx, const sdt_merge_params *params, const uint64_t *pair_ranges, uint64_t n_ranges,
                             const sdt_read_overlap *ov, sdt_read_merge *mg, uint64_t out_capacity, uint32_t *out_words,
                             uint64_t out_words_cap, uint64_t *out_offsets, uint64_t out_reads_cap, uint64_t *nreads,
                             uint64_t *n_merged, uint64_t *n_out_words);
int sdt_gpu_compact_quals_trimmed(sdt_ctx *ctx, const uint8_t *quals, uint64_t nbytes, const uint64_t *offsets,
                                  uint64_t nreads, const sdt_read_trim *recs, uint8_t *out_quals, uint64_t out_cap,
                                  uint64_t *n_out_bytes);
int sdt_gpu_compact_quals_trimmed_device(sdt_ctx *ctx, const void *d_quals, const void *d_offsets, uint64_t nreads,
                                         const void *d_recs, void *d_out_quals, uint64_t out_cap, uint64_t *n_out_bytes);
uint64_t sdt_gpu_qc_report_words(uint32_t cycles);
int sdt_gpu_qc_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint8_t *quals, uint64_t nbytes,
                     const uint64_t *offsets, uint64_t nreads, const sdt_read_trim *ranges, const uint8_t *classes,
                     const sdt_qc_params *params, uint64_t *report, uint64_t report_words);
int sdt_gpu_qc_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_quals, const void *d_offsets,
                            uint64_t nreads, const void *d_ranges, const void *d_classes, const sdt_qc_params *params,
                            void *d_report);
int sdt_gpu_asm_begin(sdt_ctx *ctx, const sdt_asm_params *params);
int sdt_gpu_asm_add(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nseqs,
                    sdt_seq_support *out);
int sdt_gpu_asm_add_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nseqs, void *d_out);
int sdt_gpu_asm_spectrum(sdt_ctx *ctx, uint64_t *matrix, uint64_t totals[4]);
int sdt_gpu_asm_end(sdt_ctx *ctx);
int sdt_gpu_compare_tables(sdt_ctx *a, sdt_ctx *b, const sdt_cmp_params *params, uint64_t *matrix, uint64_t totals[8]);
int sdt_gpu_compare_select(sdt_ctx *a, sdt_ctx *b, const sdt_cmp_range *range, uint64_t *keys, uint32_t *count_a,
                           uint32_t *count_b, uint64_t capacity, uint64_t *n);
int sdt_gpu_cluster_begin(sdt_ctx *ctx, const sdt_cluster_params *params, uint64_t info[8]);
int sdt_gpu_cluster_components(sdt_ctx *ctx, uint64_t *keys, sdt_cluster_comp *out, uint64_t capacity, uint64_t *n);
int sdt_gpu_cluster_lookup(sdt_ctx *ctx, const uint64_t *keys, uint64_t n, uint32_t *cluster);
int sdt_gpu_cluster_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, int paired, uint32_t pick_lo, uint32_t pick_hi, sdt_read_cluster *rec,
                          uint8_t *keep, uint64_t *n_kept);
int sdt_gpu_cluster_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                 int paired, uint32_t pick_lo, uint32_t pick_hi, void *d_rec, void *d_keep, uint64_t *n_kept);
int sdt_gpu_cluster_kept_reads(sdt_ctx *ctx, const uint64_t *pair_ranges, uint64_t n_ranges, uint32_t pick_lo,
                               uint32_t pick_hi, sdt_read_cluster *rec, uint64_t out_capacity, uint64_t *nreads,
                               uint64_t *n_kept);
int sdt_gpu_cluster_end(sdt_ctx *ctx);
int sdt_gpu_bubbles_begin(sdt_ctx *ctx, const sdt_bubble_params *params, uint64_t info[8]);
int sdt_gpu_bubbles_fetch(sdt_ctx *ctx, uint64_t first, uint64_t n, uint64_t *keys, sdt_bubble *rec);
int sdt_gpu_bubbles_paths(sdt_ctx *ctx, uint64_t first, uint64_t n, uint8_t *bases, uint64_t capacity, uint64_t *offsets);
int sdt_gpu_bubbles_end(sdt_ctx *ctx);
int sdt_gpu_unitigs_begin(sdt_ctx *ctx, const sdt_unitig_params *params, uint64_t info[8]);
int sdt_gpu_unitigs_fetch(sdt_ctx *ctx, uint64_t first, uint64_t n, uint64_t *keys, sdt_unitig *rec);
int sdt_gpu_unitigs_seqs(sdt_ctx *ctx, uint64_t first, uint64_t n, uint8_t *bases, uint64_t capacity, uint64_t *offsets);
int sdt_gpu_unitigs_links(sdt_ctx *ctx, uint64_t first, uint64_t n, sdt_unitig_link *links, uint64_t capacity,
                          uint64_t *n_links, uint64_t *n_dangling);
int sdt_gpu_unitigs_end(sdt_ctx *ctx);
int sdt_gpu_unitigs_index(sdt_ctx *ctx, uint64_t info[4]);
int sdt_gpu_unitigs_lookup(sdt_ctx *ctx, const uint64_t *keys, uint64_t n, sdt_unitig_pos *out);
int sdt_gpu_unitigs_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                          uint64_t nreads, sdt_read_path *rec, uint64_t *seg_offsets, sdt_path_seg *segs,
                          uint64_t capacity, uint64_t *n_segs);
int sdt_gpu_unitigs_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                 void *d_rec, void *d_seg_offsets, void *d_segs, uint64_t capacity, uint64_t *n_segs);
int sdt_gpu_unitigs_support_begin(sdt_ctx *ctx, const sdt_support_params *params);
int sdt_gpu_unitigs_support_add(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets,
                                uint64_t nreads, int paired);
int sdt_gpu_unitigs_support_add_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads,
                                       int paired);
int sdt_gpu_unitigs_support_unitigs(sdt_ctx *ctx, uint64_t first, uint64_t n, sdt_unitig_support *out);
int sdt_gpu_unitigs_support_links(sdt_ctx *ctx, uint64_t first, uint64_t n, sdt_link_support *out, uint64_t capacity,
                                  uint64_t *n_links);
int sdt_gpu_unitigs_support_junctions(sdt_ctx *ctx, sdt_unitig_junction *out, uint64_t capacity, uint64_t *n);
int sdt_gpu_unitigs_support_mates(sdt_ctx *ctx, sdt_mate_link *out, uint64_t capacity, uint64_t *n);
int sdt_gpu_unitigs_support_totals(sdt_ctx *ctx, uint64_t totals[12]);
int sdt_gpu_unitigs_support_end(sdt_ctx *ctx);

/* ---- introspection / measurement --------------------------------------------------------------- */
int sdt_gpu_key_words(const sdt_ctx *ctx);         /* 1 (K<=31), 2 (K<=63), 4 (K<=127) */
uint64_t sdt_gpu_table_slots(const sdt_ctx *ctx);
void *sdt_gpu_stream(const sdt_ctx *ctx);          /* hipStream_t the kernels are launched on */
/* launch on a caller-owned hipStream_t instead (NULL = back to a private stream); used by the multi-GPU
 * driver so that RCCL collectives and our kernels are ordered by one stream */
int sdt_gpu_set_stream(sdt_ctx *ctx, void *hip_stream);
/* HIP-event timing of the dominant (chop+insert) kernel accumulated since the last call with reset!=0:
 * total milliseconds, number of launches, k-mer occurrences those launches processed. */
int sdt_gpu_kernel_time(sdt_ctx *ctx, int reset, double *ms, uint64_t *launches, uint64_t *kmers);
/* Where the time of pass 1 went, by stage (HIP events on the context's stream, summed since the last
 * sdt_gpu_kernel_time(reset != 0)), and the locality pipeline's counters since the last reset:
 *   counters[0] LDS nodes merged into the table   [1] k-mers that took the direct path out of a full LDS table
 *           [2] k-mers that took it because the chunk pool was exhausted   [3] early flushes of a full LDS table
 *           [4] / [5] level-1 / level-2 chunks of the last batch   [6] batches counted   [7] k-mers per batch the pools hold
 *           [8..11] k_sk_count: 100 MHz clock ticks summed over workgroups in set-up / tile fill / counting / merging
 *           [12..15] k_sk_scatter_reads: the same for tile staging / window minima / run starts / emission */
#define SDT_STAGE_DIRECT      0   /* k_count_reads / k_insert_records: one atomic per occurrence */
#define SDT_STAGE_SK_SCATTER  1   /* k_sk_scatter_reads: chop + minimizers + level-1 scatter */
#define SDT_STAGE_SK_SPLIT    2   /* chunk lists + k_sk_scatter_records (level 2) */
#define SDT_STAGE_SK_COUNT    3   /* k_sk_count: LDS counting + merges */
#define SDT_STAGE_SK_FOLD     4   /* (ABI 7: the fold of the node log; always 0 now) */
#define SDT_NSTAGES           5
#define SDT_NCOUNTERS         20   /* [16] distinct records of the count stage's tiles, [17] records (level-2), [18] k-mers of the distinct records,
                                    * [19] table slots handed to k_clear since the last sdt_gpu_reset: what the level-1 scatter's fused launches left of the deferred
                                    * clear.  Counted on the host when the k_clear is enqueued; where a replay launch has already cleared the whole table on the
                                    * device (a pool that ran out of chunks), that k_clear finds it so and stores nothing, and is counted all the same */
int sdt_gpu_stage_times(sdt_ctx *ctx, double ms[SDT_NSTAGES], uint64_t counters[SDT_NCOUNTERS]);
/* the device table's slot hash of a canonical key (host-callable, identical to the device function) */
uint64_t sdt_owner_hash(const uint64_t *key_words_msw_first, int nwords);

#ifdef __cplusplus
}
#endif
#endif
