// sdt_ctx.hpp -- the device context behind the C ABI (include/sdt_gpu.h) and what the translation units of the library share:
//   sdt_gpu.hip       context life cycle, node table (growth, scans, export / import), the direct pass-1 family, host-buffer pushes
//   sdt_pipeline.hip  the locality pipeline's host side: pools, level-1 / level-2 scatter launches, the count stage's plan + launches
//   sdt_sharded.hip   multi-GPU: the exchange of level-1 chunks between the ranks, communicator glue
//   sdt_pass2.hip     second read pass (prlRead2edge): path words, patch table, k_map_reads, arcs
//   sdt_mapstage.hip  the map stage (prlContig2nodes / prlRead2Ctg)
//   sdt_search.hip    read-only questions to the counted table: batch k-mer search, per-read k-mer coverage
//   sdt_correct.hip   substitution errors of reads corrected against the counted table; the kept reads back to the host
//   sdt_select.hip    in-silico read normalisation against the counted table; a 2-bit stream compacted to the reads kept
//   sdt_trim.hip      reads cut back to their longest solid stretch against the counted table; a 2-bit stream compacted to kept ranges
//                     (these four read stages share a host layer of their own: sdt_readstage.hpp over sdt_read_plan.h, sdt_compact.hpp)
//   sdt_screen.hip    reads screened against reference sequences: a k-mer set of its own that the context keeps (one of the stages in
//                     front of pass 1 that need no table, like sdt_dedup.hip, sdt_clip.hip, sdt_overlap.hip, sdt_complexity.hip, sdt_quality.hip)
//   sdt_asm.hip       an assembly scored against the counted table: per-sequence support records, a copy number per node, the spectrum
//   sdt_compare.hip   two counted tables compared: the joint count spectrum and the k-mers within given ranges of both counts (the one
//                     unit whose entry points take two contexts)
//   sdt_cluster.hip   the counted table as a graph: its connected components, one label per slot, and the reads' clusters
//   sdt_unitig.hip    its unitigs and their links; sdt_thread.hip the reads as paths over them; sdt_support.hip what the reads support of them
//   sdt_bubble.hip    the counted table as a graph again: its bubbles (two non-branching paths between two k-mers), listed and re-walked
//   sdt_gpu_graph.hip the graph phases (own view of the context: sdt_internal.hpp GraphView)
// Not part of the ABI: nothing here is visible to a caller of libsdt_gpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <vector>
#include <new>
#include <thread>
#include <mutex>
#include <atomic>

#include "sdt_internal.hpp"
#include "sdt_superkmer.cuh"

using namespace sdt;
using sdti::fail;
#include "sdt_comm.cuh"
#include "sdt_shard_plan.h"
static_assert(SHARD_NB1 == SK_NB1, "the exchange plan and the pipeline agree about the level-1 buckets");

struct ArcEnt;                 // sdt_map_kernels.cuh

struct EventPair {
	hipEvent_t a, b;
	uint64_t kmers;
	int stage;               // SDT_STAGE_*
};

struct sdt_ctx {
	int device = 0;
	int K = 0;
	int nw = 1;
	uint64_t slots = 0;
	void *d_ent = nullptr;
	uint32_t *d_aux = nullptr;
	uint64_t *d_first = nullptr;       // SDT_FLAG_TRACK_FIRST
	// The clear DEBT: sdt_gpu_reset does not clear the table, it notes here that the slots [clear_lo, clear_hi) of entries, aux and first
	// still have to be cleared.  The first fused launches of the level-1 scatter pay it off (sdt_clear_plan.h), settle_clear pays what is
	// left with k_clear.  Only reset creates debt, and no code but those launches may see a table with debt: every entry point of the
	// library begins with SDT_ENTER (which settles) -- except the read pushes that end in launch_count (SDT_ENTER_LAZY:
	// they settle inside, where they stop fusing), reset (SDT_ENTER_LAZY: it replaces the debt) and destroy (it drops it).
	uint64_t clear_lo = 0, clear_hi = 0;
	uint64_t host_cleared = 0;         // slots settle_clear has handed to k_clear since the last reset (sdt_gpu_stage_times)
	uint64_t ord_base = 0, ord_stride = 1;
	Stats *d_stats = nullptr;
	Stats *h_stats = nullptr;          // pinned
	unsigned long long *d_hist = nullptr;
	hipStream_t stream = nullptr, copy_stream = nullptr;
	bool own_stream = true;
	// host-batch staging (double buffered)
	// A ring of NSTAGE device buffers.  A pushed batch is COPIED at once (copy stream) and queued; its kernels are launched
	// from the queue.  The one thing that blocks the host for long is a flush of the locality pipeline (two host syncs for
	// the chunk lists: ~30 ms per 2^31 k-mers), and while the host is blocked nobody feeds the copy engine -- so a launch
	// that needs a flush is put off until STAGE_AHEAD copies are queued behind it: the copies then run while the host waits
	// (without this the PCIe-inclusive rate was compute + copy, not max(compute, copy): 50 vs 76 G k-mers/s resident).
	static constexpr int NSTAGE = 48, STAGE_AHEAD = 32;
	uint32_t *d_words[NSTAGE] = {};
	uint64_t *d_offs[NSTAGE] = {};
	uint64_t cap_words[NSTAGE] = {}, cap_offs[NSTAGE] = {};
	hipEvent_t buf_free[NSTAGE] = {}, copied[NSTAGE] = {};
	int next_buf = 0;
	struct Staged { const uint32_t *dw; uint64_t *dof; uint64_t nreads, maxlen, ord_base, ord_stride; int slot; uint64_t fixed_len; };
	std::vector<Staged> staged;        // copied (or being copied), not yet launched: [staged_head, size)
	size_t staged_head = 0;
	bool draining = false;
	uint64_t push_ord_base = 0, push_ord_stride = 1;      // ordinals of the next PUSHED batch (ord_base / ord_stride: of the next LAUNCHED one)
	uint64_t push_ticket = 0;          // pushes issued so far: ticket t's host buffers are free once copied[(t - 1) % NSTAGE] has passed
	uint64_t expect_kmers = 0;         // sdt_gpu_hint_total_kmers
	// bookkeeping for growth: upper bound of distinct nodes without syncing
	uint64_t distinct_known = 0;       // as of the last sync
	uint64_t kmers_known = 0;          // occurrences counted as of the last sync (new nodes per occurrence: bound of the next launch)
	uint64_t kmers_since_sync = 0;     // launched since then (an upper bound of the new nodes they may bring)
	uint64_t hard_since_sync = 0;      // k-mers launched since then by the locality pipeline, whatever its own bound said
	uint64_t kmers_total_host = 0;
	uint64_t kmers_offered = 0;        // upper bound of the k-mers handed to pass 1 since the last reset (picks the kernel family)
	uint32_t flags = 0;
	// locality pipeline (sdt_superkmer.cuh): chunk pools of the two scatter levels, chunk lists, pending work
	struct SkState {
		bool ready = false;
		uint64_t cap_kmers = 0;            // k-mers the pools are sized for (one batch)
		bool cap_is_max = false;           // the device has no room for larger pools: do not try again
		uint64_t pending_kmers = 0;        // scattered into pool 1, not yet counted
		SkPool p1 = {nullptr, nullptr, nullptr, 0}, p2 = {nullptr, nullptr, nullptr, 0};
		unsigned long long *cursors = nullptr;   // [wgs][SK_NB1] open chunks of the level-1 scatter
		unsigned long long *blk = nullptr;       // [wgs] block of chunk ids each workgroup is handing out
		uint32_t wgs = 0;
		uint32_t *cnt1 = nullptr, *off1 = nullptr, *fill1 = nullptr, *list1 = nullptr;
		uint32_t *cnt2 = nullptr, *off2 = nullptr, *fill2 = nullptr, *list2 = nullptr;
		unsigned long long *kmers2 = nullptr, *kpre2 = nullptr;
		SkItem *items = nullptr;
		uint32_t items_cap = 0;
		uint4 *citems = nullptr, *h_citems = nullptr;       // work items of k_sk_count: [c0, c1) in list2 + their final buckets (device / pinned; sdt_count_plan.h)
		uint32_t citems_cap = 0;
		uint32_t *next_item = nullptr;                      // one counter per k_sk_count launch
		uint16_t *cut = nullptr;                            // [cut_cap] per read of a fused scatter launch: emissions made before it was cut short
		uint32_t *cut_flag = nullptr;                       // (sdt_sk_scatter_seq.cuh: SkFuse)
		uint64_t cut_cap = 0;
		uint32_t *h_off1 = nullptr, *h_off2 = nullptr;      // pinned
		unsigned long long *h_kpre2 = nullptr;              // pinned
		SkItem *h_items = nullptr;                          // pinned
		bool flushing = false;
		// statistics of the last flush (sdt_gpu_pipeline_stats)
		uint64_t st_records = 0, st_chunks1 = 0, st_chunks2 = 0, st_flushes = 0;
		uint32_t stream_flushes = 0;   // flushes since the last reset (sk_batch_limit)
		uint64_t l2_in_total = 0;      // k-mers that entered the count stage (sum of the level-2 bucket sizes): Stats.sk_counted must match
		bool exchanged = false;        // records left for / came from other ranks: Stats.sk_emitted is not this rank's input
	} sk;
	// multi-GPU (sdt_comm.cuh): communicator + double-buffered send / receive chunk buffers of the exchange
	Comm comm;
	struct Shard {
		uint64_t *send[2] = {nullptr, nullptr}, *recv[2] = {nullptr, nullptr};       // chunk payloads
		uint32_t *send_meta[2] = {nullptr, nullptr}, *recv_meta[2] = {nullptr, nullptr};
		uint32_t *iota = nullptr;                                                    // identity chunk list of a receive buffer
		uint32_t send_chunks = 0, recv_chunks = 0;
		hipEvent_t ev_gather[2] = {nullptr, nullptr}, ev_xdone[2] = {nullptr, nullptr}, ev_l2[2] = {nullptr, nullptr};
		bool x_recorded[2] = {false, false}, l2_recorded[2] = {false, false};
		uint64_t round = 0;
		// what the last exchange delivered and sk_split has not consumed yet
		bool pending = false;
		int pending_slot = 0;
		uint32_t pending_items = 0;
		std::vector<SkItem> items;
		uint64_t kmers_scattered = 0;
		// which rank owns which level-1 buckets: contiguous ranges [ranges[r], ranges[r + 1]), balanced by the bucket
		// weights of a sample of the first call's reads (the same on every rank: the weights are all-gathered)
		bool have_ranges = false;
		uint32_t ranges[65] = {0};
	} sh;
	// second pass (prlRead2edge): reads kept from pass 1, path words, patch table, arcs
	struct KeptBatch { uint32_t *d_words; uint64_t *d_offs; uint64_t nwords, nreads, ord_base, ord_stride, maxlen; };
	std::vector<KeptBatch> kept;
	// kept batches live in a few large slabs (two hipMallocs per 32 MiB batch were thousands of synchronous calls on
	// the ingest path): bump allocation, everything is released together
	struct KeepSlab { uint8_t *p; size_t size, used; };
	std::vector<KeepSlab> keep_slabs;
	void *d_patch = nullptr;
	uint64_t patch_slots = 0;
	ArcEnt *d_arcs = nullptr;
	uint64_t arc_slots = 0;
	bool paths_loaded = false;
	uint64_t *d_idx = nullptr;         // slot -> index of the node in the host's visiting order (sdt_gpu_layout_apply / sdt_gpu_set_node_index)
	sdti::GraphExt *gx = nullptr;      // graph phases (sdt_gpu_graph.hip)
	uint64_t idx_slots = 0, idx_n = 0;
	// map stage (SDT_FLAG_CONTIG_INDEX): contig ordinal -> id, contig_array, staging for sdt_gpu_align_reads
	uint32_t *d_ctg_ids = nullptr;
	uint64_t ctg_ord = 0, ctg_ids_cap = 0;
	uint32_t *d_ctg_len = nullptr, *d_ctg_twin = nullptr;
	uint64_t num_ctg = 0;
	void *ab[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // words, offsets, align_len, read_info, hits
	size_t ab_cap[5] = {0, 0, 0, 0, 0};
	unsigned long long *d_hit_cursor = nullptr;
	bool index_final = false;            // k_finalize_contig_index has run: look-ups only from here on
	// k-mer search and read profiles (sdt_search.hip): the high halves of the counts past 65 535 as a small hash keyed by slot,
	// valid for one state of the table (hi_mode < 0: to be collected again -- every call that can move or count a node says so)
	uint64_t *d_hi = nullptr;
	uint64_t hi_slots = 0;
	int hi_mode = -1;
	unsigned long long *d_cov_flags = nullptr;      // [0] reads longer than promised, [1] slots with a high half, [2] edits (sdt_correct.hip) / reads kept (sdt_select.hip)
	// the reference screen (sdt_screen.hip): a hash set canonical k-mer -> reference of its own k; lives from screen_load to
	// screen_unload / destroy, nothing else touches it
	struct ScreenSet {
		void *tab = nullptr;               // slots of 16 bytes
		uint64_t slots = 0, n_kmers = 0;
		uint32_t k = 0, n_refs = 0;
	} screen;
	// the assembly tally (sdt_asm.hip): one byte per table slot, four to a 32-bit word, and the four totals; lives from asm_begin to
	// asm_end / destroy.  It belongs to one state of the table: search_cache_drop marks it stale, and a stale tally is refused, not read
	struct AsmTally {
		uint32_t *cn = nullptr;            // (slots + 3) / 4 words
		unsigned long long *totals = nullptr;      // [4] sequences, k-mers, found, solid; [4 ..] the matrix of the last asm_spectrum
		uint64_t slots = 0;                // the table's slots at asm_begin
		uint32_t min_count = 0, rows = 0;
		bool open = false, stale = false;
	} asmt;
	// the clustering (sdt_cluster.hip): one 32-bit label per table slot, the id of the node's cluster or 0xFFFFFFFF; lives from
	// cluster_begin to cluster_end / destroy.  The component list is small and stays on the host.  Like the tally it belongs to one
	// state of the table: search_cache_drop marks it stale, and a stale clustering is refused, not read
	struct Clustering {
		uint32_t *label = nullptr;         // slots words
		uint64_t slots = 0;                // the table's slots at cluster_begin
		std::vector<uint64_t> keys;        // clusters x nw words: the smallest k-mer of every cluster, in id order
		std::vector<uint64_t> count_sum;   // per cluster
		std::vector<uint32_t> nodes;       // per cluster
		bool open = false, stale = false;
	} cl;
	// the bubble list (sdt_bubble.hip): the records and their two words each, sorted, on the device from bubbles_begin to
	// bubbles_end / destroy; nothing per table slot.  bubbles_paths walks the table again from these, so the list belongs to one state of
	// the table like the clustering: stale once search_cache_drop, delow or a graph phase has said so
	struct Bubbles {
		uint64_t *keys = nullptr;          // n x 2 nw words: s, then t
		void *rec = nullptr;               // n records of 48 bytes
		uint64_t n = 0;
		uint64_t slots = 0;                // the table's slots at bubbles_begin
		uint32_t min_count = 0, max_count = 0, min_link = 0, max_len = 0;    // the rule of that begin (min_count: already max(min_count, 1))
		bool open = false, stale = false;
	} bb;
	// the unitig list (sdt_unitig.hip): the records and their two words each, sorted by the first word, and the second order by the
	// reverse complement of the last word that unitigs_links searches, on the device from unitigs_begin to unitigs_end / destroy; nothing
	// per table slot.  unitigs_seqs and unitigs_links read the table again, so the list goes stale where the bubble list does
	struct Unitigs {
		uint64_t *keys = nullptr;          // n x 2 nw words: x0, then the last word
		void *rec = nullptr;               // n records of 24 bytes
		uint64_t *idx_keys = nullptr;      // n x nw words: revcomp(last), ascending
		uint32_t *idx_id = nullptr;        // ... and the unitig of each
		void *lab = nullptr;               // unitigs_index (sdt_thread.hip): 8 B per table slot, (unitig, pos << 1 | s) or all ones; goes with the list
		// unitigs_support_begin (sdt_support.hip): one block -- 48 counters, 16 B per unitig of (segs, kmers), 8 x 8 B per unitig of link
		// slots, the junction set at 24 B and the mate set at 16 B per slot; goes with the list, stays across a second unitigs_index
		void *sup = nullptr;
		uint64_t sup_jn_slots = 0, sup_jn_cap = 0, sup_mt_slots = 0, sup_mt_cap = 0;      // slots: a power of two, or 0 = not kept
		uint64_t n = 0;
		uint64_t live = 0;                 // the live nodes of unitigs_begin (= the sum of the records' nodes)
		uint64_t slots = 0;                // the table's slots at unitigs_begin
		uint32_t min_count = 0, max_count = 0, min_link = 0;    // the rule of that begin (min_count: already max(min_count, 1))
		bool open = false, stale = false;
	} ug;
	// timing
	std::vector<EventPair> ev;
	size_t ev_used = 0;
	int cu_count = 256;
};

constexpr double MAX_LOAD = 0.70;
// the flat table: what the direct kernel family counts into (and grows)
template <int NW> inline Table<NW> flat_of(const sdt_ctx *c)
{
	Table<NW> t;
	t.ent = (Entry<NW> *)c->d_ent;
	t.aux = c->d_aux;
	t.fslots = c->slots;
	t.first = c->d_first;
	return t;
}

// the node table as every stage after pass 1 sees it
template <int NW> inline Table<NW> table_of(const sdt_ctx *c) { return flat_of<NW>(c); }
inline uint64_t view_slots(const sdt_ctx *c) { return c->slots; }

inline size_t entry_bytes(int nw) { return nw == 1 ? sizeof(Entry<1>) : nw == 2 ? sizeof(Entry<2>) : sizeof(Entry<4>); }

inline int scan_grid(const sdt_ctx *c, uint64_t items) { return sdti::scan_grid(c->cu_count, items); }

// (SDT_WAVE_BLOCKS: test hook -- the kernels that give every wavefront a read run in that many workgroups, so that a wavefront takes
// read after read of a small batch and what it carries from one to the next (an LDS strip, counters) is seen; 0: no hook.  The
// decision itself is wave_blocks of sdt_read_plan.h)
inline uint64_t wave_blocks_forced()
{
	static const int forced = sdt_knob_int(sdt_test_env("SDT_WAVE_BLOCKS"), 0);
	return forced > 0 ? (uint64_t)forced : 0;
}


// the table is about to change (nodes counted, moved or replaced): what sdt_search.hip derived from it is stale, and so is the
// assembly tally of sdt_asm.hip and the clustering of sdt_cluster.hip, which are kept by slot, and the bubble list of sdt_bubble.hip
// and the unitig list of sdt_unitig.hip, whose paths are walked in the table again
inline void search_cache_drop(sdt_ctx *c)
{
	c->hi_mode = -1;
	c->asmt.stale = true;
	c->cl.stale = true;
	c->bb.stale = true;
	c->ug.stale = true;
}

inline int env_int(const char *name, int dflt) { const char *v = getenv(name); return v && *v ? atoi(v) : dflt; }
inline int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- sdt_gpu.hip ----
int settle_clear(sdt_ctx *c);                  // what is left of the clear debt is cleared on c->stream; the debt is dropped
// the two ways into the library (tests/test_entry_forms.py: every function of include/sdt_gpu.h that takes a context begins with one)
#define SDT_ENTER_LAZY(c) HIPCHK(hipSetDevice((c)->device))
#define SDT_ENTER(c)                                  \
	do {                                              \
		SDT_ENTER_LAZY(c);                            \
		const int rc_enter_ = settle_clear(c);        \
		if (rc_enter_ != SDT_OK) return rc_enter_;    \
	} while (0)
uint64_t flat_slots_for(uint64_t nodes);
void *keep_alloc(sdt_ctx *c, size_t bytes);
void keep_release(sdt_ctx *c);
// slots [lo, slots); the gates: k_clear (sdt_table_kernels.cuh)
int launch_clear(sdt_ctx *c, void *ent, uint32_t *aux, uint64_t *first, uint64_t slots, uint64_t lo = 0, const uint32_t *only_if = nullptr,
                 const unsigned long long *unless = nullptr);
int alloc_table(sdt_ctx *c, uint64_t slots, void **ent, uint32_t **aux, uint64_t **first);
int sync_stats(sdt_ctx *c);
int grow_table(sdt_ctx *c, uint64_t need_nodes);
int ensure_room(sdt_ctx *c, uint64_t incoming);
EventPair *next_event(sdt_ctx *c);
size_t tile_smem_bytes(int max_tile_words);
int tile_words_for(uint64_t max_read_len);
int drain_pushes(sdt_ctx *c, bool force);      // batches that were pushed but not launched yet are launched (force: all of them)
// ---- sdt_pipeline.hip ----
int sk_flush(sdt_ctx *c);
void sk_free(sdt_ctx *c);
// ---- sdt_sharded.hip ----
void shard_free(sdt_ctx *c);
int sk_flush_sharded(sdt_ctx *c);
// (what the read stages on the counted table share -- sdt_search.hip, sdt_correct.hip, sdt_select.hip, sdt_trim.hip: sdt_readstage.hpp)
