/* sdt_pregraph.c -- `sdt-pregraph -s configFile -o outputGraph [-K kmer -p n_cpu -d kmerFreqCutoff]`
 *
 * The reference's `pregraph` command line (pregraph.c:118-204) over the MI355X hashing path
 * (include/sdt_gpu.h).  Same options, same K clamp (pregraph.c:38-59), same stdout phrases for the
 * counters, and <prefix>.kmerFreq byte-identical to the reference (freqStat, prlHashReads.c:994-1023).
 * -p is the number of host parser threads here (the reference's worker pool is the GPU now).
 * There is no CPU fallback: without a gfx950 device the program exits non-zero.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <assert.h>
#include <unistd.h>
#include <pthread.h>
#include <sys/stat.h>

#include "../sdt_knobs.h"
#include "../../../include/sdt_gpu.h"
#include "libcfg.h"
#include "seqio.h"
#include "readstream.h"
#include "pg_ranks.h"
#include "graph/graph.h"
#include "graph/par.h"
#include "graph/big.h"

#ifndef SDT_MAX_K
#define SDT_MAX_K 127        /* one binary covers the 31/63/127mer variants; --max-k emulates a smaller one */
#endif

static void usage(int max_k)
{
	printf("\npregraph -s configFile -o outputGraph [-K kmer -p n_cpu -d kmerFreqCutoff]\n");
	printf("  -s\t<string>\tconfigFile: the config file of reads\n");
	printf("  -o\t<string>\toutputGraph: prefix of output graph file name\n");
	printf("  -K\t<int>\t\tkmer(min 13, max %d): kmer size, [23]\n", max_k);
	printf("  -p\t<int>\t\tn_cpu: number of cpu for use, [8]\n");
	printf("  -d\t<int>\t\tkmerFreqCutoff: kmers with frequency no larger than KmerFreqCutoff will be deleted, [0]\n");
}

typedef struct {
	sdt_ctx *gpu;
	unsigned long long reads;
	/* --gpus N: chunk i of the stream is counted by rank i % N; one collective push per group of N chunks */
	int rank, nranks, keep_all, keep_mine, fill, have;
	unsigned long long kept_reads;     /* reads handed to sdt_gpu_keep_reads (a rank that owns no chunk of the input keeps none) */
	int K, hinted;
	uint64_t total_text;               /* bytes of all input files (0: unknown) */
	uint32_t *w;
	uint64_t *o, nw, n, cap_w, cap_o, ord_base, ord_stride;
	/* --gpus N without a rank that keeps every read: nobody scans foreign chunks (seqio.h: sdt_read_shard_skip_foreign).  The record
	 * counts of a group's chunks are gathered when the group is complete, and only then does a rank know the ordinals of its own */
	int defer;
	struct { int sid, stride, parity; uint64_t n; } grp[PG_MAX_RANKS];
	sdt_stream_ordinals ords;
} push_state;

/* millisecond phase timer on stderr (the reference's own lines on stdout have 1 s resolution) */
static double now_ms(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static double g_t_last, g_t_main;
static int g_quiet;                 /* --gpus N: ranks > 0 */
static void phase(const char *name)
{
	if (g_quiet) return;
	const double t = now_ms();
	fprintf(stderr, "[sdt-pregraph] %-28s %9.1f ms\n", name, t - g_t_last);
	g_t_last = t;
}

/* bytes of every file pass 1 will read (readstream.c's selection: asm_flags 1 or 3) */
static uint64_t input_bytes(const sdt_cfg *cfg)
{
	uint64_t total = 0;
	for (int i = 0; i < cfg->nlibs; i++) {
		const sdt_lib *l = &cfg->libs[i];
		if (l->asm_flag != 1 && l->asm_flag != 3) continue;
		char **lists[] = {l->f1, l->f2, l->q1, l->q2, l->p, l->f, l->q};
		const int counts[] = {l->nf1, l->nf2, l->nq1, l->nq2, l->np, l->nf, l->nq};
		for (int k = 0; k < 7; k++)
			for (int j = 0; j < counts[k]; j++) {
				struct stat sb;
				if (stat(lists[k][j], &sb) == 0) total += (uint64_t)sb.st_size;
			}
	}
	return total;
}

/* pooled batches (pinned buffers, seqio.h) are pushed asynchronously: the buffer goes back to the pool once its copy has left it,
 * a few pushes later */
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

static void count_reads_line(push_state *st, uint64_t n)
{
	const unsigned long long before = st->reads / 1000000ULL;
	st->reads += n;
	if (st->reads / 1000000ULL != before)
		printf("--- %lluth reads\n", st->reads / 1000000ULL * 1000000ULL);    /* prlHashReads.c:587-588 */
}

static int push_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	push_state *st = (push_state *)user;
	count_reads_line(st, b->nreads);
	static int parse_only = -1;                              /* SDT_PARSE_ONLY=1 (measurement): parse and pack, push nothing */
	if (parse_only < 0) parse_only = sdt_tuning_env("SDT_PARSE_ONLY") != NULL;
	if (parse_only) return 0;
	if (st->total_text && !st->hinted && b->text_bytes && b->nreads) {
		/* the size of the job from its first chunk: k-mers per byte of text x bytes of all files (the pools of the locality
		 * pipeline are then the job's from the first batch on) */
		uint64_t km = 0;
		for (uint64_t i = 0; i < b->nreads; i++) { const uint64_t len = b->offsets[i + 1] - b->offsets[i]; if (len > (uint64_t)st->K) km += len - (uint64_t)st->K + 1; }
		sdt_gpu_hint_total_kmers(st->gpu, (uint64_t)((double)km / (double)b->text_bytes * (double)st->total_text));
		st->hinted = 1;
	}
	sdt_gpu_set_read_ordinal(st->gpu, ord_base, ord_stride);
	if (b->pool_slot >= 0) {
		uint64_t ticket = 0;
		if (b->fixed_len ? SDT_CALL(sdt_gpu_push_reads_fixed_async, st->gpu, b->words, b->nwords, b->nreads, b->fixed_len, &ticket)
		                 : SDT_CALL(sdt_gpu_push_reads_async, st->gpu, b->words, b->nwords, b->offsets, b->nreads, &ticket)) return -1;
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

static int flush_group(push_state *st)
{
	static const uint32_t none[4] = {0, 0, 0, 0};
	static const uint64_t zero[1] = {0};
	if (st->defer) {
		/* who parsed what: one all-gather (a sum over vectors with one non-zero entry each) per group of nranks chunks, then every rank
		 * does the arithmetic of readstream.c for the group's chunks in order */
		int64_t cnt[PG_MAX_RANKS];
		if (st->nranks > PG_MAX_RANKS) { fprintf(stderr, "[rank %d] %d ranks: cnt[] and grp[] hold %d\n", st->rank, st->nranks, PG_MAX_RANKS); return -1; }
		memset(cnt, 0, sizeof cnt);
		if (st->have) cnt[st->rank] = (int64_t)st->grp[st->rank].n;
		if (SDT_CALL(sdt_gpu_allreduce_i64, st->gpu, cnt, st->nranks)) return -1;      /* (the record counts of a group) */
		for (int i = 0; i < st->fill; i++) {
			const uint64_t base = sdt_stream_ordinals_next(&st->ords, st->grp[i].sid, st->grp[i].stride, st->grp[i].parity, (uint64_t)cnt[i]);
			if (i == st->rank) { st->ord_base = base; st->ord_stride = (uint64_t)st->grp[i].stride; }
			count_reads_line(st, (uint64_t)cnt[i]);
		}
		if (st->have && st->keep_mine && st->n) {
			sdt_gpu_set_read_ordinal(st->gpu, st->ord_base, st->ord_stride);
			if (SDT_CALL(sdt_gpu_keep_reads, st->gpu, st->w, st->nw, st->o, st->n)) return -1;
			st->kept_reads += st->n;
		}
	}
	if (st->have) sdt_gpu_set_read_ordinal(st->gpu, st->ord_base, st->ord_stride);
	const int bad = SDT_CALL(sdt_gpu_push_reads_sharded, st->gpu, st->have ? st->w : none, st->have ? st->nw : 4, st->have ? st->o : zero, st->have ? st->n : 0);
	st->have = 0;
	st->fill = 0;
	return bad ? -1 : 0;
}

static int push_batch_sharded(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	push_state *st = (push_state *)user;
	if (st->defer) {
		if (b->owner < 0 || b->owner >= PG_MAX_RANKS || b->owner != st->fill) { fprintf(stderr, "[rank %d] chunk %llu out of turn\n", st->rank, (unsigned long long)b->chunk_index); return -1; }
		st->grp[b->owner].sid = b->stream_id; st->grp[b->owner].stride = (int)ord_stride; st->grp[b->owner].parity = b->stream_parity;
		st->grp[b->owner].n = b->count_unknown ? 0 : b->nreads;
	} else
		count_reads_line(st, b->nreads);
	if (!st->defer && ((st->keep_all && !b->counted_only) || (st->keep_mine && b->owner == st->rank)) && b->nreads) {
		/* the reads of the second pass stay resident: this rank's own share (every rank maps its reads), or -- rank 0 without that -- all */
		sdt_gpu_set_read_ordinal(st->gpu, ord_base, ord_stride);
		if (SDT_CALL(sdt_gpu_keep_reads, st->gpu, b->words, b->nwords, b->offsets, b->nreads)) return -1;
		st->kept_reads += b->nreads;
	}
	if (b->owner == st->rank && b->nreads) {                      /* mine: it waits for the end of its group */
		if (b->nwords > st->cap_w) { st->cap_w = b->nwords * 5 / 4; st->w = (uint32_t *)realloc(st->w, st->cap_w * 4); }
		if (b->nreads + 1 > st->cap_o) { st->cap_o = (b->nreads + 1) * 5 / 4; st->o = (uint64_t *)realloc(st->o, st->cap_o * 8); }
		if (!st->w || !st->o) { fprintf(stderr, "[rank %d] out of host memory for a batch of %llu reads\n", st->rank, (unsigned long long)b->nreads); return -1; }
		memcpy(st->w, b->words, b->nwords * 4);
		memcpy(st->o, b->offsets, (b->nreads + 1) * 8);
		st->nw = b->nwords; st->n = b->nreads; st->ord_base = ord_base; st->ord_stride = ord_stride;
		st->have = 1;
	}
	if (++st->fill == st->nranks)
		return flush_group(st);
	return 0;
}

/* arcs of several ranks in one array: equal (from, to) pairs become one arc -- multiplicities add up, the first occurrence is the
 * smallest.  Returns the number of arcs left (in the front of the arrays). */
typedef struct { uint64_t key, ord; uint32_t mult; } arc_rec;
static int arc_rec_cmp(const void *a, const void *b)
{
	const arc_rec *x = (const arc_rec *)a, *y = (const arc_rec *)b;
	return x->key < y->key ? -1 : (x->key > y->key ? 1 : (x->ord < y->ord ? -1 : (x->ord > y->ord)));
}
static uint64_t arcs_combine(uint32_t *from, uint32_t *to, uint32_t *mult, uint64_t *ord, uint64_t n)
{
	arc_rec *v = (arc_rec *)malloc((n + 1) * sizeof(arc_rec));
	if (!v) { fprintf(stderr, "out of host memory for %llu arcs\n", (unsigned long long)n); exit(1); }
	for (uint64_t i = 0; i < n; i++) { v[i].key = ((uint64_t)from[i] << 32) | to[i]; v[i].ord = ord[i]; v[i].mult = mult[i]; }
	qsort(v, n, sizeof(arc_rec), arc_rec_cmp);
	uint64_t m = 0;
	for (uint64_t i = 0; i < n;) {
		uint64_t j = i, sum = 0;
		while (j < n && v[j].key == v[i].key) sum += v[j++].mult;
		from[m] = (uint32_t)(v[i].key >> 32); to[m] = (uint32_t)v[i].key; ord[m] = v[i].ord;      /* (sorted: the smallest ordinal first) */
		mult[m] = sum > 0xFFFFFFFFULL ? 0xFFFFFFFFu : (uint32_t)sum;
		m++;
		i = j;
	}
	free(v);
	return m;
}

/* second pass (prlRead2edge): unpack each read and thread it through the edge graph */
typedef struct {
	graph_t *G;
	struct arcs *A;
	unsigned long long reads;
} arc_state;

static int arc_batch(void *user, const sdt_batch *b, uint64_t ord_base, uint64_t ord_stride)
{
	arc_state *st = (arc_state *)user;
	uint8_t *codes = NULL;
	size_t cap = 0;
	for (uint64_t r = 0; r < b->nreads; r++) {
		const uint64_t o = b->offsets[r], len = b->offsets[r + 1] - o;
		if (len > cap) { cap = len * 2 + 64; codes = (uint8_t *)realloc(codes, cap); }
		for (uint64_t i = 0; i < len; i++)
			codes[i] = (uint8_t)((b->words[(o + i) >> 4] >> (30 - 2 * ((o + i) & 15))) & 3u);
		arcs_add_read(st->G, st->A, codes, (int)len, ord_base + r * ord_stride);
	}
	st->reads += b->nreads;
	free(codes);
	return 0;
}

/* graph.h dev_walks: bring the device mirror up to date with what the host wrote, then take the walks of every
 * node from it (sdt_gpu_tip_walks) */
typedef struct { sdt_ctx *gpu; int nwk, indexed, by_index; } dev_state;     /* by_index: the device numbered the nodes itself (sdt_gpu_layout_apply) */

static void gather_keys(void *vc, uint64_t lo, uint64_t hi, int tid)
{
	(void)tid;
	void **a = (void **)vc;
	const graph_t *g = (const graph_t *)a[0];
	uint64_t *k = (uint64_t *)a[1];
	const int nwk = (int)(intptr_t)a[2];
	for (uint64_t i = lo; i < hi; i++)
		for (int w = 0; w < nwk; w++) k[i * nwk + w] = g->nodes[i].seq.w[4 - nwk + w];
}

/* what the second read pass needs of every node (sdt_gpu_load_paths): skip flag, linear, twin, edge id */
static void gather_paths(void *vc, uint64_t lo, uint64_t hi, int tid)
{
	(void)tid;
	void **a = (void **)vc;
	const graph_t *G = (const graph_t *)a[0];
	uint64_t *pk = (uint64_t *)a[1], *pw = (uint64_t *)a[2];
	const int nwk = (int)(intptr_t)a[3];
	for (uint64_t i = lo; i < hi; i++) {
		const gnode_t *nd = &G->nodes[i];
		if (pk) for (int w = 0; w < nwk; w++) pk[i * nwk + w] = nd->seq.w[4 - nwk + w];
		const int skip = nd->deleted || (nd->linear && !nd->inEdge);
		pw[i] = (uint64_t)skip | ((uint64_t)nd->linear << 1) | ((uint64_t)nd->twin << 2) | ((uint64_t)nd->l_links << 32);
	}
}

static void gather_dirty(void *vc, uint64_t lo, uint64_t hi, int tid)
{
	(void)tid;
	void **a = (void **)vc;
	const graph_t *g = (const graph_t *)a[0];
	uint64_t *k = (uint64_t *)a[1];
	uint32_t *l = (uint32_t *)a[2], *r = (uint32_t *)a[3];
	const int nwk = (int)(intptr_t)a[4];
	for (uint64_t j = lo; j < hi; j++) {
		const gnode_t *nd = &g->nodes[g->dlist[j]];
		if (k) for (int w = 0; w < nwk; w++) k[j * nwk + w] = nd->seq.w[4 - nwk + w];
		l[j] = nd->l_links;
		r[j] = nd->r_links | ((uint32_t)nd->linear << 24) | ((uint32_t)nd->deleted << 25);
	}
}

/* the device table mirrors the host graph: node order known to the device, nodes written since the last call sent over */
static int dev_mirror_sync_(graph_t *g);
static int dev_mirror_sync(graph_t *g)
{
	const double t0 = now_ms();
	const size_t dn = g->dn;
	const int rc = dev_mirror_sync_(g);
	if (sdt_env("SDT_TIMING") && !g_quiet) fprintf(stderr, "[device]   mirror sync: %zu nodes written by the host sent over in %.1f ms\n", dn, now_ms() - t0);
	return rc;
}
static int dev_mirror_sync_(graph_t *g)
{
	dev_state *D = (dev_state *)g->dev_user;
	const int nwk = D->nwk;
	if (!D->indexed) {
		uint64_t *k = (uint64_t *)malloc((g->n + 1) * (size_t)nwk * 8);
		void *ga[3] = {g, k, (void *)(intptr_t)nwk};
		par_for(0, g->n, 1 << 16, gather_keys, ga);
		const int rc = sdt_gpu_set_node_index(D->gpu, k, g->n);
		free(k);
		if (rc != SDT_OK) return pg_fail("sdt_gpu_set_node_index");
		D->indexed = 1;
	}
	if (g->dn && D->by_index) {                                /* what the host wrote goes over by node index: no keys, no look-ups */
		uint32_t *l = (uint32_t *)malloc(g->dn * 4), *r = (uint32_t *)malloc(g->dn * 4);
		void *da[5] = {g, NULL, l, r, (void *)(intptr_t)nwk};
		par_for(0, g->dn, 1 << 14, gather_dirty, da);
		const int rc = sdt_gpu_update_nodes_by_index(D->gpu, g->dlist, l, r, g->dn);
		free(l); free(r);
		if (rc != SDT_OK) return pg_fail("sdt_gpu_update_nodes_by_index");
	} else if (g->dn) {
		uint64_t *k = (uint64_t *)malloc(g->dn * (size_t)nwk * 8);
		uint32_t *l = (uint32_t *)malloc(g->dn * 4), *r = (uint32_t *)malloc(g->dn * 4);
		void *da[5] = {g, k, l, r, (void *)(intptr_t)nwk};
		par_for(0, g->dn, 1 << 14, gather_dirty, da);
		const int rc = sdt_gpu_update_nodes(D->gpu, k, l, r, g->dn);
		free(k); free(l); free(r);
		if (rc != SDT_OK) return pg_fail("sdt_gpu_update_nodes");
	}
	return 0;
}

/* graph_index_hook: the device knows every node's place in the host array, let it build the host's look-up index */
static int dev_index_hook(graph_t *g, void *user)
{
	dev_state *D = (dev_state *)user;
	g->dev_user = D;
	const double t0 = now_ms();
	if (dev_mirror_sync(g) != 0) exit(1);
	const double t1 = now_ms();
	uint64_t cap = 1024;
	while (cap < 2 * g->n + 2) cap <<= 1;
	if (g->index64) {                                                    /* a graph past 2^32 nodes: 64-bit entries (calloc'ed by graph.c) */
		if (SDT_CALL(sdt_gpu_build_host_index64, D->gpu, g->index64, g->index_mask + 1)) exit(1);
	} else {
		g->index = (uint32_t *)malloc(cap * sizeof(uint32_t));
		g->index_mask = cap - 1;
		if (!g->index || SDT_CALL(sdt_gpu_build_host_index, D->gpu, g->index, cap)) exit(1);
	}
	if (sdt_env("SDT_TIMING")) fprintf(stderr, "[graph]      node order to the device %.1f ms, index built + copied back %.1f ms\n", t1 - t0, now_ms() - t1);
	return 0;
}

static int dev_edge_ports_hook(graph_t *g, uint64_t **records, uint64_t *nr)
{
	dev_state *D = (dev_state *)g->dev_user;
	if (dev_mirror_sync(g) != 0) return 1;
	uint64_t cap = g->n / 8 + 4096;
	for (;;) {
		uint64_t *rec = (uint64_t *)malloc(cap * 17 * sizeof(uint64_t));
		if (!rec) { fprintf(stderr, "out of memory for %llu port records\n", (unsigned long long)cap); return 1; }
		const int rc = sdt_gpu_edge_ports(D->gpu, rec, cap, nr);
		if (rc == SDT_OK) { *records = rec; return 0; }
		free(rec);
		if (rc == SDT_EFULL && *nr > cap) { cap = *nr; continue; }
		return pg_fail("sdt_gpu_edge_ports");
	}
}

static int dev_build_edges_hook(graph_t *g, uint64_t **records, int *key_words, uint64_t *n_edges, uint64_t *num_ed, char **bases, uint64_t *n_bases)
{
	dev_state *D = (dev_state *)g->dev_user;
	if (dev_mirror_sync(g) != 0) return 1;
	const int rc = sdt_gpu_build_edges(D->gpu, n_edges, num_ed, n_bases);
	if (rc == SDT_ESTATE && strstr(sdt_gpu_last_error(), "does not lead back")) return 2;       /* not symmetric: the sequential way */
	if (rc != SDT_OK) return pg_fail("sdt_gpu_build_edges");
	const int rw = 4 + 2 * D->nwk;
	uint64_t *rec = (uint64_t *)malloc((*n_edges + 1) * (size_t)rw * sizeof(uint64_t));
	char *b = (char *)malloc(*n_bases + 16);
	if (!rec || !b) { fprintf(stderr, "out of memory for %llu edges\n", (unsigned long long)*n_edges); return 1; }
	if (SDT_CALL(sdt_gpu_fetch_records, D->gpu, rec, *n_edges * (uint64_t)rw) || SDT_CALL(sdt_gpu_fetch_edge_bases, D->gpu, b, *n_bases)) return 1;
	*records = rec;
	*bases = b;
	*key_words = D->nwk;
	return 0;
}

static int dev_minor_out_hook(graph_t *g, double threshold, uint64_t **records, uint64_t *nj, uint64_t *nr)
{
	dev_state *D = (dev_state *)g->dev_user;
	if (dev_mirror_sync(g) != 0) return 1;
	const double t0 = now_ms();
	if (SDT_CALL(sdt_gpu_minor_out_labelled, D->gpu, threshold, nj, nr)) return 1;
	const double t1 = now_ms();
	uint64_t *rec = (uint64_t *)malloc((*nr + 1) * MO_RW * sizeof(uint64_t));
	if (!rec) { fprintf(stderr, "out of memory for %llu junction records\n", (unsigned long long)*nr); return 1; }
	if (SDT_CALL(sdt_gpu_fetch_records, D->gpu, rec, *nr * MO_RW)) { free(rec); return 1; }
	if (sdt_env("SDT_TIMING") && !g_quiet) fprintf(stderr, "[device]   junction dry run + components %.1f ms, %llu + %llu records fetched in %.1f ms\n", t1 - t0, (unsigned long long)*nj, (unsigned long long)(*nr - *nj), now_ms() - t1);
	*records = rec;
	return 0;
}

/* removeMinorOut's commit on the device, the long components on the host's threads at the same time (graph.h) */
static int dev_minor_out_commit_begin_hook(graph_t *g, double threshold, uint64_t **skipped, uint64_t *n_skipped, uint64_t *n_skipped_records)
{
	dev_state *D = (dev_state *)g->dev_user;
	if (dev_mirror_sync(g) != 0) return 1;
	const double t0 = now_ms();
	uint64_t nj = 0, nr = 0, largest = 0, nsk = 0, nskr = 0;
	if (SDT_CALL(sdt_gpu_minor_out_labelled, D->gpu, threshold, &nj, &nr)) return 1;
	const double t1 = now_ms();
	/* one lane walks a component at about a microsecond per dependent access (~100 us per visit); a host thread takes ~150 ns */
	/* (the device's lanes and the host's threads work side by side: at 200 M reads 1536 / 2048 / 2560 / 3072 / 4096 visits per component gave
	 * 983 / 895 / 829 / 813 / 1020 ms for the whole pass -- past 3072 the host waits for the longest lane, profiles/r5/README.md) */
	/* Round 6: the limit follows the size of the job.  The device's part lasts as long as its longest lane -- limit x ~50 us, whatever the
	 * job --, the host's part grows with the visits of the components past the limit: 3072 is where they meet at 16.5 M visits (200 M
	 * reads); at 1.8 M visits (8 M reads) the host was done with its six long components after 7 ms and then waited 154 ms for the lanes of
	 * 3072 visits (profiles/r6/e2e_8M_se_ours_only.json).  visits / 5000, within 256 .. 3072. */
	uint64_t by_size = nj / 5000;
	if (by_size < 256) by_size = 256;
	if (by_size > 3072) by_size = 3072;
	const uint64_t max_comp = sdt_test_env("SDT_COMMIT_MAX_COMPONENT") ? strtoull(sdt_test_env("SDT_COMMIT_MAX_COMPONENT"), NULL, 10) : by_size;
	if (SDT_CALL(sdt_gpu_minor_out_commit_begin, D->gpu, threshold, max_comp, &largest, &nsk, &nskr)) return 1;
	const double t2 = now_ms();
	uint64_t *sk = (uint64_t *)malloc((nskr + 1) * MO_RW * sizeof(uint64_t));
	if (!sk) { fprintf(stderr, "out of memory for %llu records\n", (unsigned long long)nskr); return 1; }
	if (SDT_CALL(sdt_gpu_fetch_skipped, D->gpu, sk, nskr)) return 1;
	if (nsk) *skipped = sk; else { free(sk); *skipped = NULL; }
	*n_skipped = nsk;
	*n_skipped_records = nskr;
	if (sdt_env("SDT_TIMING") && !g_quiet)
		fprintf(stderr, "[device]   junction dry run + components %.1f ms (%llu visits, largest component %llu), components + long ones gathered %.1f ms, %llu records of long components fetched in %.1f ms\n",
		        t1 - t0, (unsigned long long)nj, (unsigned long long)largest, t2 - t1, (unsigned long long)nskr, now_ms() - t2);
	return 0;
}

static int dev_minor_out_commit_finish_hook(graph_t *g, uint64_t *off, uint64_t *linear)
{
	dev_state *D = (dev_state *)g->dev_user;
	const double t0 = now_ms();
	uint64_t nw = 0;
	if (SDT_CALL(sdt_gpu_minor_out_commit_finish, D->gpu, off, linear, &nw)) return 1;
	const double t1 = now_ms();
	uint64_t *node = (uint64_t *)malloc((nw + 1) * sizeof(uint64_t));
	uint32_t *l = (uint32_t *)malloc((nw + 1) * sizeof(uint32_t)), *r = (uint32_t *)malloc((nw + 1) * sizeof(uint32_t));
	if (!node || !l || !r) { fprintf(stderr, "out of memory for %llu written nodes\n", (unsigned long long)nw); return 1; }
	if (SDT_CALL(sdt_gpu_fetch_written, D->gpu, node, l, r, nw)) return 1;
	const double t2 = now_ms();
	graph_apply_written(g, node, l, r, nw);
	free(node); free(l); free(r);
	if (sdt_env("SDT_TIMING") && !g_quiet)
		fprintf(stderr, "[device]   waited %.1f ms for the device's visits + marking + list, %llu written nodes fetched in %.1f ms, applied in %.1f ms\n",
		        t1 - t0, (unsigned long long)nw, t2 - t1, now_ms() - t2);
	return 0;
}

static int dev_walks_hook(graph_t *g, int thin, int cut_len, uint64_t **records, uint64_t *nr)
{
	dev_state *D = (dev_state *)g->dev_user;
	if (dev_mirror_sync(g) != 0) return 1;
	const double t0 = now_ms();
	if (SDT_CALL(sdt_gpu_tip_walks_labelled, D->gpu, thin, cut_len, nr)) return 1;
	const double t1 = now_ms();
	uint64_t *rec = (uint64_t *)malloc((*nr + 1) * 3 * sizeof(uint64_t));
	if (!rec) { fprintf(stderr, "out of memory for %llu walk records\n", (unsigned long long)*nr); return 1; }
	if (SDT_CALL(sdt_gpu_fetch_records, D->gpu, rec, *nr * 3)) { free(rec); return 1; }
	if (sdt_env("SDT_TIMING") && !g_quiet) fprintf(stderr, "[device]   walks + components %.1f ms, %llu records fetched in %.1f ms\n", t1 - t0, (unsigned long long)*nr, now_ms() - t1);
	*records = rec;
	return 0;
}

/* *.vertex written beside the second read pass (the device is busy, the host is not), then the node array is let go */
typedef struct { graph_t *G; const char *prefix; uint64_t nv; int have; pthread_t th; } vx_job;      /* have: the thread was started */
static void *vertex_thread(void *v)
{
	vx_job *J = (vx_job *)v;
	J->nv = graph_write_vertex(J->G, J->prefix);
	graph_free_later(J->G->nodes, J->G->index, J->G->dirty, J->G->dlist);
	J->G->nodes = NULL; J->G->index = NULL; J->G->dirty = NULL; J->G->dlist = NULL;
	return NULL;
}

/* One job: the options as given, the route they select -- decided once, in decide_route() -- and what one phase hands to the next */
typedef struct {
	char cfgfile[4096], prefix[4096];
	int K, threads, d, dd, max_k, device, gpus, share_device, hash_only, host_map, host_walks;
	unsigned long long est;
	/* the route */
	int device_graph;              /* layout, cutting and edges on the device; otherwise the host replays the layout from exported arrays */
	int per_rank_map;              /* --gpus N: every rank keeps the reads it parsed and maps them itself once rank 0 has the graph */
	int keep_all;                  /* --gpus N: rank 0 parses and keeps every read, the second pass is its device's alone */
	/* the run */
	int rank, max_read_len, my_threads, nwk, nwv;
	pg_boot *boot;
	sdt_cfg cfg;
	time_t t_start;
	size_t chunk;
	sdt_ctx *gpu;
	uint64_t kmers, nodes, my_nodes, kept_reads, text_parsed, text_seen;
} job_t;

/* the options; 0, or the exit code */
static int parse_options(job_t *J, int argc, char **argv)
{
	int have_s = 0, have_o = 0, c;
	static struct option longopts[] = {{"max-k", required_argument, 0, 1000}, {"device", required_argument, 0, 1001},
	                                   {"est-distinct", required_argument, 0, 1002}, {"hash-only", no_argument, 0, 1003}, {"host-map", no_argument, 0, 1004}, {"host-walks", no_argument, 0, 1005},
	                                   {"gpus", required_argument, 0, 1006}, {"share-device", no_argument, 0, 1007},
	                                   {0, 0, 0, 0}};
	J->K = 23; J->threads = 8; J->dd = 5; J->gpus = 1;
	/* accept an optional leading "pregraph" sub-command like the reference's dispatcher (main.c:49-106) */
	if (argc > 1 && strcmp(argv[1], "pregraph") == 0) { argv++; argc--; }
	while ((c = getopt_long(argc, argv, "a:s:o:K:p:d:Di:n", longopts, NULL)) != -1) {
		switch (c) {
		case 's': have_s = 1; snprintf(J->cfgfile, sizeof J->cfgfile, "%s", optarg); break;
		case 'o': have_o = 1; snprintf(J->prefix, sizeof J->prefix, "%s", optarg); break;
		case 'K': J->K = atoi(optarg); break;
		case 'p': J->threads = atoi(optarg); break;
		case 'd': J->d = atoi(optarg) >= 0 ? atoi(optarg) : 0; break;       /* pregraph.c:159 */
		case 'i': J->dd = atoi(optarg) >= 0 ? atoi(optarg) : 0; break;      /* pregraph.c:170-173 */
		case 'a': graph_init_kmerset_size = atoi(optarg); break;             /* pregraph.c:160-162; layout replay, graph/graph.c */
		case 'D': break;                                                     /* accepted, commented out upstream (pregraph.c:155-158) */
		case 'n':
			fprintf(stderr, "-n (N-aware k-mers) is not supported: the reference path is broken (survey 9.3-q11)\n");
			return 1;
		case 1000: J->max_k = atoi(optarg); break;
		case 1001: J->device = atoi(optarg); break;
		case 1002: J->est = strtoull(optarg, NULL, 10); break;
		case 1003: J->hash_only = 1; break;
		case 1004: J->host_map = 1; break;
		case 1005: J->host_walks = 1; break;
		case 1006: J->gpus = atoi(optarg); break;             /* one process per GPU: devices --device .. --device + N - 1 */
		case 1007: J->share_device = 1; break;                /* validation: all ranks on --device, shared-memory transport */
		default:
			if (!have_s || !have_o) { usage(J->max_k ? J->max_k : SDT_MAX_K); return 255; }
		}
	}
	/* which reference binary is being stood in for: it fixes the words per printed k-mer and the bytes hash_kmer
	 * runs over (31mer / 63mer / 127mer); default = the smallest shipped variant that can hold K */
	if (J->max_k == 0) J->max_k = J->K <= 31 ? 31 : SDT_MAX_K;
	if (!have_s || !have_o) { usage(J->max_k); return 255; }
	if (J->d > 127) J->d = (signed char)J->d;                               /* deLowKmer is a char (survey q12) */
	/* pregraph.c:38-59 */
	if (J->K % 2 == 0) { J->K++; printf("K should be an odd number\n"); }
	if (J->K < 13) { J->K = 13; printf("K should not be less than 13\n"); }
	else if (J->K > J->max_k) J->K = J->max_k;
	return 0;
}

/* The route, from the options and the environment.  Nothing later re-derives it: the node-limit fallback (wide_node_index) is a
 * separate decision that needs the node count and never changes these. */
static void decide_route(job_t *J)
{
	J->device_graph = !J->host_map && !J->host_walks && J->threads <= 256 && !sdt_test_env("SDT_HOST_LAYOUT");
	/* --gpus N: every rank keeps the reads it parsed and maps them itself once rank 0 has the graph (the default path: layout, cutting
	 * and edges on rank 0's device); with --host-map / --host-walks the second pass is the host's, which reads the files again */
	J->per_rank_map = J->gpus > 1 && !J->hash_only && J->device_graph && !sdt_test_env("SDT_RANK0_MAP");
	J->keep_all = J->gpus > 1 && !J->hash_only && !J->host_map && !J->per_rank_map;
}

static void timing_preamble(job_t *J)
{
	J->t_start = time(NULL);
	g_t_last = g_t_main = now_ms();
	if (sdt_test_env("SDT_LAYOUT_CHECK")) setenv("SDT_KEEP_FIRST", "1", 0);      /* the check sorts by the first-occurrence ordinals once more */
	if (!sdt_env("SDT_TIMING")) return;
	/* how long the loader took to get here (process start from /proc/self/stat, in clock ticks since boot): what a caller's
	 * wall clock holds beyond "total inside main" is this plus the kernel's teardown of the address space after _exit */
	FILE *sf = fopen("/proc/self/stat", "r");
	char sb[2048];
	if (!sf) return;
	const size_t got = fread(sb, 1, sizeof sb - 1, sf);
	fclose(sf);
	sb[got] = 0;
	const char *q = strrchr(sb, ')');
	unsigned long long start = 0;
	int field = 2;
	for (q = q ? q + 1 : sb; *q && field < 22; q++) if (*q == ' ') field++;
	if (field == 22) start = strtoull(q, NULL, 10);
	struct timespec bt;
	clock_gettime(CLOCK_BOOTTIME, &bt);
	const double since = bt.tv_sec * 1e3 + bt.tv_nsec * 1e-6 - (double)start * 1e3 / (double)sysconf(_SC_CLK_TCK);
	fprintf(stderr, "[sdt-pregraph] %-28s %9.1f ms\n", "before main (loader)", since);
}

static void parser_threads(job_t *J)
{
	/* parser threads: the job's CPUs minus the pushing thread and the runtime's helpers -- under a CPU quota (cgroup cpu.max) one
	 * runnable thread too many throttles every thread of the process, the one that feeds the device included (200 M reads with
	 * -p 16 on 16 CPUs: 6.3 s against 1.6 s with -p 8).  -p stays the number of sets of the layout (graph.c). */
	const int threads = J->threads, gpus = J->gpus, usable = par_threads();
	const int cap = sdt_env("SDT_PARSE_THREADS") ? atoi(sdt_env("SDT_PARSE_THREADS")) : (usable > 4 ? usable - 3 : usable);
	int parse_threads = threads;
	if (parse_threads > cap) parse_threads = cap > 0 ? cap : 1;
	/* --gpus N: every rank parses its own chunks and nothing else (seqio.h: sdt_read_shard_skip_foreign), so the parser threads are
	 * shared out evenly -- two at least; when one rank keeps every read (SDT_RANK0_MAP, the way of rounds 2-4) rank 0 parses all of the
	 * text and gets most of the threads, the others only count records */
	J->my_threads = gpus == 1 ? parse_threads
	              : J->keep_all ? (J->rank == 0 ? (threads - (gpus - 1) > threads / 2 ? threads - (gpus - 1) : (threads + 1) / 2) : 2)
	              : (parse_threads / gpus > 2 ? parse_threads / gpus : 2);
}

/* the device of this rank and, with --gpus N, the communicator */
static int open_device(job_t *J)
{
	pg_boot *boot = J->boot;
	/* SDT_PIPELINE=1 (tests): the locality pipeline also for jobs below its 2^27 k-mer threshold */
	const uint32_t iflags = (J->hash_only ? 0 : (SDT_FLAG_TRACK_FIRST | ((J->host_map || J->gpus > 1) ? 0 : SDT_FLAG_KEEP_READS))) |
	                        (sdt_test_env("SDT_PIPELINE") ? SDT_FLAG_PARTITION : 0);
	if (SDT_CALL(sdt_gpu_init, &J->gpu, J->share_device ? J->device : J->device + J->rank, J->K, J->est / (unsigned long long)J->gpus, iflags)) return 1;
	if (J->gpus > 1 && J->share_device) {
		if (SDT_CALL(sdt_gpu_comm_init_shm, J->gpu, boot->name, J->rank, J->gpus)) return 1;
	} else if (J->gpus > 1) {
		if (J->rank == 0) {
			const int bad = SDT_CALL(sdt_gpu_comm_id, &boot->id);
			__sync_synchronize();
			boot->ready = bad ? -1 : 1;
		}
		while (!boot->ready) usleep(1000);
		if (boot->ready != 1) return 1;                              /* (rank 0 has said why) */
		if (SDT_CALL(sdt_gpu_comm_init, J->gpu, &boot->id, J->rank, J->gpus)) return 1;
	}
	phase("config + gpu init");
	return 0;
}

/* pass 1: every read parsed, packed and counted -- one GPU, or this rank's chunks of the stream */
static int pass1(job_t *J, push_state *st)
{
	int rc;
	memset(st, 0, sizeof *st);
	st->gpu = J->gpu; st->rank = J->rank; st->nranks = J->gpus; st->keep_all = J->keep_all && J->rank == 0;
	st->keep_mine = J->per_rank_map;
	J->chunk = sdt_test_env("SDT_CHUNK_BYTES") ? (size_t)strtoull(sdt_test_env("SDT_CHUNK_BYTES"), NULL, 10) : (size_t)(32u << 20);   /* (tests: many small chunks) */
	if (J->gpus == 1) {
		st->K = J->K;
		st->total_text = input_bytes(&J->cfg);
		if (!sdt_tuning_env("SDT_NO_PINNED_POOL")) sdt_pool_enable(sdt_gpu_host_alloc, sdt_gpu_host_free, J->my_threads + PUSH_DEPTH + 8);
		rc = sdt_stream_reads(&J->cfg, J->max_read_len, J->my_threads, J->chunk, 1, push_batch, st, NULL);
		if (rc == 0 && inflight_retire(J->gpu, 0) != 0) rc = -1;
		sdt_pool_disable();
	} else {
		sdt_read_shard_begin(J->rank, J->gpus, st->keep_all);
		/* (the same on every rank: only rank 0 has keep_all set, but whether ANY rank keeps everything is a property of the run) */
		st->defer = !J->keep_all;
		sdt_read_shard_skip_foreign(st->defer);
		sdt_stream_ordinals_init(&st->ords);
		rc = sdt_stream_reads(&J->cfg, J->max_read_len, J->my_threads, J->chunk, 1, push_batch_sharded, st, NULL);
		if (rc == 0 && st->fill) rc = flush_group(st);
		J->text_parsed = sdt_reader_bytes_parsed; J->text_seen = sdt_reader_bytes_seen;
		sdt_read_shard_begin(0, 1, 0);
	}
	J->kept_reads = st->kept_reads;
	if (rc != 0) { sdt_gpu_destroy(J->gpu); return 1; }
	return 0;
}

/* the counters of pass 1, -d, the linear mark and *.kmerFreq; 0, or the exit code */
static int count_and_freq(job_t *J, unsigned long long reads)
{
	sdt_ctx *gpu = J->gpu;
	uint64_t removed = 0, linear = 0;
	if (SDT_CALL(sdt_gpu_finish_count, gpu, &J->kmers, &J->nodes)) return 1;
	J->my_nodes = J->nodes;
	if (J->gpus > 1) {                                           /* the counters the reference prints are sums over its sets */
		int64_t v[2] = {(int64_t)J->kmers, (int64_t)J->nodes};
		if (SDT_CALL(sdt_gpu_allreduce_i64, gpu, v, 2)) return 1;
		J->kmers = (uint64_t)v[0]; J->nodes = (uint64_t)v[1];
	}
	if (sdt_env("SDT_TIMING") && !g_quiet) {
		double ms[SDT_NSTAGES];
		uint64_t cn[SDT_NCOUNTERS];
		if (sdt_gpu_stage_times(gpu, ms, cn) == SDT_OK)
			fprintf(stderr, "[ingest] consumer waited %.0f ms for the parsers, spent %.0f ms pushing; device stages: direct %.0f, scatter %.0f, split %.0f, count %.0f ms; %llu batches counted, %llu early flushes, %d parser threads\n",
			        sdt_reader_wait_ms, sdt_reader_fn_ms, ms[0], ms[1], ms[2], ms[3], (unsigned long long)cn[6], (unsigned long long)cn[3], J->my_threads);
	}
	if (sdt_env("SDT_TIMING") && !g_quiet && J->gpus > 1)
		fprintf(stderr, "[ingest] rank 0 of %d parsed %.1f of %.1f MB of text (%.3f of the input; the other chunks are their owners')\n", J->gpus,
		        J->text_parsed / 1e6, J->text_seen / 1e6, J->text_seen ? (double)J->text_parsed / (double)J->text_seen : 0.0);
	phase("parse + hash (GPU)");
	printf("time spent on hash reads: %ds, %llu reads processed\n", (int)(time(NULL) - J->t_start), reads);
	printf("%llu nodes allocated, %llu kmer in reads, %llu kmer processed\n", (unsigned long long)J->nodes,
	       (unsigned long long)J->kmers, (unsigned long long)J->kmers);
	if (J->d && SDT_CALL(sdt_gpu_delow, gpu, J->d, &removed)) return 1;
	int64_t hist[257];
	if (SDT_CALL(sdt_gpu_mark_and_hist, gpu, hist, &linear)) return 1;
	if (J->gpus > 1) {
		int64_t v[259];
		memcpy(v, hist, sizeof hist);
		v[257] = (int64_t)linear; v[258] = (int64_t)removed;
		if (SDT_CALL(sdt_gpu_allreduce_i64, gpu, v, 259)) return 1;
		memcpy(hist, v, sizeof hist);
		linear = (uint64_t)v[257]; removed = (uint64_t)v[258];
	}
	if (J->d) printf("%llu kmer removed\n", (unsigned long long)removed);
	printf("%llu linear nodes\n", (unsigned long long)linear);
	char name[4200];
	snprintf(name, sizeof name, "%s.kmerFreq", J->prefix);
	if (J->rank == 0) {
		FILE *fo = fopen(name, "w");
		if (!fo) { printf("Cannot open %s. Now exit to system...\n", name); return 255; }
		for (int i = 1; i < 256; i++)
			fprintf(fo, "%lld\n", (long long)hist[i]);
		fclose(fo);
	}
	phase("delow/mark/kmerFreq (GPU)");
	printf("time spent on pre-graph construction: %ds\n\n", (int)(time(NULL) - J->t_start));
	printf("deLowKmer %d, deLowEdge %d\n", J->d, 1);
	return 0;
}

/* Past 2^32 - 16 nodes (the reference's sets are 64-bit: inc/newhash.h:79-88 `ubyte8 size, count, max`) the device's graph phases
 * take their 64-bit node indices (sdt_gpu_set_graph_index_bits; the library would pick them by node count anyway): layout,
 * cutting and edges stay on the device, and the host's look-up index gets 64-bit entries (graph.c, from the device).  Where the
 * host route is taken anyway (--host-walks, --host-map, -p > 256, SDT_HOST_LAYOUT) the host replays the layout, builds its 64-bit
 * index itself and runs cutting and kmer2edges on its threads.  SDT_NODE_LIMIT moves the threshold so that the tests can take
 * these paths on a golden case.
 * This never changes the route: "graph phases on the host" (host_walks) is set only where device_graph is false already. */
static int wide_node_index(job_t *J, uint64_t nodes)
{
	const uint64_t node_limit = sdt_test_env("SDT_NODE_LIMIT") ? strtoull(sdt_test_env("SDT_NODE_LIMIT"), NULL, 10) : 0xFFFFFFF0ULL;
	if (nodes < node_limit) return 0;
	if (J->device_graph) {
		if (SDT_CALL(sdt_gpu_set_graph_index_bits, J->gpu, 64)) return 1;
		if (!g_quiet) fprintf(stderr, "[sdt-pregraph] %llu nodes: past the 32-bit node indices; the device runs layout, cutting and edges with 64-bit node indices\n",
		                      (unsigned long long)nodes);
		return 0;
	}
	if (!g_quiet) fprintf(stderr, "[sdt-pregraph] %llu nodes: past the 32-bit node indices of the device's graph phases; layout, cutting and edges run on the host\n",
	                      (unsigned long long)nodes);
	assert(!J->device_graph);
	J->host_walks = 1;
	graph_force_wide_index = 1;
	return 0;
}

/* --gpus N, a rank above 0 after pass 1: its shard goes to rank 0 through a segment of its own and its table back to the device; with
 * the second pass on every rank it then waits for the graph, maps its reads and leaves its arcs.  Returns the process's exit code. */
static int rank_after_pass1(job_t *J)
{
	pg_boot *boot = J->boot;
	sdt_ctx *gpu = J->gpu;
	const int rank = J->rank;
	pg_nodes sh;
	uint64_t n = 0;
	int64_t token = 0;
	int ok = 1;
	if (pg_nodes_map(&sh, rank, J->my_nodes, J->nwk, 1)) { fprintf(stderr, "[rank %d] shared memory for %llu nodes failed\n", rank, (unsigned long long)J->my_nodes); return 1; }
	if (SDT_CALL(sdt_gpu_export_nodes, gpu, sh.keys, sh.l, sh.r, sh.c, sh.first, J->my_nodes, &n)) return 1;
	if (SDT_CALL(sdt_gpu_allreduce_i64, gpu, &token, 1) ||          /* "my shard is in shared memory" */
	    SDT_CALL(sdt_gpu_allreduce_i64, gpu, &token, 1)) return 1;  /* "rank 0 has it" */
	pg_seg_close(&sh.seg, 1);
	/* the shard is with rank 0: its table, the ordinals and the pools of the locality pipeline go back to the device now, not
	 * when the graph arrives (under --share-device they would sit beside rank 0's graph buffers until then) */
	if (SDT_CALL(sdt_gpu_release_table, gpu)) return 1;
	if (J->per_rank_map) {
		/* wait for the graph (rank 0 lays it out, cuts it and builds the edges: seconds to minutes -- polled, not a collective with
		 * its deadline; the parent's death takes this process along), map my reads, leave my arcs */
		while (boot->paths_state == 0) usleep(2000);
		const uint64_t pn = boot->paths_n, qn = boot->patch_n;
		pg_paths pt;
		pg_arcs ar;
		uint64_t nreads2 = 0, narcs = 0;
		/* a rank that owned no chunk of the input (fewer chunks than ranks) kept no reads: it has nothing to map and leaves an
		 * empty arc list (sdt_gpu_map_reads would refuse: "the reads were not kept") */
		const int have_reads = J->kept_reads > 0;
		ar.seg.base = pt.seg.base = NULL;
		ok = boot->paths_state == 1;
		if (ok && pg_paths_map(&pt, pn, qn, J->nwk, 0)) { fprintf(stderr, "[rank %d] cannot map the path table\n", rank); ok = 0; }
		if (ok && have_reads && (SDT_CALL(sdt_gpu_import_paths, gpu, pt.pk, pt.pw, pn, pt.qk, pt.qi, qn, boot->num_ed) ||
		                         SDT_CALL(sdt_gpu_map_reads, gpu, &nreads2, &narcs))) ok = 0;
		pg_seg_close(&pt.seg, 0);
		if (ok && pg_arcs_map(&ar, rank, narcs, 1)) { fprintf(stderr, "[rank %d] no shared memory for %llu arcs\n", rank, (unsigned long long)narcs); ok = 0; }
		if (ok && have_reads && SDT_CALL(sdt_gpu_export_arcs, gpu, ar.from, ar.to, ar.mult, ar.ord, narcs, &narcs)) ok = 0;
		boot->arcs_n[rank] = narcs;
		boot->arcs_reads[rank] = nreads2;
		__sync_synchronize();
		boot->arcs_state[rank] = ok ? 1 : -1;
		while (ok && boot->paths_state == 1) usleep(2000);         /* rank 0 is reading them */
		pg_seg_close(&ar.seg, 1);
	}
	sdt_gpu_destroy(gpu);
	return ok ? 0 : 1;
}

/* the node table as host arrays (graph_build's input) */
typedef struct { uint64_t *keys, *first; uint32_t *l, *r, *c; } node_arrays;
static int node_arrays_alloc(node_arrays *A, uint64_t n, int nwk)
{
	A->keys = (uint64_t *)malloc((n + 1) * (size_t)nwk * 8); A->first = (uint64_t *)malloc((n + 1) * 8);
	A->l = (uint32_t *)malloc((n + 1) * 4); A->r = (uint32_t *)malloc((n + 1) * 4); A->c = (uint32_t *)malloc((n + 1) * 4);
	if (A->keys && A->first && A->l && A->r && A->c) return 0;
	fprintf(stderr, "out of host memory for %llu nodes\n", (unsigned long long)n);
	return 1;
}

/* --gpus N, rank 0 takes the shards of the other ranks.  The graph on the device: straight into its device table (it then lays the whole
 * graph out like a single-GPU run), nothing is gathered in host arrays.  Otherwise: every shard into host arrays, its own first, and
 * -- unless the second pass is the host's too -- the others' into its device table as well. */
static int gather_shards(job_t *J, const int64_t *sizes, node_arrays *A)
{
	const uint64_t n = J->nodes, mine = J->my_nodes;
	const int nwk = J->nwk, to_host = !J->device_graph;
	uint64_t got = 0, at = mine;
	int64_t token = 0;
	if (to_host && (node_arrays_alloc(A, n, nwk) || SDT_CALL(sdt_gpu_export_nodes, J->gpu, A->keys, A->l, A->r, A->c, A->first, mine, &got))) return 1;
	if (SDT_CALL(sdt_gpu_allreduce_i64, J->gpu, &token, 1)) return 1;   /* every shard is in shared memory */
	for (int r = 1; r < J->gpus; r++) {
		const uint64_t m_n = (uint64_t)sizes[r];
		pg_nodes sh;
		if (pg_nodes_map(&sh, r, m_n, nwk, 0)) { fprintf(stderr, "cannot map the shard of rank %d\n", r); return 1; }
		if (to_host) {
			memcpy(A->keys + at * nwk, sh.keys, m_n * (size_t)nwk * 8); memcpy(A->first + at, sh.first, m_n * 8);
			memcpy(A->l + at, sh.l, m_n * 4); memcpy(A->r + at, sh.r, m_n * 4); memcpy(A->c + at, sh.c, m_n * 4);
		} else if (SDT_CALL(sdt_gpu_import_nodes, J->gpu, sh.keys, sh.l, sh.r, sh.c, sh.first, m_n)) return 1;
		at += m_n;
		pg_seg_close(&sh.seg, 0);
	}
	if (SDT_CALL(sdt_gpu_allreduce_i64, J->gpu, &token, 1)) return 1;   /* the other ranks may go */
	if (!to_host) { phase("shards into rank 0's table"); return 0; }
	if (at != n) { fprintf(stderr, "shards hold %llu nodes, the counters say %llu\n", (unsigned long long)at, (unsigned long long)n); return 1; }
	if (!J->host_map && SDT_CALL(sdt_gpu_import_nodes, J->gpu, A->keys + mine * nwk, A->l + mine, A->r + mine, A->c + mine, A->first + mine, n - mine)) return 1;
	return 0;
}

/* the visiting order with the device: it sorts the nodes by (set, first occurrence) and sends the keys, the host
 * replays the probing of every set (graph_replay_order), the device numbers the nodes and sends them in that order */
static graph_t *graph_from_device(job_t *J, uint64_t n, dev_state *Dp)
{
	sdt_ctx *gpu = J->gpu;
	const int nwk = J->nwk, nwv = J->nwv, threads = J->threads;
	uint64_t *keys = (uint64_t *)malloc((n + 1) * (size_t)nwk * 8);
	uint64_t *set_start = (uint64_t *)calloc((size_t)threads + 1, sizeof(uint64_t));
	/* all of it on the device (sort, replay of the probing as rounds of priority insertion, numbering); the two-step form
	 * with the host's replay when a limit of the device form is passed, on request (SDT_HOST_REPLAY), and -- SDT_LAYOUT_CHECK
	 * -- beside it: both orders must then name the same key at every visiting position */
	int on_device = 0;
	uint64_t *check_keys = NULL;
	if (!sdt_test_env("SDT_HOST_REPLAY")) {
		const int rcl = sdt_gpu_layout_on_device(gpu, threads, nwv, graph_init_kmerset_size != 0, set_start, &n);
		if (rcl == SDT_OK) on_device = 1;
		else if (rcl == SDT_ELIMIT) { if (!g_quiet) fprintf(stderr, "[sdt-pregraph] %s: the host replays the layout\n", sdt_gpu_last_error()); }
		else if (rcl != SDT_EINVAL) { pg_fail("sdt_gpu_layout_on_device"); return NULL; }
		if (on_device) phase("layout: sort + replay + numbering (GPU)");
	}
	if (!on_device || sdt_test_env("SDT_LAYOUT_CHECK")) {
		uint64_t *hk = on_device ? (uint64_t *)malloc((n + 1) * (size_t)nwk * 8) : keys;
		uint64_t *ss = on_device ? (uint64_t *)calloc((size_t)threads + 1, sizeof(uint64_t)) : set_start;
		if (SDT_CALL(sdt_gpu_layout_sorted_keys, gpu, threads, nwv, hk, n, ss, &n)) return NULL;
		phase("layout: sort (GPU) + keys D2H");
		uint64_t *order = (uint64_t *)malloc((n + 1) * 8);
		graph_replay_order(nwv, nwk, threads, hk, ss, order);
		phase("layout: replay (host)");
		if (on_device) {
			check_keys = (uint64_t *)malloc((n + 1) * (size_t)nwk * 8);
			for (uint64_t vv = 0; vv < n; vv++) memcpy(check_keys + vv * nwk, hk + order[vv] * nwk, (size_t)nwk * 8);
			free(hk); free(ss);
		} else if (SDT_CALL(sdt_gpu_layout_apply, gpu, order, n)) return NULL;
		free(order);
	}
	uint32_t *ll = (uint32_t *)malloc((n + 1) * 4), *rf = (uint32_t *)malloc((n + 1) * 4), *cnt = (uint32_t *)malloc((n + 1) * 4);
	if (SDT_CALL(sdt_gpu_export_ordered, gpu, keys, ll, rf, cnt, n)) return NULL;
	phase("layout: export in visiting order (D2H)");
	if (check_keys) {
		if (memcmp(check_keys, keys, n * (size_t)nwk * 8) != 0) { fprintf(stderr, "SDT_LAYOUT_CHECK: the device's visiting order differs from the host replay's\n"); return NULL; }
		fprintf(stderr, "[sdt-pregraph] SDT_LAYOUT_CHECK: device and host replay agree on all %llu visiting positions\n", (unsigned long long)n);
		free(check_keys);
	}
	Dp->gpu = gpu; Dp->indexed = 1; Dp->by_index = 1;
	graph_index_hook = dev_index_hook;
	graph_index_hook_user = Dp;
	graph_index_hook_early = sdt_tuning_env("SDT_INDEX_INLINE") == NULL;      /* (the device numbered the nodes itself) */
	graph_t *G = graph_from_ordered(J->K, nwv, nwk, threads, n, keys, ll, rf, cnt, set_start);
	graph_free_later(keys, ll, rf, cnt);
	free(set_start);
	phase("graph + index");
	return G;
}

/* the node table in the reference's visiting order as the host graph (graph/graph.h), with the device behind its dry runs where
 * there is one: rank 0's gather under --gpus N, then the layout on the device or graph_build's replay of it from exported arrays */
static graph_t *build_graph(job_t *J, uint64_t n, const int64_t *sizes, dev_state *Dp)
{
	node_arrays A = {NULL, NULL, NULL, NULL, NULL};
	graph_t *G;
	Dp->nwk = J->nwk;
	if (J->gpus > 1) {
		n = J->nodes;                                         /* all shards */
		if (gather_shards(J, sizes, &A)) return NULL;
	}
	if (J->device_graph) {
		if (!(G = graph_from_device(J, n, Dp))) return NULL;
	} else {
		if (J->gpus == 1 && (node_arrays_alloc(&A, n, J->nwk) || SDT_CALL(sdt_gpu_export_nodes, J->gpu, A.keys, A.l, A.r, A.c, A.first, n, &n))) return NULL;
		if (J->host_map) { sdt_gpu_destroy(J->gpu); J->gpu = NULL; }
		phase("export nodes (D2H)");
		Dp->gpu = J->gpu;
		if (J->gpu && !J->host_walks) {
			graph_index_hook = dev_index_hook;
			graph_index_hook_user = Dp;
		}
		G = graph_build(J->K, J->nwv, J->nwk, J->threads, n, A.keys, A.l, A.r, A.c, A.first);
		graph_free_later(A.keys, A.first, A.l, A.r);
		free(A.c);
		phase("layout replay + index (host)");
	}
	if (J->gpu && !J->host_walks) {                                    /* dry runs from the device mirror of the graph */
		G->dirty = (uint8_t *)calloc(G->n + 1, 1);
		G->dev_walks = dev_walks_hook;
		G->dev_minor_out = dev_minor_out_hook;
		if (Dp->by_index) { G->dev_minor_out_commit_begin = dev_minor_out_commit_begin_hook; G->dev_minor_out_commit_finish = dev_minor_out_commit_finish_hook; }
		G->dev_edge_ports = dev_edge_ports_hook;
		if (Dp->by_index && !sdt_test_env("SDT_HOST_EDGES")) G->dev_build_edges = dev_build_edges_hook;
		G->dev_user = Dp;
	}
	return G;
}

/* the three cleaning passes and kmer2edges in call_pregraph's order; returns the number of edges */
static uint64_t clean_and_build_edges(job_t *J, graph_t *G)
{
	time_t t0 = time(NULL);
	graph_remove_minor_out(G, J->dd);                                  /* pregraph.c:68-71 */
	phase(G->dev_minor_out ? "removeMinorOut (GPU dry run + host commit)" : "removeMinorOut (host)");
	printf("time spent on cut kmer: %ds\n\n", (int)(time(NULL) - t0));
	t0 = time(NULL);
	if (!J->d) graph_remove_single_tips(G);                            /* pregraph.c:75-88 */
	graph_remove_minor_tips(G);
	phase(G->dev_walks ? "tip cutting (GPU walks + host commit)" : "tip cutting (host)");
	printf("time spent on cutTipe: %ds\n\n", (int)(time(NULL) - t0));
	t0 = time(NULL);
	const uint64_t ne = graph_build_edges(G, J->prefix);               /* pregraph.c:95-98 */
	phase(G->dev_edge_ports ? "kmer2edges (GPU walks + host ids, stamping)" : "kmer2edges (host)");
	printf("time spent on making edges: %ds\n\n", (int)(time(NULL) - t0));
	return ne;
}

/* the second read pass on the host (--host-map): the files are read again */
static int read2edge_host(job_t *J, graph_t *G)
{
	arc_state as = {G, arcs_new(), 0};
	if (sdt_stream_reads(&J->cfg, J->max_read_len, J->threads, J->chunk, 1, arc_batch, &as, NULL) != 0) return 1;
	printf("%llu reads processed\n", as.reads);
	arcs_write(as.A, J->prefix);
	arcs_free(as.A);
	return 0;
}

/* the second read pass on the GPU over the reads kept in HBM: send the cleaned graph back as path words, map, fetch the arcs; with
 * --gpus N and the pass on every rank, rank 0 publishes the graph and adds the other ranks' arcs to its own */
static int read2edge_device(job_t *J, graph_t *G, const dev_state *Dp, vx_job *vx)
{
	sdt_ctx *gpu = J->gpu;
	const int nwk = J->nwk;
	/* with the device mirror in place the path words go over by node index; otherwise with their keys */
	const int by_index = G->dev_walks != NULL && Dp->indexed;
	/* the edges were built on the device: the path words are there already */
	uint64_t *pk = NULL, *pw = NULL;
	if (!G->edges_on_device) {
		pk = by_index ? NULL : (uint64_t *)malloc((G->n + 1) * (size_t)nwk * 8);
		pw = (uint64_t *)malloc((G->n + 1) * 8);
		void *pa[4] = {G, pk, pw, (void *)(intptr_t)nwk};
		par_for(0, G->n, 1 << 16, gather_paths, pa);
	}
	uint64_t np = 0;
	uint64_t *qk = (uint64_t *)malloc((G->patch_n + 1) * (size_t)nwk * 8), *qi = (uint64_t *)malloc((G->patch_n + 1) * 8);
	for (uint64_t i = 0; G->patch && i <= G->patch_mask; i++)
		if (G->patch[i].used) {
			for (int w = 0; w < nwk; w++) qk[np * nwk + w] = G->patch[i].seq.w[4 - nwk + w];
			qi[np++] = (uint64_t)G->patch[i].edge | ((uint64_t)G->patch[i].twin << 32);
		}
	/* with the edges (and the path words) made on the device the host graph has one duty left, *.vertex: write it now and
	 * let go of the node array while the device maps the reads (its line is printed in its turn) */
	if (G->edges_on_device) {
		graph_vertex_quiet = 1;
		vx->G = G; vx->prefix = J->prefix;
		vx->have = pthread_create(&vx->th, NULL, vertex_thread, vx) == 0;
		if (!vx->have) graph_vertex_quiet = 0;                    /* (no thread: *.vertex is written in its turn, with its line) */
	}
	uint64_t nreads2 = 0, narcs = 0;
	const double t_r0 = now_ms();
	if (SDT_CALL(sdt_gpu_load_paths, gpu, pk, pw, G->n, qk, qi, np, G->num_ed)) return 1;
	pg_paths shared;
	shared.seg.base = NULL;
	if (J->per_rank_map) {
		/* every rank maps its own reads: the graph as that pass needs it goes into shared memory */
		if (pg_paths_publish(J->boot, gpu, nwk, qk, qi, np, G->num_ed, &shared)) return 1;
		phase("path table -> shared memory");
	}
	const double t_r1 = now_ms();
	if (SDT_CALL(sdt_gpu_map_reads, gpu, &nreads2, &narcs)) return 1;
	const double t_r2 = now_ms();
	free(pk); free(pw); free(qk); free(qi);
	pg_arcs a;
	void *blk = malloc(pg_arcs_bytes(narcs));
	if (!blk) { fprintf(stderr, "out of host memory for %llu arcs\n", (unsigned long long)narcs); return 1; }
	pg_arcs_carve(&a, blk, narcs);
	if (SDT_CALL(sdt_gpu_export_arcs, gpu, a.from, a.to, a.mult, a.ord, narcs, &narcs)) return 1;
	if (J->per_rank_map) {
		/* the arcs of the other ranks: same (from, to) pairs add up, the first occurrence is the earliest (prlRead2path.c:415-430
		 * counts per thread and adds up the same way) */
		if (pg_arcs_collect(J->boot, J->gpus, &a, &narcs, &nreads2)) return 1;
		pg_seg_close(&shared.seg, 1);
		narcs = arcs_combine(a.from, a.to, a.mult, a.ord, narcs);
	}
	const double t_r3 = now_ms();
	printf("%llu reads processed\n", (unsigned long long)nreads2);
	arcs_write_arrays(J->prefix, a.from, a.to, a.mult, a.ord, narcs);
	if (sdt_env("SDT_TIMING") && !g_quiet)
		fprintf(stderr, "[read2edge] gather %.1f ms, load paths + patch table %.1f ms, map reads %.1f ms, export %llu arcs %.1f ms, sort + write %.1f ms\n",
		        t_r0 - g_t_last, t_r1 - t_r0, t_r2 - t_r1, (unsigned long long)narcs, t_r3 - t_r2, now_ms() - t_r3);
	free(a.seg.base);
	return 0;
}

/* *.vertex (unless it was written beside the second pass) and preGraphBasic */
static void write_vertex_and_basic(job_t *J, graph_t *G, uint64_t ne, vx_job *vx)
{
	uint64_t nv;
	graph_edges_join(G);                                                /* (*.edge.gz was written beside the second read pass) */
	if (vx->have) {
		pthread_join(vx->th, NULL);
		nv = vx->nv;
		printf("%llu vertex outputed\n", (unsigned long long)nv);
	} else nv = graph_write_vertex(G, J->prefix);                        /* pregraph.c:106 */
	graph_write_basic(J->prefix, nv, J->K, ne, J->max_read_len);
	phase("vertex + preGraphBasic");              /* G is not freed: the process ends here and the kernel is faster at it */
}

int main(int argc, char **argv)
{
	static job_t J;
	static dev_state D;
	push_state st;
	int rc = parse_options(&J, argc, argv);
	if (rc) return rc;
	decide_route(&J);
	timing_preamble(&J);
	if (sdt_cfg_load(J.cfgfile, &J.cfg) != 0) return 255;
	J.max_read_len = J.cfg.max_rd_len ? J.cfg.max_rd_len : 100;              /* prlHashReads.c:361-364 */
	printf("In %s, %d libs, max seq len %d, max name len %d\n\n", J.cfgfile, J.cfg.nlibs, J.max_read_len, 256);

	/* --gpus N: one process per GPU, forked BEFORE anything touches the HIP runtime.  Rank 0 is this process: it prints,
	 * writes the files and runs the graph phases; the others count their share of the reads and hand their nodes over. */
	if (J.gpus < 1 || J.gpus > PG_MAX_RANKS) { fprintf(stderr, "--gpus must be 1..%d\n", PG_MAX_RANKS); return 255; }
	if ((J.rank = pg_ranks_start(J.gpus, &J.boot)) < 0) return 1;
	g_quiet = J.rank > 0;
	parser_threads(&J);
	if (open_device(&J) || pass1(&J, &st)) return 1;
	if ((rc = count_and_freq(&J, st.reads)) != 0) return rc;
	if (!J.hash_only) {
		/* hand the node table to the host graph phases in the reference's visiting order (graph/graph.h) */
		uint64_t n = 0;
		int64_t sizes[PG_MAX_RANKS];
		vx_job vx;
		J.nwk = sdt_gpu_key_words(J.gpu);
		J.nwv = J.max_k <= 31 ? 1 : (J.max_k <= 63 ? 2 : 4);
		if (SDT_CALL(sdt_gpu_export_nodes, J.gpu, NULL, NULL, NULL, NULL, NULL, 0, &n)) return 1;
		if (wide_node_index(&J, J.gpus > 1 ? J.nodes : n)) return 1;
		if (J.gpus > 1) {
			/* shards -> rank 0.  Every rank learns all shard sizes; ranks > 0 export into a shared-memory segment each and
			 * leave once rank 0 has taken their nodes (its own device table: sdt_gpu_import_nodes, or host arrays as well) */
			memset(sizes, 0, sizeof sizes);
			sizes[J.rank] = (int64_t)J.my_nodes;
			if (SDT_CALL(sdt_gpu_allreduce_i64, J.gpu, sizes, J.gpus)) return 1;
			if (J.rank > 0) return rank_after_pass1(&J);
		}
		graph_t *G = build_graph(&J, n, sizes, &D);
		if (!G) return 1;
		const uint64_t ne = clean_and_build_edges(&J, G);
		const time_t t0 = time(NULL);
		printf("%d thread created prlRead2path\n", J.threads);             /* pregraph.c:101-104 */
		memset(&vx, 0, sizeof vx);
		if (J.host_map ? read2edge_host(&J, G) : read2edge_device(&J, G, &D, &vx)) return 1;
		phase(J.host_map ? "read2edge (host)" : "read2edge (GPU)");
		printf("time spent on mapping reads: %ds\n\n", (int)(time(NULL) - t0));
		write_vertex_and_basic(&J, G, ne, &vx);
	}
	if (J.gpu) sdt_gpu_destroy(J.gpu);
	phase("release the device");
	if (sdt_env("SDT_TIMING") && !g_quiet) fprintf(stderr, "[sdt-pregraph] %-28s %9.1f ms\n", "total inside main", now_ms() - g_t_main);
	sdt_cfg_free(&J.cfg);
	if (J.gpus == 1 && !sdt_env("SDT_SLOW_EXIT")) {
		/* every file is closed and the device is released: skip the runtime's and the allocator's own teardown (atexit handlers,
		 * unloading code objects, returning gigabytes page by page) -- the kernel takes the address space back in one go */
		fflush(stdout);
		fflush(stderr);
		_exit(0);
	}
	if (J.gpus > 1 && J.rank == 0) pg_ranks_wait();                 /* the ranks that are still leaving */
	return 0;
}
