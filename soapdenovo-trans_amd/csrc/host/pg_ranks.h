/* pg_ranks.h -- the ranks of one `sdt-pregraph --gpus N` job: the fork, what the ranks tell each other through shared memory, the
 * three segment formats, and the one failure statement of the host program */
#ifndef SDT_PG_RANKS_H
#define SDT_PG_RANKS_H
#include <stddef.h>
#include <stdint.h>
#include "../../../include/sdt_gpu.h"

#define PG_MAX_RANKS 64

/* "call the ABI, on failure print and leave": 0 when the entry point returned SDT_OK; otherwise 1, after `<entry point>: <error>` has
 * gone to stderr (with `[rank r] ` in front on the ranks above 0) */
extern int pg_rank;
int pg_fail(const char *entry);
#define SDT_CALL(fn, ...) (fn(__VA_ARGS__) == SDT_OK ? 0 : pg_fail(#fn))

/* what the ranks share from the fork on */
typedef struct {
	volatile int ready; sdt_comm_id id; char name[64];
	/* second read pass on every rank (round 5): rank 0 publishes the graph (key -> path word, patch table) in shared memory and says
	 * so here; every rank maps ITS reads and leaves its arcs in a segment of its own */
	volatile int paths_state;                  /* 0 not yet, 1 published, 2 rank 0 has all arcs (the ranks may go) */
	volatile unsigned long long paths_n, patch_n, num_ed;
	volatile int arcs_state[PG_MAX_RANKS];     /* 1: this rank's arcs are in its segment, -1: it failed */
	volatile unsigned long long arcs_n[PG_MAX_RANKS], arcs_reads[PG_MAX_RANKS];
} pg_boot;

/* One process per GPU, forked BEFORE anything touches the HIP runtime.  Returns this process's rank (0: the caller itself, which prints,
 * writes the files and runs the graph phases) with pg_rank set, or -1 when the ranks could not be started.  gpus == 1: no fork, *boot
 * stays NULL.  Rank 0 takes the ranks that are still alive, and every segment of the job, with it on every way out. */
int pg_ranks_start(int gpus, pg_boot **boot);
/* rank 0, at the end: the ranks that are still leaving */
void pg_ranks_wait(void);

/* The segments `/sdt_<job>_n<r>`, `/sdt_<job>_a<r>` and `/sdt_<job>_paths`.  One view each: *_bytes is the size of the segment, *_carve
 * lays the typed pointers over a block of that size (writer and readers alike), *_map opens (create: makes) the segment and carves it
 * -- 0, or 1 when there is no such shared memory.  Every array has one entry more than it holds.  (The arcs' pair is public: rank 0
 * keeps its own arcs in a malloc'ed block of the same layout.) */
typedef struct { void *base; size_t bytes; char path[96]; } pg_seg;                               /* a mapped segment (base NULL: none) */
typedef struct { pg_seg seg; uint64_t *keys, *first; uint32_t *l, *r, *c; } pg_nodes;          /* a rank's shard of the node table */
typedef struct { pg_seg seg; uint64_t *pk, *pw, *qk, *qi; } pg_paths;                         /* rank 0's graph for the second pass */
typedef struct { pg_seg seg; uint64_t *ord; uint32_t *from, *to, *mult; } pg_arcs;            /* a rank's arcs */

int pg_nodes_map(pg_nodes *v, int rank, uint64_t n, int nwk, int create);
int pg_paths_map(pg_paths *v, uint64_t pn, uint64_t qn, int nwk, int create);
size_t pg_arcs_bytes(uint64_t n);
void pg_arcs_carve(pg_arcs *v, void *base, uint64_t n);
int pg_arcs_map(pg_arcs *v, int rank, uint64_t n, int create);
/* unmap a view's segment (nothing where none is mapped); unlink_it: its name goes as well */
void pg_seg_close(pg_seg *s, int unlink_it);

/* rank 0: the path table of the device (sdt_gpu_export_paths) and the patch table into the paths segment, then the ranks are told */
int pg_paths_publish(pg_boot *boot, sdt_ctx *gpu, int nwk, const uint64_t *qk, const uint64_t *qi, uint64_t np, uint64_t num_ed, pg_paths *seg);
/* rank 0: waits for the arcs of every other rank and puts them behind its own *narcs arcs (`a`: a carved malloc block, replaced by a
 * larger one); *narcs and *nreads grow by what the ranks had; then the ranks may go */
int pg_arcs_collect(pg_boot *boot, int gpus, pg_arcs *a, uint64_t *narcs, uint64_t *nreads);
#endif
