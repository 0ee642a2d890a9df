/* pg_ranks.c -- the ranks of one `sdt-pregraph --gpus N` job and their shared-memory segments (pg_ranks.h) */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <unistd.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>

#include "pg_ranks.h"
#include "graph/par.h"

int pg_rank;

int pg_fail(const char *entry)
{
	if (pg_rank > 0) fprintf(stderr, "[rank %d] ", pg_rank);
	fprintf(stderr, "%s: %s\n", entry, sdt_gpu_last_error());
	return 1;
}

/* Failure propagation between the forked ranks.  RCCL collectives have no timeout: a rank that leaves early would keep its
 * peers blocked for ever, holding their GPUs.  So: every child dies with its parent (PR_SET_PDEATHSIG); rank 0 -- the parent --
 * reaps children in a SIGCHLD handler and, when one of them failed, kills the rest and exits; and whenever rank 0 itself
 * leaves (any `return`, atexit) it takes the children that are still alive with it. */
static volatile pid_t g_child[PG_MAX_RANKS];
static volatile int g_nchild;
static char g_job[64];                      /* the job's name in /dev/shm */

/* the one place that knows what a segment is called: its file under /dev/shm; the name shm_open takes is the part after SHM_DIR */
#define SHM_DIR "/dev/shm"
typedef enum { SEG_NODES, SEG_ARCS, SEG_PATHS } seg_kind;
static void seg_path(char *out, size_t cap, seg_kind kind, int rank)
{
	memcpy(out, SHM_DIR, sizeof SHM_DIR);
	out += sizeof SHM_DIR - 1; cap -= sizeof SHM_DIR - 1;
	if (kind == SEG_PATHS) snprintf(out, cap, "/sdt_%s_paths", g_job);
	else snprintf(out, cap, "/sdt_%s_%c%d", g_job, kind == SEG_NODES ? 'n' : 'a', rank);
}

/* rank 0: every segment the job may make, whoever makes it (a rank killed while polling never unlinks its own), named when the job is:
 * the ways out -- the signal handler among them -- only walk this table (unlink() is async-signal-safe, formatting a name is not);
 * unlinking a name that is not there costs a failed system call */
static char g_seg[2 * PG_MAX_RANKS][sizeof(((pg_seg *)0)->path)];
static volatile int g_nseg;

static void unlink_segments(void)
{
	for (int i = 0; i < g_nseg; i++) unlink(g_seg[i]);
}

static void kill_children(void)
{
	for (int i = 0; i < g_nchild; i++)
		if (g_child[i] > 0) { kill(g_child[i], SIGKILL); (void)waitpid(g_child[i], NULL, 0); g_child[i] = 0; }
	unlink_segments();
}

static void on_sigchld(int sig)
{
	(void)sig;
	int st;
	/* only the ranks recorded in g_child are reaped here (another child of the process is not this handler's business) */
	for (int k = 0; k < g_nchild; k++) {
		const pid_t c = g_child[k];
		if (c <= 0 || waitpid(c, &st, WNOHANG) != c) continue;
		g_child[k] = 0;
		if (!(WIFEXITED(st) && WEXITSTATUS(st) == 0)) {
			static const char msg[] = "sdt-pregraph: a rank failed; stopping the others\n";
			if (write(2, msg, sizeof msg - 1) < 0) { }
			for (int i = 0; i < g_nchild; i++)
				if (g_child[i] > 0) kill(g_child[i], SIGKILL);
			unlink_segments();
			_exit(1);
		}
	}
}

int pg_ranks_start(int gpus, pg_boot **bootp)
{
	*bootp = NULL;
	if (gpus == 1) return 0;
	pg_boot *boot = (pg_boot *)mmap(NULL, sizeof(pg_boot), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
	if (boot == MAP_FAILED) { perror("mmap"); return -1; }
	memset(boot, 0, sizeof *boot);
	snprintf(boot->name, sizeof boot->name, "pg%d", (int)getpid());
	snprintf(g_job, sizeof g_job, "%s", boot->name);
	seg_path(g_seg[0], sizeof g_seg[0], SEG_PATHS, 0);
	for (int r = 1; r < gpus; r++) {
		seg_path(g_seg[2 * r - 1], sizeof g_seg[0], SEG_ARCS, r);
		seg_path(g_seg[2 * r], sizeof g_seg[0], SEG_NODES, r);
	}
	g_nseg = 2 * gpus - 1;
	*bootp = boot;
	fflush(stdout);
	struct sigaction sa;
	memset(&sa, 0, sizeof sa);
	sa.sa_handler = on_sigchld;
	sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
	sigaction(SIGCHLD, &sa, NULL);
	atexit(kill_children);
	const pid_t parent = getpid();
	for (int r = 1; r < gpus; r++) {
		/* SIGCHLD stays blocked from before the fork until the pid is on record: a child that dies at once is then reaped
		 * by the handler like any other (not left as a slot that is waited for at the end and killed by a recycled pid) */
		sigset_t blk, old;
		sigemptyset(&blk);
		sigaddset(&blk, SIGCHLD);
		sigprocmask(SIG_BLOCK, &blk, &old);
		const pid_t pid = fork();
		if (pid < 0) { perror("fork"); return -1; }
		if (pid == 0) {
			pg_rank = r;
			g_nchild = 0;                                         /* (a child has no children to take along) */
			g_nseg = 0;                                           /* (nor the job's segments to clear away) */
			signal(SIGCHLD, SIG_DFL);
			sigprocmask(SIG_SETMASK, &old, NULL);
			prctl(PR_SET_PDEATHSIG, SIGKILL);
			if (getppid() != parent) return -1;                   /* the parent is gone already (also under a subreaper) */
			if (!freopen("/dev/null", "w", stdout)) return -1;     /* one voice: rank 0's */
			return r;
		}
		g_child[g_nchild] = pid;
		g_nchild = g_nchild + 1;
		sigprocmask(SIG_SETMASK, &old, NULL);
	}
	return 0;
}

void pg_ranks_wait(void)
{
	for (int tries = 0; tries < 30000; tries++) {                /* (the handler reaps them) */
		int alive = 0;
		for (int i = 0; i < g_nchild; i++) alive += g_child[i] > 0;
		if (!alive) break;
		usleep(1000);
	}
}

/* first touch of a fresh segment, on all threads: the pages of a new shared-memory object are made (and cleared) by the kernel at the
 * first write, one fault per page on the writing thread -- the device-to-host copy of a 2 GB path table into a fresh segment ran at
 * 3 GB/s (685 ms at 20 M reads with four ranks, profiles/r6) when its four staging threads took those faults one by one */
static void touch_pages(void *vc, uint64_t lo, uint64_t hi, int tid)
{
	(void)tid;
	volatile char *b = (volatile char *)vc;
	for (uint64_t pg = lo; pg < hi; pg++) b[pg << 12] = 0;
}

static void *seg_map(pg_seg *s, seg_kind kind, int rank, size_t bytes, int create)
{
	s->base = NULL;
	s->bytes = bytes;
	seg_path(s->path, sizeof s->path, kind, rank);
	const char *name = s->path + sizeof SHM_DIR - 1;
	int fd = create ? shm_open(name, O_CREAT | O_RDWR, 0600) : shm_open(name, O_RDWR, 0600);
	if (fd < 0) return NULL;
	if (create && ftruncate(fd, (off_t)bytes) != 0) { close(fd); return NULL; }
	void *p = mmap(NULL, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
	close(fd);
	if (p == MAP_FAILED) return NULL;
	if (create && bytes >= ((size_t)64 << 20)) par_for(0, (bytes + 4095) >> 12, 4096, touch_pages, p);
	return p;
}

void pg_seg_close(pg_seg *s, int unlink_it)
{
	if (!s->base) return;
	munmap(s->base, s->bytes);
	s->base = NULL;
	if (unlink_it) shm_unlink(s->path + sizeof SHM_DIR - 1);
}

/* node shard: keys (n+1)*nwk u64, first (n+1) u64, l, r, c (n+1) u32 each */
static size_t pg_nodes_bytes(uint64_t n, int nwk) { return (size_t)(n + 1) * ((size_t)nwk * 8 + 8 + 12); }
static void pg_nodes_carve(pg_nodes *v, void *base, uint64_t n, int nwk)
{
	v->seg.base = base; v->seg.bytes = pg_nodes_bytes(n, nwk);
	v->keys = (uint64_t *)base; v->first = v->keys + (n + 1) * (size_t)nwk;
	v->l = (uint32_t *)(v->first + n + 1); v->r = v->l + n + 1; v->c = v->r + n + 1;
}
int pg_nodes_map(pg_nodes *v, int rank, uint64_t n, int nwk, int create)
{
	void *p = seg_map(&v->seg, SEG_NODES, rank, pg_nodes_bytes(n, nwk), create);
	if (p) pg_nodes_carve(v, p, n, nwk);
	return p == NULL;
}

/* path table: pk (pn+1)*nwk, pw (pn+1), qk (qn+1)*nwk, qi (qn+1), all u64 */
static size_t pg_paths_bytes(uint64_t pn, uint64_t qn, int nwk) { return (size_t)(pn + 1) * ((size_t)nwk * 8 + 8) + (size_t)(qn + 1) * ((size_t)nwk * 8 + 8); }
static void pg_paths_carve(pg_paths *v, void *base, uint64_t pn, uint64_t qn, int nwk)
{
	v->seg.base = base; v->seg.bytes = pg_paths_bytes(pn, qn, nwk);
	v->pk = (uint64_t *)base; v->pw = v->pk + (pn + 1) * (size_t)nwk;
	v->qk = v->pw + pn + 1; v->qi = v->qk + (qn + 1) * (size_t)nwk;
}
int pg_paths_map(pg_paths *v, uint64_t pn, uint64_t qn, int nwk, int create)
{
	void *p = seg_map(&v->seg, SEG_PATHS, 0, pg_paths_bytes(pn, qn, nwk), create);
	if (p) pg_paths_carve(v, p, pn, qn, nwk);
	return p == NULL;
}

/* arc list: ord (n+1) u64, then from, to, mult (n+1) u32 each */
size_t pg_arcs_bytes(uint64_t n) { return (size_t)(n + 1) * 20; }
void pg_arcs_carve(pg_arcs *v, void *base, uint64_t n)
{
	v->seg.base = base; v->seg.bytes = pg_arcs_bytes(n);
	v->ord = (uint64_t *)base;
	v->from = (uint32_t *)(v->ord + n + 1); v->to = v->from + n + 1; v->mult = v->to + n + 1;
}
int pg_arcs_map(pg_arcs *v, int rank, uint64_t n, int create)
{
	void *p = seg_map(&v->seg, SEG_ARCS, rank, pg_arcs_bytes(n), create);
	if (p) pg_arcs_carve(v, p, n);
	return p == NULL;
}

int pg_paths_publish(pg_boot *boot, sdt_ctx *gpu, int nwk, const uint64_t *qk, const uint64_t *qi, uint64_t np, uint64_t num_ed, pg_paths *seg)
{
	uint64_t pn = 0;
	if (SDT_CALL(sdt_gpu_export_paths, gpu, NULL, NULL, 0, &pn)) return 1;
	if (pg_paths_map(seg, pn, np, nwk, 1)) { fprintf(stderr, "shared memory for the path table of %llu nodes failed\n", (unsigned long long)pn); return 1; }
	if (SDT_CALL(sdt_gpu_export_paths, gpu, seg->pk, seg->pw, pn, &pn)) return 1;
	memcpy(seg->qk, qk, np * (size_t)nwk * 8);
	memcpy(seg->qi, qi, np * 8);
	boot->paths_n = pn; boot->patch_n = np; boot->num_ed = num_ed;
	__sync_synchronize();
	boot->paths_state = 1;
	return 0;
}

int pg_arcs_collect(pg_boot *boot, int gpus, pg_arcs *a, uint64_t *narcs, uint64_t *nreads)
{
	uint64_t total = *narcs;
	for (int r = 1; r < gpus; r++) {
		while (boot->arcs_state[r] == 0) usleep(1000);
		if (boot->arcs_state[r] < 0) { fprintf(stderr, "rank %d failed in the second pass\n", r); return 1; }
		total += boot->arcs_n[r];
		*nreads += boot->arcs_reads[r];
	}
	pg_arcs all, mine = *a;
	void *blk = malloc(pg_arcs_bytes(total));
	if (!blk) { fprintf(stderr, "out of host memory for %llu arcs\n", (unsigned long long)total); return 1; }
	pg_arcs_carve(&all, blk, total);
	uint64_t at = 0;
	for (int r = 0; r < gpus; r++) {
		const uint64_t m_n = r ? boot->arcs_n[r] : *narcs;
		if (r && pg_arcs_map(&mine, r, m_n, 0)) { fprintf(stderr, "cannot map the arcs of rank %d\n", r); return 1; }
		memcpy(all.ord + at, mine.ord, m_n * 8); memcpy(all.from + at, mine.from, m_n * 4);
		memcpy(all.to + at, mine.to, m_n * 4); memcpy(all.mult + at, mine.mult, m_n * 4);
		at += m_n;
		if (r) pg_seg_close(&mine.seg, 0);
	}
	__sync_synchronize();
	boot->paths_state = 2;                                /* the other ranks may go */
	free(a->seg.base);
	*a = all;
	*narcs = total;
	return 0;
}
