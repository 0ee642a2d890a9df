/* readwalk_host_check.c -- the device-free walk over the kept reads that every read stage of `sdt-kmers` shares (csrc/host/readwalk.c)
 * on hand-made kept batches: the record lines and the two FASTA files of a stage whose records keep a range and of one that keeps all
 * or nothing, the refusals (an ordinal without a read, an impossible record), a FASTA record across the 1 MiB block boundary, and a
 * file that cannot be written (/dev/full).
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
 *       -o readwalk_host_check tools/readwalk_host_check.c soapdenovo-trans_amd/csrc/host/readwalk.c \
 *       soapdenovo-trans_amd/csrc/host/trimsplit.c soapdenovo-trans_amd/csrc/host/normsplit.c && ./readwalk_host_check [a directory to write in] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "../soapdenovo-trans_amd/csrc/host/readwalk.h"
#include "../soapdenovo-trans_amd/csrc/host/putdec.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* a stage of the check's own: a record is start, len and a verdict; verdict 9 is impossible */
typedef struct { uint32_t start, len, verdict; } rec;
typedef struct { const rec *r; int by_verdict; uint64_t noted; } state;

static int note(void *st, uint64_t ord, uint64_t read_len, uint64_t *start, uint64_t *len)
{
	state *s = (state *)st;
	const rec *r = s->r + ord;
	if (r->verdict == 9 || (!s->by_verdict && (uint64_t)r->start + r->len > read_len)) {
		fprintf(stderr, "readwalk_host_check: the record of read %llu is %u %u %u\n", (unsigned long long)ord + 1, r->start, r->len, r->verdict);
		return -1;
	}
	s->noted++;
	if (!s->by_verdict) { *start = r->start; *len = r->len; }
	return 0;
}

static char *put_line(const void *st, char *p, uint64_t ord)
{
	const rec *r = ((const state *)st)->r + ord;
	p = sdt_put_dec(p, r->start, ' ');
	p = sdt_put_dec(p, r->len, ' ');
	return sdt_put_dec(p, r->verdict, '\n');
}

static int alive(const void *st, uint64_t ord)
{
	const state *s = (const state *)st;
	return s->by_verdict ? s->r[ord].verdict == 0 : s->r[ord].len != 0;
}

static const sdt_walk_stage by_range = {{".lines", ".pairs", ".single"}, 3 * 11, 0, note, put_line, alive, NULL, NULL};
static const sdt_walk_stage by_verdict = {{".lines", ".pairs", ".single"}, 3 * 11, 1, note, put_line, alive, NULL, NULL};

/* n reads of the letters given as one batch: malloc'ed words and offsets as kept_add takes them (A0 C1 T2 G3) */
static void make_batch(const char *const *reads, uint64_t n, uint32_t **words, uint64_t **offsets)
{
	uint64_t bases = 0;
	for (uint64_t i = 0; i < n; i++) bases += strlen(reads[i]);
	*words = (uint32_t *)calloc(bases / 16 + 1, sizeof(uint32_t));
	*offsets = (uint64_t *)calloc(n + 1, sizeof(uint64_t));
	if (!*words || !*offsets) { fprintf(stderr, "readwalk_host_check: out of memory\n"); exit(1); }
	uint64_t g = 0;
	for (uint64_t i = 0; i < n; i++) {
		for (const char *c = reads[i]; *c; c++, g++) (*words)[g >> 4] |= (uint32_t)((*c & 6) >> 1) << (30 - 2 * (int)(g & 15));
		(*offsets)[i + 1] = g;
	}
}

/* The stream of the first cases: ordinals 0..2 single reads (one batch, stride 1), [3, 9) three pairs of a pair of files (two batches,
 * stride 2: the range starts at an odd ordinal).  reads: how many ordinals the stream is said to have. */
static void make_stream(kept_reads *k, sdt_pair_ranges *pr, uint64_t reads)
{
	static const char *const singles[3] = {"ACGTACGTAC", "GGGGG", "TTACGCATT"};
	static const char *const first[3] = {"ACACACAC", "CCCCCCCCCCCCCCCCCA", "GATTACA"};          /* ordinals 3, 5, 7 */
	static const char *const second[3] = {"TGTGTGTG", "AAAAAAAAAAAAAAAAAC", "TGTAATC"};         /* ordinals 4, 6, 8 */
	uint32_t *w;
	uint64_t *o;
	CHECK(kept_init(k, 3, reads) == 0);
	make_batch(singles, 3, &w, &o);
	CHECK(kept_add(k, 0, w, o, 3, 0, 1) == 0);
	make_batch(first, 3, &w, &o);
	CHECK(kept_add(k, 1, w, o, 3, 3, 2) == 0);
	make_batch(second, 3, &w, &o);
	CHECK(kept_add(k, 2, w, o, 3, 4, 2) == 0);
	CHECK(k->longest == 18);
	memset(pr, 0, sizeof *pr);
	CHECK(sdt_pair_ranges_note(pr, 0, 1, 0, 3) == 0);
	CHECK(sdt_pair_ranges_note(pr, 3, 2, 0, 3) == 0);
	CHECK(sdt_pair_ranges_note(pr, 4, 2, 1, 3) == 0);
	CHECK(pr->n == 1 && pr->v[0] == 3 && pr->v[1] == 9);
}

/* is the file prefix + suffix exactly this text */
static int file_is(const char *prefix, const char *suffix, const char *want, size_t n)
{
	char path[4200];
	snprintf(path, sizeof path, "%s%s", prefix, suffix);
	FILE *f = fopen(path, "rb");
	if (!f) return 0;
	char *got = (char *)malloc(n + 2);
	const size_t m = got ? fread(got, 1, n + 1, f) : 0;
	fclose(f);
	const int same = got && m == n && memcmp(got, want, n) == 0;
	free(got);
	return same;
}
#define FILE_IS(prefix, suffix, text) file_is(prefix, suffix, text, strlen(text))

int main(int argc, char **argv)
{
	char prefix[4100];
	kept_reads k;
	sdt_pair_ranges pr;
	sdt_walk_tally t;
	snprintf(prefix, sizeof prefix, "%s/readwalk_host_check", argc > 1 ? argv[1] : ".");

	/* records that keep a range; mates are routed independently */
	{
		const rec r[9] = {{0, 10, 0}, {0, 0, 3}, {2, 4, 2},
		                  {0, 8, 0}, {1, 7, 2},                              /* both mates survive */
		                  {0, 0, 3}, {0, 18, 0},                             /* the first mate was dropped: the second is an orphan */
		                  {3, 4, 2}, {0, 3, 2}};
		state st = {r, 0, 0};
		make_stream(&k, &pr, 9);
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_range, &st, 7, &t) == 0);
		CHECK(t.kept == 7 && t.bases_in == 90 && t.bases_out == 10 + 4 + 8 + 7 + 18 + 4 + 3 && st.noted == 9);
		CHECK(FILE_IS(prefix, ".lines", "0 10 0\n0 0 3\n2 4 2\n0 8 0\n1 7 2\n0 0 3\n0 18 0\n3 4 2\n0 3 2\n"));
		CHECK(FILE_IS(prefix, ".pairs", ">4\nACACACAC\n>5\nGTGTGTG\n>8\nTACA\n>9\nTGT\n"));
		CHECK(FILE_IS(prefix, ".single", ">1\nACGTACGTAC\n>3\nACGC\n>7\nAAAAAAAAAAAAAAAAAC\n"));
		/* the device counted other reads than the records keep */
		st.noted = 0;
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_range, &st, 8, &t) == 1 && t.kept == 7);
		/* without pair ranges every kept read is a single read */
		CHECK(sdt_walk_reads(&k, NULL, prefix, &by_range, &st, 7, &t) == 0);
		CHECK(FILE_IS(prefix, ".pairs", ""));
		CHECK(FILE_IS(prefix, ".single", ">1\nACGTACGTAC\n>3\nACGC\n>4\nACACACAC\n>5\nGTGTGTG\n>7\nAAAAAAAAAAAAAAAAAC\n>8\nTACA\n>9\nTGT\n"));

		/* an impossible record (read 5 keeps [1, 9) of 8 bases): refused, and nothing past it written */
		rec bad[9];
		memcpy(bad, r, sizeof bad);
		bad[4].len = 8;
		state sb = {bad, 0, 0};
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_range, &sb, 7, &t) == 1 && sb.noted == 4);
		CHECK(FILE_IS(prefix, ".lines", "0 10 0\n0 0 3\n2 4 2\n0 8 0\n"));
		CHECK(FILE_IS(prefix, ".pairs", ">4\nACACACAC\n"));
		CHECK(FILE_IS(prefix, ".single", ">1\nACGTACGTAC\n>3\nACGC\n"));
		kept_free(&k);
		sdt_pair_ranges_free(&pr);
	}

	/* records that keep all or nothing; the mates of a pair are a unit */
	{
		const rec r[9] = {{0, 0, 0}, {0, 0, 1}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 1}, {0, 0, 1}, {0, 0, 0}, {0, 0, 0}};
		state st = {r, 1, 0};
		make_stream(&k, &pr, 9);
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_verdict, &st, 6, &t) == 0);
		CHECK(t.kept == 6 && t.bases_in == 90 && t.bases_out == 10 + 9 + 8 + 8 + 7 + 7);
		CHECK(FILE_IS(prefix, ".lines", "0 0 0\n0 0 1\n0 0 0\n0 0 0\n0 0 0\n0 0 1\n0 0 1\n0 0 0\n0 0 0\n"));
		CHECK(FILE_IS(prefix, ".pairs", ">4\nACACACAC\n>5\nTGTGTGTG\n>8\nGATTACA\n>9\nTGTAATC\n"));
		CHECK(FILE_IS(prefix, ".single", ">1\nACGTACGTAC\n>3\nTTACGCATT\n"));
		kept_free(&k);
		sdt_pair_ranges_free(&pr);

		/* a stream of ten ordinals of which no kept read has the last: refused; an ordinal past the stream: refused */
		const rec r10[10] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
		state s10 = {r10, 1, 0};
		make_stream(&k, &pr, 10);
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_verdict, &s10, 10, &t) == 1 && s10.noted == 9);
		kept_free(&k);
		CHECK(kept_init(&k, 1, 2) == 0);
		static const char *const three[3] = {"ACG", "T", "GG"};
		uint32_t *w;
		uint64_t *o;
		make_batch(three, 3, &w, &o);
		CHECK(kept_add(&k, 0, w, o, 3, 0, 1) == 1);
		kept_free(&k);
		sdt_pair_ranges_free(&pr);
	}

	/* 1 100 pairs of reads of 1 000 bases: the FASTA records of the pairs file fill more than two blocks of 1 MiB, and one of them lies
	 * across the first boundary.  The file is complete and in order. */
	{
		enum { N = 2200, L = 1000 };
		uint32_t *w = (uint32_t *)calloc((size_t)N * L / 16 + 1, sizeof(uint32_t));
		uint64_t *o = (uint64_t *)calloc(N + 1, sizeof(uint64_t));
		rec *r = (rec *)calloc(N, sizeof(rec));
		char *want = (char *)malloc((size_t)N * (L + 8)), *p = want;
		CHECK(w && o && r && want);
		if (!w || !o || !r || !want) return 1;
		int straddles = 0;
		for (uint64_t i = 0; i < N; i++) {
			const size_t before = (size_t)(p - want);
			p += sprintf(p, ">%llu\n", (unsigned long long)i + 1);
			for (uint64_t j = 0; j < L; j++) {
				const uint64_t g = i * L + j;
				const uint32_t code = (uint32_t)((g * 2654435761u >> 7) & 3u);
				w[g >> 4] |= code << (30 - 2 * (int)(g & 15));
				*p++ = "ACTG"[code];
			}
			*p++ = '\n';
			straddles |= before < OB_BLOCK && (size_t)(p - want) > OB_BLOCK;
			o[i + 1] = (i + 1) * L;
			r[i].len = L;
		}
		CHECK(straddles && (size_t)(p - want) > 2 * OB_BLOCK);
		CHECK(kept_init(&k, 1, N) == 0);
		CHECK(kept_add(&k, 0, w, o, N, 0, 1) == 0);
		memset(&pr, 0, sizeof pr);
		CHECK(sdt_pair_ranges_note(&pr, 0, 2, 0, N / 2) == 0);
		state st = {r, 0, 0};
		CHECK(sdt_walk_reads(&k, &pr, prefix, &by_range, &st, N, &t) == 0);
		CHECK(t.kept == N && t.bases_out == (unsigned long long)N * L);
		CHECK(file_is(prefix, ".pairs", want, (size_t)(p - want)));
		CHECK(FILE_IS(prefix, ".single", ""));
		free(want);

		/* the same into a pairs file that cannot be written: the walk says so by name, and stops at the block that failed */
		char full[4200], errpath[4200], said[8400];
		snprintf(full, sizeof full, "%s.full", prefix);
		snprintf(errpath, sizeof errpath, "%s.stderr", prefix);
		const sdt_walk_stage to_full = {{".lines", ".full", ".single"}, 3 * 11, 0, note, put_line, alive, NULL, NULL};
		remove(full);
		CHECK(symlink("/dev/full", full) == 0);
		st.noted = 0;
		fflush(stderr);
		const int keep = dup(2);
		CHECK(keep >= 0 && freopen(errpath, "w", stderr) != NULL);
		const int rc = sdt_walk_reads(&k, &pr, prefix, &to_full, &st, N, &t);
		fflush(stderr);
		CHECK(dup2(keep, 2) == 2);
		close(keep);
		clearerr(stderr);
		CHECK(rc == 1);
		CHECK(st.noted > OB_BLOCK / (L + 8) && st.noted < 2 * OB_BLOCK / L);   /* the first block failed: the second is not filled */
		FILE *fe = fopen(errpath, "r");
		CHECK(fe != NULL);
		const size_t m = fe ? fread(said, 1, sizeof said - 1, fe) : 0;
		if (fe) fclose(fe);
		said[m] = 0;
		char expect[4300];
		snprintf(expect, sizeof expect, "sdt-kmers: write to %s failed\n", full);
		CHECK(strcmp(said, expect) == 0);
		remove(full);
		remove(errpath);
		kept_free(&k);
		sdt_pair_ranges_free(&pr);
		free(r);
	}

	static const char *const suffixes[3] = {".lines", ".pairs", ".single"};
	for (int i = 0; i < 3; i++) {
		char path[4200];
		snprintf(path, sizeof path, "%s%s", prefix, suffixes[i]);
		remove(path);
	}
	if (failures) { fprintf(stderr, "readwalk_host_check: %d checks failed\n", failures); return 1; }
	printf("readwalk_host_check: ok\n");
	return 0;
}
