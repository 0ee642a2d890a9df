/* quality_host_check.c -- the device-free host side of `sdt-kmers qtrim` on synthetic input:
 *   * csrc/host/qualsplit.c: what a read's record line looks like, which records can be those of a read of a given length under given
 *     parameters, the line of the verdict that dropped a read, and the histogram of the kept lengths with its summary line: an empty
 *     histogram, every verdict, every cause, records that are refused and leave the histogram as it was;
 *   * csrc/host/seqio.c with sdt_read_quals on: a tiny FASTQ file whose records are a lower-case read, a read with dropped
 *     characters, a read that is letters for 32 characters and then has a dropped one (the AVX2 path hands over to the scalar one), a
 *     read longer than max_read_len, a record with a short and one with a long quality line, and a record with CRLF line ends; once
 *     as it is and once under reverse_seq.  The bytes that come out are asserted one by one, the bases are those of a run with the
 *     switch off, and a FASTA file has no qualities.
 * Run it with and without SDT_TEST_HOOKS=1 SDT_NO_SIMD=1: the scalar path has to give the same bytes.
 * Stand-alone, meant for a sanitizer build on the CPU:
 *   gcc -O1 -g -std=gnu11 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -o quality_host_check \
 *       tools/quality_host_check.c soapdenovo-trans_amd/csrc/host/qualsplit.c soapdenovo-trans_amd/csrc/host/seqio.c -lpthread && ./quality_host_check */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "../soapdenovo-trans_amd/csrc/host/qualsplit.h"
#include "../soapdenovo-trans_amd/csrc/host/seqio.h"

static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

/* what sdt_len_hist_write writes, in a block of exactly its length */
static char *written(const sdt_len_hist *h)
{
	FILE *f = tmpfile();
	if (!f) return NULL;
	CHECK(sdt_len_hist_write(f, h) == 0);
	const long n = ftell(f);
	rewind(f);
	char *got = (char *)malloc((size_t)n + 1);
	CHECK(fread(got, 1, (size_t)n, f) == (size_t)n);
	got[n] = 0;
	fclose(f);
	return got;
}

static void records_and_histogram(void)
{
	/* the record line: the widest fields fill the promised size exactly */
	char *line = (char *)malloc(SDT_QUAL_LINE_MAX);
	const sdt_read_quality widest = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
	char *end = sdt_put_qual_line(line, &widest);
	CHECK(end - line == SDT_QUAL_LINE_MAX && memcmp(line, "4294967295 4294967295 4294967295 4294967295 4294967295 4294967295\n", (size_t)(end - line)) == 0);
	const sdt_read_quality some = {104, 4, 8021, 3, 104, 2};
	end = sdt_put_qual_line(line, &some);
	CHECK(end - line == 19 && memcmp(line, "104 4 8021 3 104 2\n", 19) == 0);
	const sdt_read_quality none = {0, 0, 0, 0, 0, 3};
	end = sdt_put_qual_line(line, &none);
	CHECK(end - line == 12 && memcmp(line, "0 0 0 0 0 3\n", 12) == 0);
	free(line);

	/* the cause of a drop, line by line, under phred 33, cut 20, low 15, 40 %, 30 000 ppm, 20 bases */
	const sdt_quality_params p = {33, 20, 15, 40, 30000, 20, 0, 0}, off = {33, 20, 0, 100, 0, 0, 0, 0};
	const sdt_read_quality r_short = {19, 0, 316, 0, 0, 3}, r_low = {100, 41, 16000, 0, 0, 3}, r_err = {100, 40, 30001, 0, 0, 3};
	const sdt_read_quality r_all = {19, 19, 1000000, 0, 0, 3}, r_whole = {150, 60, 30000, 0, 150, 0}, r_clip = {100, 40, 30000, 7, 100, 2};
	CHECK(sdt_qual_drop_cause(&r_short, &p) == SDT_QUAL_SHORT && sdt_qual_drop_cause(&r_low, &p) == SDT_QUAL_LOW && sdt_qual_drop_cause(&r_err, &p) == SDT_QUAL_ERRORS);
	CHECK(sdt_qual_drop_cause(&r_all, &p) == SDT_QUAL_SHORT);                          /* the first line that applies */
	CHECK(sdt_qual_drop_cause(&r_whole, &p) == SDT_QUAL_KEPT && sdt_qual_drop_cause(&r_clip, &p) == SDT_QUAL_KEPT);
	/* the filters switched off; an empty segment is short even with min_len 0 */
	CHECK(sdt_qual_drop_cause(&r_low, &off) == SDT_QUAL_KEPT && sdt_qual_drop_cause(&r_err, &off) == SDT_QUAL_KEPT && sdt_qual_drop_cause(&r_short, &off) == SDT_QUAL_KEPT);
	CHECK(sdt_qual_drop_cause(&none, &off) == SDT_QUAL_SHORT);

	/* records that a read of 150 bases can have under p, and records that it cannot */
	const sdt_read_quality fine[] = {{150, 60, 30000, 0, 150, 0}, {100, 40, 30000, 7, 100, 2}, {20, 0, 0, 130, 20, 2}, {19, 0, 316, 0, 0, 3},
	                                 {100, 41, 16000, 0, 0, 3}, {100, 40, 30001, 0, 0, 3}, {0, 0, 0, 0, 0, 3}, {149, 0, 100, 1, 149, 2}, {149, 0, 100, 0, 149, 2}};
	for (size_t i = 0; i < sizeof fine / sizeof fine[0]; i++) CHECK(sdt_qual_record_ok(fine + i, 150, &p) == 1);
	const sdt_read_quality wrong[] = {{150, 60, 30000, 0, 150, 1}, {150, 60, 30000, 0, 150, 4}, {150, 60, 30000, 0, 150, 2}, {151, 0, 0, 0, 151, 0},
	                                  {100, 101, 0, 0, 0, 3}, {100, 0, 1000001, 0, 0, 3}, {0, 0, 5, 0, 0, 3}, {100, 40, 30000, 0, 0, 3}, {100, 41, 16000, 7, 100, 2},
	                                  {19, 0, 316, 0, 19, 2}, {100, 40, 30000, 7, 99, 2}, {100, 40, 30000, 51, 100, 2}, {100, 40, 30000, 7, 100, 0},
	                                  {150, 0, 100, 1, 150, 0}, {19, 0, 316, 3, 0, 3}, {19, 0, 316, 0, 19, 3}, {100, 0, 100, 0, 0, 2}};
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_qual_record_ok(wrong + i, 150, &p) == 0);
	CHECK(sdt_qual_record_ok(&none, 0, &p) == 1 && sdt_qual_record_ok(&none, 0, &off) == 1);
	const sdt_read_quality empty_whole = {0, 0, 0, 0, 0, 0};
	CHECK(sdt_qual_record_ok(&empty_whole, 0, &off) == 0);

	/* an empty histogram: the summary line alone */
	sdt_len_hist *h = (sdt_len_hist *)calloc(1, sizeof(sdt_len_hist));
	char *got = written(h);
	CHECK(got && strcmp(got, "# reads 0 whole 0 clipped 0 dropped 0 short 0 low 0 errors 0 bases_in 0 bases_out 0\n") == 0);
	free(got);
	for (size_t i = 0; i < sizeof fine / sizeof fine[0]; i++) CHECK(sdt_len_hist_note(h, fine + i, 150, &p) == 0);
	CHECK(sdt_len_hist_note(h, &none, 0, &p) == 0);
	const sdt_read_quality longer = {5000, 0, 0, 0, 5000, 0};
	CHECK(sdt_len_hist_note(h, &longer, 5000, &p) == 0);
	CHECK(h->reads == 11 && h->whole == 2 && h->clipped == 4 && h->dropped == 5 && h->n_short == 3 && h->n_low == 1 && h->n_errors == 1);
	CHECK(h->bases_in == 9 * 150 + 5000 && h->bases_out == 150 + 100 + 20 + 149 + 149 + 5000);
	got = written(h);
	CHECK(got && strcmp(got, "20 1\n100 1\n149 2\n150 1\n5000 1\n# reads 11 whole 2 clipped 4 dropped 5 short 3 low 1 errors 1 bases_in 6350 bases_out 5568\n") == 0);
	free(got);
	/* records that no read of that length has: nothing is noted */
	for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) CHECK(sdt_len_hist_note(h, wrong + i, 150, &p) == -2);
	CHECK(sdt_len_hist_note(h, &widest, 150, &p) == -2 && sdt_len_hist_note(h, fine + 0, 149, &p) == -2);
	CHECK(h->reads == 11 && h->bases_in == 6350 && h->by_len[150] == 1);
	sdt_len_hist_free(h);
	CHECK(h->by_len == NULL && h->cap == 0);
	free(h);
}

/* ---- seqio.c ---- */
enum { NREC = 7, MAX_READ_LEN = 40 };
static const char *const FASTQ =
	"@lower\nacgtnACGTNacgtac\n+\nIIIIHHHHGGFFEEDD\n"
	"@dropped\nACGT-ACGT*ACGTAC.GT\n+\n0123456789abcdefghi\n"
	"@handover\nACGTACGTACGTACGTACGTACGTACGTACGTAC-GT\n+\nABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijk\n"
	"@long\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmn\n"
	"@shortqual\nACGTACGTAC\n+\nIIIIII\n"
	"@longqual\nACGTACGTAC\n+\n0123456789ABC\n"
	"@crlf\r\nACGTACGTAC\r\n+\r\nIIIIIHHHHH\r\n";
/* the quality bytes per read as the lines have them; '~' stands for the byte 0 that fills a short quality line */
static const char *const WANT[NREC] = {"IIIIHHHHGGFFEEDD", "01235678abcdefghi", "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghjk", "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcd",
                                       "IIIIII~~~~", "0123456789", "IIIIIHHHHH"};

typedef struct {
	uint64_t nreads, nbases, faults, nwords;
	uint64_t offs[NREC + 1];
	uint8_t quals[512];
	uint32_t words[64];
	int has_quals, calls;
} seen_t;

static int collect(void *user, const sdt_batch *b)
{
	seen_t *s = (seen_t *)user;
	s->calls++;
	s->nreads = b->nreads;
	s->faults = b->qual_faults;
	s->has_quals = b->quals != NULL;
	if (b->nreads > NREC) return -1;
	memcpy(s->offs, b->offsets, (b->nreads + 1) * sizeof(uint64_t));
	s->nbases = b->offsets[b->nreads];
	if (s->nbases > sizeof s->quals || b->nwords > 64) return -1;
	if (b->quals) memcpy(s->quals, b->quals, s->nbases);       /* exactly the bytes of the reads: the sanitizer sees a short buffer */
	s->nwords = b->nwords;
	memcpy(s->words, b->words, b->nwords * sizeof(uint32_t));
	return 0;
}

static void parser(void)
{
	char path[] = "/tmp/quality_host_check_XXXXXX";
	const int fd = mkstemp(path);
	CHECK(fd >= 0);
	if (fd < 0) return;
	CHECK(write(fd, FASTQ, strlen(FASTQ)) == (ssize_t)strlen(FASTQ));
	close(fd);
	seen_t *off = (seen_t *)calloc(1, sizeof(seen_t)), *on = (seen_t *)calloc(1, sizeof(seen_t));
	for (int reverse = 0; reverse < 2; reverse++) {
		uint64_t n = 0;
		memset(off, 0, sizeof *off);
		memset(on, 0, sizeof *on);
		/* the switch off (the default): no qualities, no faults */
		CHECK(sdt_read_file(path, 'q', MAX_READ_LEN, reverse, 2, 1 << 20, collect, off, &n) == 0 && n == NREC);
		CHECK(off->calls == 1 && off->nreads == NREC && !off->has_quals && off->faults == 0);
		sdt_read_quals(1);
		CHECK(sdt_read_file(path, 'q', MAX_READ_LEN, reverse, 2, 1 << 20, collect, on, &n) == 0 && n == NREC);
		sdt_read_quals(0);
		CHECK(on->calls == 1 && on->nreads == NREC && on->has_quals && on->faults == 2);
		/* the bases are what they were */
		CHECK(on->nwords == off->nwords && memcmp(on->words, off->words, on->nwords * sizeof(uint32_t)) == 0);
		CHECK(memcmp(on->offs, off->offs, sizeof on->offs) == 0);
		for (int r = 0; r < NREC; r++) {
			const size_t len = strlen(WANT[r]);
			CHECK(on->offs[r + 1] - on->offs[r] == len);
			if (on->offs[r + 1] - on->offs[r] != len) continue;
			for (size_t i = 0; i < len; i++) {
				const char w = WANT[r][reverse ? len - 1 - i : i];
				const uint8_t want = w == '~' ? 0 : (uint8_t)w, got = on->quals[on->offs[r] + i];
				if (got != want) { fprintf(stderr, "reverse %d read %d base %zu: byte %u, %u expected\n", reverse, r, i, got, want); failures++; }
			}
		}
	}
	unlink(path);
	/* a FASTA file has no qualities, switch or not */
	char fpath[] = "/tmp/quality_host_check_XXXXXX";
	const int ffd = mkstemp(fpath);
	CHECK(ffd >= 0);
	if (ffd >= 0) {
		const char *fa = ">a\nACGTACGTAC\n>b\nACGT\n";
		CHECK(write(ffd, fa, strlen(fa)) == (ssize_t)strlen(fa));
		close(ffd);
		uint64_t n = 0;
		memset(on, 0, sizeof *on);
		sdt_read_quals(1);
		CHECK(sdt_read_file(fpath, 'a', MAX_READ_LEN, 0, 1, 1 << 20, collect, on, &n) == 0 && n == 2);
		sdt_read_quals(0);
		CHECK(on->calls == 1 && on->nreads == 2 && !on->has_quals && on->faults == 0 && on->nbases == 14);
		unlink(fpath);
	}
	free(off);
	free(on);
}

int main(void)
{
	records_and_histogram();
	parser();
	if (failures) { fprintf(stderr, "quality_host_check: %d checks failed\n", failures); return 1; }
	printf("quality_host_check: ok\n");
	return 0;
}
