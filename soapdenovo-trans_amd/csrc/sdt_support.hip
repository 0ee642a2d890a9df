// sdt_support.hip -- read support tallied on the unitig list (the rule: include/sdt_gpu.h).  support_begin = one cleared block of the
// context's own (48 counters, 16 B per unitig, 8 x 8 B per unitig of link slots, the two hash sets); the add forms = k_sp_reads, the walk
// of k_th_reads that counts instead of writing (sdt_support_kernels.cuh); support_links = the records of sdt_gpu_unitigs_links for the
// range and k_sp_links over them; the two lists are read back whole and put in order on the host.  Nothing here writes the table, the
// kept reads, the index or another cache or tally of the context.  The tally belongs to the list: unitigs_free (sdt_unitig.hip) and
// sdt_gpu_destroy free it, a second unitigs_index leaves it, and where the list or the index is stale or gone the calls refuse with the
// messages of sdt_thread.hip.  State rules and staging are those of the read stages (sdt_readstage.hpp).
#include "sdt_readstage.hpp"
#include "sdt_support_kernels.cuh"
#include <algorithm>
#include <cstddef>

static_assert(sizeof(sdt_unitig_support) == sizeof(UnitigSupport) && offsetof(sdt_unitig_support, kmers) == 8, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_link_support) == sizeof(LinkSupport) && offsetof(sdt_link_support, against) == 8, "include/sdt_gpu.h and the kernel agree");
static_assert(sizeof(sdt_unitig_junction) == 24 && offsetof(sdt_unitig_junction, count) == 16, "sdt_unitig_junction is 24 bytes");
static_assert(sizeof(sdt_mate_link) == 16 && offsetof(sdt_mate_link, pairs) == 8, "sdt_mate_link is 16 bytes");
static_assert(SP_DROPPED + 1 == 12, "the totals of include/sdt_gpu.h are twelve words");

constexpr uint64_t SP_MAX_ENTRIES = 1ULL << 36;          // of one set: its slots are the next power of two of twice as many

// the messages of the unitig calls and of the threading calls (sdt_unitig.hip: unitigs_open, sdt_thread.hip: index_open), then its own
static int support_open(const sdt_ctx *c, const char *what)
{
	if (!c->ug.open)
		return fail(SDT_ESTATE, "%s: no unitig list: call sdt_gpu_unitigs_begin first", what);
	if (c->ug.stale || c->ug.slots != c->slots)
		return fail(SDT_ESTATE, "%s: the table changed since sdt_gpu_unitigs_begin", what);
	if (!c->ug.lab)
		return fail(SDT_ESTATE, "%s: no sdt_gpu_unitigs_index of this unitig list", what);
	if (!c->ug.sup)
		return fail(SDT_ESTATE, "%s: no sdt_gpu_unitigs_support_begin of this unitig list", what);
	return SDT_OK;
}

static void support_free(sdt_ctx *c)
{
	if (c->ug.sup) (void)hipFree(c->ug.sup);
	c->ug.sup = nullptr;
	c->ug.sup_jn_slots = c->ug.sup_jn_cap = c->ug.sup_mt_slots = c->ug.sup_mt_cap = 0;
}

static uint64_t set_slots(uint64_t cap)
{
	if (!cap) return 0;
	uint64_t s = 64;
	while (s < 2 * cap) s <<= 1;
	return s;
}

// where the parts of the block lie
static SupportTally tally_of(const sdt_ctx *c)
{
	uint8_t *p = (uint8_t *)c->ug.sup;
	SupportTally t;
	t.ctr = (unsigned long long *)p;
	t.us = (UnitigSupport *)(p + SP_COUNTERS * sizeof(unsigned long long));
	t.along = (unsigned long long *)(t.us + c->ug.n);
	t.jn = (JunctionEnt *)(t.along + 8 * c->ug.n);
	t.mt = (MateEnt *)(t.jn + c->ug.sup_jn_slots);
	t.jn_mask = c->ug.sup_jn_slots - 1;
	t.jn_cap = c->ug.sup_jn_cap;
	t.mt_mask = c->ug.sup_mt_slots - 1;
	t.mt_cap = c->ug.sup_mt_cap;
	if (!c->ug.sup_jn_slots) t.jn = nullptr;
	if (!c->ug.sup_mt_slots) t.mt = nullptr;
	return t;
}

static uint64_t block_bytes(uint64_t n, uint64_t jn_slots, uint64_t mt_slots)
{
	return SP_COUNTERS * sizeof(unsigned long long) + n * (sizeof(UnitigSupport) + 8 * sizeof(unsigned long long)) + jn_slots * sizeof(JunctionEnt) +
	       mt_slots * sizeof(MateEnt);
}

static int add_args_ok(uint64_t nreads, int paired)
{
	if (paired && (nreads & 1))
		return fail(SDT_EINVAL, "paired reads: reads 2t and 2t + 1 are mates, %llu reads is an odd number", (unsigned long long)nreads);
	return SDT_OK;
}

// one dense device-resident batch, checked arguments; enqueued only
static int add_batch(sdt_ctx *c, const uint32_t *d_words, const uint64_t *d_offs, uint64_t nreads, int paired)
{
	const int per = paired ? 2 : 1;
	const uint64_t items = nreads / (uint64_t)per;
	const int g = wave_grid(c, items);
	const uint32_t min_link = c->ug.min_link;
	const SupportTally t = tally_of(c);
	EventPair *ev = next_event(c);
	if (ev) HIPCHK(hipEventRecord(ev->a, c->stream));
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_sp_reads<NW>, dim3(g), dim3(TPB), 0, c->stream, d_words, d_offs, items, per, c->K, min_link, table_of<NW>(c), (const uint2 *)c->ug.lab, t);
	});
	HIPCHK(hipGetLastError());
	if (ev) {
		HIPCHK(hipEventRecord(ev->b, c->stream));
		ev->kmers = nreads;                                  // (reads, not k-mers: their lengths are on the device only)
	}
	return SDT_OK;
}

// the counters, read back; waits
static int counters(sdt_ctx *c, unsigned long long h[SP_COUNTERS])
{
	HIPCHK(hipMemcpyAsync(h, c->ug.sup, SP_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

static bool junctions_full(const sdt_ctx *c, const unsigned long long *h) { return h[SP_JUNCTIONS_DROPPED] || h[SP_N_JUNCTIONS] > c->ug.sup_jn_cap; }
static bool mates_full(const sdt_ctx *c, const unsigned long long *h) { return h[SP_MATES_DROPPED] || h[SP_N_MATES] > c->ug.sup_mt_cap; }

// waits for the adds, and says whether a set has filled up
static int add_finish(sdt_ctx *c)
{
	unsigned long long h[SP_COUNTERS];
	const int rc = counters(c, h);
	if (rc != SDT_OK) return rc;
	const bool jf = c->ug.sup_jn_slots && junctions_full(c, h), mf = c->ug.sup_mt_slots && mates_full(c, h);
	if (jf || mf)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_add: the %s set is full (%llu junctions for a capacity of %llu, %llu mate links for %llu; %llu entries dropped): "
		            "its list is lost, the tallies per unitig and per link are exact", jf ? (mf ? "junction and the mate-link" : "junction") : "mate-link", h[SP_N_JUNCTIONS],
		            (unsigned long long)c->ug.sup_jn_cap, h[SP_N_MATES], (unsigned long long)c->ug.sup_mt_cap, h[SP_JUNCTIONS_DROPPED] + h[SP_MATES_DROPPED]);
	return SDT_OK;
}

static int range_ok(const sdt_ctx *c, const char *what, uint64_t first, uint64_t n)
{
	if (first > c->ug.n || n > c->ug.n - first)
		return fail(SDT_EINVAL, "%s: unitigs %llu .. %llu of %llu", what, (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)c->ug.n);
	return SDT_OK;
}

// the link records of the range on the host (sdt_gpu_unitigs_links, asked for its size first)
static int links_of(sdt_ctx *c, uint64_t first, uint64_t n, std::vector<sdt_unitig_link> &links)
{
	uint64_t total = 0;
	int rc = sdt_gpu_unitigs_links(c, first, n, nullptr, 0, &total, nullptr);
	if (rc != SDT_OK) return rc;
	links.resize((size_t)total);
	if (total) rc = sdt_gpu_unitigs_links(c, first, n, links.data(), total, &total, nullptr);
	return rc;
}

extern "C" {

int sdt_gpu_unitigs_support_begin(sdt_ctx *c, const sdt_support_params *params)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!params)
		return fail(SDT_EINVAL, "sdt_support_params is NULL");
	if (params->flags || params->reserved)
		return fail(SDT_EINVAL, "sdt_support_params.flags = 0x%x, reserved = 0x%x: no flag is defined, reserved is 0", params->flags, params->reserved);
	if (params->junction_capacity > SP_MAX_ENTRIES || params->mate_capacity > SP_MAX_ENTRIES)
		return fail(SDT_EINVAL, "sdt_support_params: junction_capacity = %llu, mate_capacity = %llu: 2^36 at the most each", (unsigned long long)params->junction_capacity,
		            (unsigned long long)params->mate_capacity);
	SDT_ENTER(c);
	int rc = SDT_OK;
	if (!c->ug.open) rc = fail(SDT_ESTATE, "sdt_gpu_unitigs_support_begin: no unitig list: call sdt_gpu_unitigs_begin first");
	else if (c->ug.stale || c->ug.slots != c->slots) rc = fail(SDT_ESTATE, "sdt_gpu_unitigs_support_begin: the table changed since sdt_gpu_unitigs_begin");
	else if (!c->ug.lab) rc = fail(SDT_ESTATE, "sdt_gpu_unitigs_support_begin: no sdt_gpu_unitigs_index of this unitig list");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_support_begin");
	if (rc != SDT_OK) return rc;
	if (c->ug.n >= 0x7FFFFFFFULL)
		return fail(SDT_ELIMIT, "sdt_gpu_unitigs_support_begin: %llu unitigs: an oriented unitig, id << 1 | o, is 32-bit and all ones is taken", (unsigned long long)c->ug.n);
	HIPCHK(hipStreamSynchronize(c->stream));
	support_free(c);                                         // (a second begin replaces the first)
	const uint64_t jn_slots = set_slots(params->junction_capacity), mt_slots = set_slots(params->mate_capacity);
	const uint64_t bytes = block_bytes(c->ug.n, jn_slots, mt_slots);
	const hipError_t em = hipMalloc(&c->ug.sup, bytes);
	if (em != hipSuccess) {
		c->ug.sup = nullptr;
		return fail(SDT_ENOMEM, "the support tally: %llu bytes (80 per unitig, %llu junction slots of 24, %llu mate-link slots of 16): %s", (unsigned long long)bytes,
		            (unsigned long long)jn_slots, (unsigned long long)mt_slots, hipGetErrorString(em));
	}
	c->ug.sup_jn_slots = jn_slots;
	c->ug.sup_jn_cap = params->junction_capacity;
	c->ug.sup_mt_slots = mt_slots;
	c->ug.sup_mt_cap = params->mate_capacity;
	const hipError_t e = hipMemsetAsync(c->ug.sup, 0, bytes, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);
	if (e != hipSuccess || e2 != hipSuccess) support_free(c);
	HIPCHK(e);
	HIPCHK(e2);
	return SDT_OK;
}

int sdt_gpu_unitigs_support_add_device(sdt_ctx *c, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!d_packed_words || !d_offsets)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = add_args_ok(nreads, paired);
	if (rc == SDT_OK) rc = support_open(c, "sdt_gpu_unitigs_support_add");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_support_add");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	rc = add_batch(c, (const uint32_t *)d_packed_words, (const uint64_t *)d_offsets, nreads, paired);
	if (rc != SDT_OK) return rc;
	return add_finish(c);
}

int sdt_gpu_unitigs_support_add(sdt_ctx *c, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (nreads == 0)
		return SDT_OK;
	if (!packed_words || !offsets)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = add_args_ok(nreads, paired);
	if (rc == SDT_OK) rc = support_open(c, "sdt_gpu_unitigs_support_add");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_support_add");
	if (rc != SDT_OK) return rc;
	StreamCheck in;
	rc = stream_args_ok(offsets, nreads, nwords, &in);
	if (rc != SDT_OK) return rc;
	if (in.longest >> 32)
		return fail(SDT_EINVAL, "a read of %llu bases: the k-mers of a segment are counted in 32 bits", (unsigned long long)in.longest);
	SDT_ENTER(c);
	// (a piece of a paired batch holds whole pairs)
	rc = for_each_piece(c, packed_words, offsets, nreads, paired ? 2 : 1, "unitig support staging", [&](const StagedPiece &p) -> int {
		const int rc = add_batch(c, p.d_words, p.d_offs, p.nr, paired);
		if (rc != SDT_OK) return rc;
		HIPCHK(hipStreamSynchronize(c->stream));             // (the next piece is staged in the same buffers)
		return SDT_OK;
	});
	if (rc != SDT_OK) return rc;
	return add_finish(c);
}

int sdt_gpu_unitigs_support_unitigs(sdt_ctx *c, uint64_t first, uint64_t n, sdt_unitig_support *out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0)
		return SDT_OK;
	if (!out)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = support_open(c, "sdt_gpu_unitigs_support_unitigs");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_unitigs_support_unitigs", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	HIPCHK(hipMemcpyAsync(out, tally_of(c).us + first, n * sizeof(UnitigSupport), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return SDT_OK;
}

int sdt_gpu_unitigs_support_links(sdt_ctx *c, uint64_t first, uint64_t n, sdt_link_support *out, uint64_t capacity, uint64_t *n_links)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (n == 0) {
		if (n_links) *n_links = 0;
		return SDT_OK;
	}
	if (!n_links || (!out && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	int rc = support_open(c, "sdt_gpu_unitigs_support_links");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_support_links");
	if (rc == SDT_OK) rc = range_ok(c, "sdt_gpu_unitigs_support_links", first, n);
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	uint64_t total = 0;
	rc = sdt_gpu_unitigs_links(c, first, n, nullptr, 0, &total, nullptr);
	if (rc != SDT_OK) return rc;
	*n_links = total;
	if (!out && capacity == 0)
		return SDT_OK;                                       // (the size only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_links: %llu links, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	if (total == 0)
		return SDT_OK;
	std::vector<sdt_unitig_link> links((size_t)total);
	rc = sdt_gpu_unitigs_links(c, first, n, links.data(), total, &total, nullptr);
	if (rc != SDT_OK) return rc;
	DevBuf d_links, d_out;
	rc = d_links.get(total * sizeof(UnitigLink), "sdt_gpu_unitigs_support_links: links");
	if (rc == SDT_OK) rc = d_out.get(total * sizeof(LinkSupport), "sdt_gpu_unitigs_support_links: tallies");
	if (rc != SDT_OK) return rc;
	HIPCHK(hipMemcpyAsync(d_links.p, links.data(), total * sizeof(UnitigLink), hipMemcpyHostToDevice, c->stream));
	const SupportTally t = tally_of(c);
	by_key_width(c, [&](auto nw) {
		constexpr int NW = decltype(nw)::value;
		hipLaunchKernelGGL(k_sp_links<NW>, dim3(scan_grid(c, total)), dim3(TPB), 0, c->stream, (const UnitigLink *)d_links.p, total, (const uint64_t *)c->ug.keys, c->K,
		                   (const unsigned long long *)t.along, (LinkSupport *)d_out.p);
	});
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.p, total * sizeof(LinkSupport), hipMemcpyDeviceToHost, c->stream);
	const hipError_t e2 = hipStreamSynchronize(c->stream);       // (the buffers go when this returns)
	HIPCHK(e);
	HIPCHK(e2);
	return SDT_OK;
}

int sdt_gpu_unitigs_support_junctions(sdt_ctx *c, sdt_unitig_junction *out, uint64_t capacity, uint64_t *n_out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!n_out || (!out && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	const int rc = support_open(c, "sdt_gpu_unitigs_support_junctions");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	if (!c->ug.sup_jn_slots)
		return fail(SDT_EINVAL, "sdt_gpu_unitigs_support_junctions: junction_capacity was 0 at sdt_gpu_unitigs_support_begin: the junctions are not kept");
	unsigned long long h[SP_COUNTERS];
	const int rc2 = counters(c, h);
	if (rc2 != SDT_OK) return rc2;
	if (junctions_full(c, h))
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_junctions: the junction set filled up (%llu junctions and more for a capacity of %llu): the list is lost",
		            h[SP_N_JUNCTIONS], (unsigned long long)c->ug.sup_jn_cap);
	const uint64_t total = h[SP_N_JUNCTIONS];
	*n_out = total;
	if (!out && capacity == 0)
		return SDT_OK;                                       // (the size only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_junctions: %llu junctions, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	std::vector<JunctionEnt> ent((size_t)c->ug.sup_jn_slots);
	HIPCHK(hipMemcpyAsync(ent.data(), tally_of(c).jn, ent.size() * sizeof(JunctionEnt), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	uint64_t k = 0;
	for (const JunctionEnt &e : ent) {
		if (e.key == SP_EMPTY) continue;
		if (k == total)
			return fail(SDT_ESTATE, "sdt_gpu_unitigs_support_junctions: the set holds more than the %llu entries it counted", (unsigned long long)total);
		out[k++] = sdt_unitig_junction{e.from, (uint32_t)((e.key - 1) >> 4) << 1, e.to, 0u, e.count};
	}
	if (k != total)
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_support_junctions: the set holds %llu entries, it counted %llu", (unsigned long long)k, (unsigned long long)total);
	std::sort(out, out + total, [](const sdt_unitig_junction &a, const sdt_unitig_junction &b) {
		return a.via != b.via ? a.via < b.via : a.from != b.from ? a.from < b.from : a.to < b.to;
	});
	return SDT_OK;
}

int sdt_gpu_unitigs_support_mates(sdt_ctx *c, sdt_mate_link *out, uint64_t capacity, uint64_t *n_out)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!n_out || (!out && capacity))
		return fail(SDT_EINVAL, "NULL argument");
	const int rc = support_open(c, "sdt_gpu_unitigs_support_mates");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	if (!c->ug.sup_mt_slots)
		return fail(SDT_EINVAL, "sdt_gpu_unitigs_support_mates: mate_capacity was 0 at sdt_gpu_unitigs_support_begin: the mate links are not kept");
	unsigned long long h[SP_COUNTERS];
	const int rc2 = counters(c, h);
	if (rc2 != SDT_OK) return rc2;
	if (mates_full(c, h))
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_mates: the mate-link set filled up (%llu mate links and more for a capacity of %llu): the list is lost",
		            h[SP_N_MATES], (unsigned long long)c->ug.sup_mt_cap);
	const uint64_t total = h[SP_N_MATES];
	*n_out = total;
	if (!out && capacity == 0)
		return SDT_OK;                                       // (the size only)
	if (total > capacity)
		return fail(SDT_EFULL, "sdt_gpu_unitigs_support_mates: %llu mate links, room for %llu", (unsigned long long)total, (unsigned long long)capacity);
	std::vector<MateEnt> ent((size_t)c->ug.sup_mt_slots);
	HIPCHK(hipMemcpyAsync(ent.data(), tally_of(c).mt, ent.size() * sizeof(MateEnt), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	uint64_t k = 0;
	for (const MateEnt &e : ent) {
		if (e.key == SP_EMPTY) continue;
		if (k == total)
			return fail(SDT_ESTATE, "sdt_gpu_unitigs_support_mates: the set holds more than the %llu entries it counted", (unsigned long long)total);
		out[k++] = sdt_mate_link{(uint32_t)((e.key - 1) >> 32), (uint32_t)(e.key - 1), e.count};
	}
	if (k != total)
		return fail(SDT_ESTATE, "sdt_gpu_unitigs_support_mates: the set holds %llu entries, it counted %llu", (unsigned long long)k, (unsigned long long)total);
	std::sort(out, out + total, [](const sdt_mate_link &a, const sdt_mate_link &b) { return a.from != b.from ? a.from < b.from : a.to < b.to; });
	return SDT_OK;
}

int sdt_gpu_unitigs_support_totals(sdt_ctx *c, uint64_t totals[12])
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	if (!totals)
		return fail(SDT_EINVAL, "NULL argument");
	int rc = support_open(c, "sdt_gpu_unitigs_support_totals");
	if (rc == SDT_OK) rc = search_ready(c, "sdt_gpu_unitigs_support_totals");
	if (rc != SDT_OK) return rc;
	SDT_ENTER(c);
	unsigned long long h[SP_COUNTERS];
	rc = counters(c, h);
	if (rc != SDT_OK) return rc;
	// the traversals without a record: what was added to the link slots that no record of the list has
	unsigned long long with_record = 0;
	if (h[SP_TRAV]) {
		std::vector<sdt_unitig_link> links;
		rc = links_of(c, 0, c->ug.n, links);
		if (rc != SDT_OK) return rc;
		std::vector<unsigned long long> along((size_t)(8 * c->ug.n));
		HIPCHK(hipMemcpyAsync(along.data(), tally_of(c).along, along.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		for (const sdt_unitig_link &l : links) with_record += along[(size_t)(((uint64_t)l.from << 1 | (l.info & 1u)) << 2 | (l.info >> 2 & 3u))];
	}
	for (int i = 0; i < 12; i++) totals[i] = h[i];
	totals[SP_NO_RECORD] = h[SP_TRAV] - with_record;
	totals[SP_DROPPED] = h[SP_JUNCTIONS_DROPPED] + h[SP_MATES_DROPPED];
	return SDT_OK;
}

int sdt_gpu_unitigs_support_end(sdt_ctx *c)
{
	if (!c)
		return fail(SDT_EINVAL, "ctx is NULL");
	SDT_ENTER(c);
	HIPCHK(hipStreamSynchronize(c->stream));
	support_free(c);
	return SDT_OK;
}

} // extern "C"
