// sdt_read_plan.h -- what the read stages on the counted table (profile, correct, normalise, trim: sdt_search.hip, sdt_correct.hip,
// sdt_select.hip, sdt_trim.hip) decide on the host before anything reaches the device, as PURE functions: the launch geometry of a
// strip kernel, the check of a host stream's offsets, and the cut of a host batch into the pieces that are staged one at a time.
// sdt_readstage.hpp calls them for every stage; tools/read_plan_check.cpp (tests/test_read_plan.py) calls them on the CPU under
// sanitizers.  No HIP in here.
#pragma once
#include <stdint.h>

namespace sdt {

// ---- the launch geometry of a strip kernel ----
// A strip kernel gives every wavefront one read and a strip of LDS with one 32-bit count per k-mer of the longest read; a workgroup
// has 64 KiB of strips.  Reads of up to 4 096 k-mers run 4 wavefronts per workgroup, up to 8 192 two, up to 16 384 one; longer reads
// do not fit (the length table of the README).
constexpr uint64_t STRIP_LDS_BYTES = 64 * 1024;
constexpr uint64_t STRIP_MAX_KMERS = STRIP_LDS_BYTES / sizeof(uint32_t);

struct StripGeometry {
	uint64_t max_read_len;         // as given, raised to K
	uint64_t mk;                   // k-mers of a read of that length
	bool fits;                     // false: mk > STRIP_MAX_KMERS, and nothing below is set
	int waves;                     // wavefronts of a workgroup that take a read each
	uint32_t lds_bytes;            // 4 * mk * waves
	uint32_t blocks;
};

inline StripGeometry strip_geometry(int K, uint64_t nreads, uint64_t max_read_len, int cu_count)
{
	StripGeometry g = {max_read_len < (uint64_t)K ? (uint64_t)K : max_read_len, 0, false, 0, 0, 0};
	g.mk = g.max_read_len - (uint64_t)K + 1;
	g.fits = g.mk <= STRIP_MAX_KMERS;
	if (!g.fits) return g;
	const uint64_t per_wave = g.mk * sizeof(uint32_t);
	g.waves = 4;
	while (g.waves > 1 && per_wave * g.waves > STRIP_LDS_BYTES) g.waves >>= 1;
	g.lds_bytes = (uint32_t)(per_wave * g.waves);
	uint64_t blocks = nreads / g.waves + (nreads % g.waves != 0);
	const uint64_t cap = (uint64_t)cu_count * 32;      // (the kernels stride over the reads)
	if (blocks > cap) blocks = cap;
	if (blocks == 0) blocks = 1;
	g.blocks = (uint32_t)blocks;
	return g;
}

// the longest read so far, over the millions of reads of a batch: a branch that is almost never taken, where a conditional move per
// read is a chain of dependent instructions as long as the batch (2 ms per 4 M reads in the wall clock of a host form)
inline void raise_to(uint64_t &longest, uint64_t len)
{
	if (__builtin_expect(len > longest, 0)) longest = len;
}

// ---- a host stream: nreads reads of 2-bit bases in nwords words, read i = bases [offsets[i], offsets[i + 1]) ----
enum StreamFault { STREAM_OK = 0, STREAM_NOT_MONOTONIC, STREAM_TOO_SHORT };

struct StreamCheck {
	StreamFault fault;
	uint64_t read;                 // STREAM_NOT_MONOTONIC: the first read that ends before it starts
	uint64_t need_words;           // the words the stream takes with its pad words (0 for no reads: then offsets is not looked at)
	uint64_t longest;              // bases of the longest read
};

inline StreamCheck check_stream(const uint64_t *offsets, uint64_t nreads, uint64_t nwords, uint64_t pad)
{
	StreamCheck s = {STREAM_OK, 0, 0, 0};
	for (uint64_t i = 0; i < nreads; i++) {
		if (offsets[i + 1] < offsets[i]) {
			s.fault = STREAM_NOT_MONOTONIC;
			s.read = i;
			return s;
		}
		raise_to(s.longest, offsets[i + 1] - offsets[i]);
	}
	s.need_words = nreads ? ((offsets[nreads] + 15) >> 4) + pad : 0;
	if (s.need_words > nwords) s.fault = STREAM_TOO_SHORT;
	return s;
}

// ---- the piece of a checked stream that starts at read r0 ----
// A piece is a run of units of `step` reads (2: the mates of a pair stay together; nreads is then even).  The first unit is always
// taken, further ones while the piece stays below piece_reads reads and within piece_bases bases.  The piece is staged as the words
// that hold its bases and `pad` words behind them, with its offsets rebased to the first of those words.
struct ReadPiece {
	uint64_t r1;                   // reads [r0, r1)
	uint64_t maxlen;               // bases of the longest of them
	uint64_t w0, nwords;           // words [w0, w0 + nwords) of the stream; read i of the piece starts at base offsets[r0 + i] - 16 * w0 of them
};

inline ReadPiece next_piece(const uint64_t *offsets, uint64_t nreads, uint64_t r0, uint64_t step, uint64_t piece_reads, uint64_t piece_bases,
                            uint64_t pad)
{
	// the units the reads cap allows; the offsets of a checked stream ascend, so those of them that stay within piece_bases are a
	// prefix, and its end is found by bisection (a walk over every read of a batch of millions showed in the host forms' wall clock)
	uint64_t lo = 1, hi = (piece_reads + step - 1) / step;
	if (hi > (nreads - r0) / step) hi = (nreads - r0) / step;
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1) / 2;
		if (offsets[r0 + mid * step] - offsets[r0] <= piece_bases) lo = mid; else hi = mid - 1;
	}
	ReadPiece p = {r0 + lo * step, 0, offsets[r0] >> 4, 0};
	for (uint64_t i = r0; i < p.r1; i++) raise_to(p.maxlen, offsets[i + 1] - offsets[i]);
	p.nwords = ((offsets[p.r1] + 15) >> 4) + pad - p.w0;
	return p;
}

} // namespace sdt
