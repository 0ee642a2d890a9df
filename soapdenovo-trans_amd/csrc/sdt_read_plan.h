// sdt_read_plan.h -- what the read stages on the counted table (profile, correct, normalise, trim: sdt_search.hip, sdt_correct.hip,
// sdt_select.hip, sdt_trim.hip) decide on the host before anything reaches the device, as PURE functions: the launch geometry of a
// strip kernel, the check of a host stream's offsets, and the cut of a host batch into the pieces that are staged one at a time.
// sdt_readstage.hpp calls them for every stage; tools/read_plan_check.cpp (tests/test_read_plan.py) calls them on the CPU under
// sanitizers.  The six stages that need no table have theirs here too: the duplicate filter (sdt_dedup.hip), the adapter and tail
// clipping (sdt_clip.hip), the mate overlap (sdt_overlap.hip), the low-complexity filter (sdt_complexity.hip), the reference screen
// (sdt_screen.hip) and the quality trim (sdt_quality.hip), which also has its cut of a byte stream into pieces here.  The merge of
// overlapping mates (sdt_merge.hip) has its refusals and the decision of a pair here, the QC report (sdt_qc.hip) its refusals, the
// layout of the report and its grid.  No HIP in here.
#pragma once
#include <stdint.h>

namespace sdt {

// ---- the grid of a kernel that gives every wavefront one item (a read, a pair) and strides over the rest ----
// `waves` wavefronts of a workgroup take an item each.  The workgroups that `items` items fill, cu_count * 32 at most and one at least;
// forced != 0 (SDT_WAVE_BLOCKS: test hook) puts that many in the place of cu_count * 32, so that a batch of test size goes round the
// kernels' loop over the items many times.  Every read stage and align_reads take their grid from here.
constexpr uint32_t wave_blocks(uint64_t items, uint64_t waves, int cu_count, uint64_t forced)
{
	const uint64_t blocks = items / waves + (items % waves != 0);
	const uint64_t cap = forced ? forced : (uint64_t)cu_count * 32;      // (the kernels stride over the items)
	return (uint32_t)(blocks > cap ? cap : (blocks ? blocks : 1));
}

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

inline StripGeometry strip_geometry(int K, uint64_t nreads, uint64_t max_read_len, int cu_count, uint64_t forced_blocks = 0)
{
	StripGeometry g = {max_read_len < (uint64_t)K ? (uint64_t)K : max_read_len, 0, false, 0, 0, 0};
	g.mk = g.max_read_len - (uint64_t)K + 1;
	g.fits = g.mk <= STRIP_MAX_KMERS;
	if (!g.fits) return g;
	const uint64_t per_wave = g.mk * sizeof(uint32_t);
	g.waves = 4;
	while (g.waves > 1 && per_wave * g.waves > STRIP_LDS_BYTES) g.waves >>= 1;
	g.lds_bytes = (uint32_t)(per_wave * g.waves);
	g.blocks = wave_blocks(nreads, (uint64_t)g.waves, cu_count, forced_blocks);
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

// ---- units of the reads kept in HBM: single reads and interleaved pairs, by read ordinal (select_kept_reads, dedup_kept_reads) ----
// (tools/dedup_plan_check.cpp holds the cut to a walk over the ordinals)
// pair_ranges[2i], pair_ranges[2i + 1] = [first, end) of ordinals that hold pairs, the first mate at first + 2t: ascending, disjoint,
// of even length.  Returns n_ranges when they are, else the index of the first range that is not, and why.
enum PairRangeFault { PAIR_RANGES_OK = 0, PAIR_RANGE_NOT_PAIRS, PAIR_RANGE_OVERLAPS };

inline uint64_t check_pair_ranges(const uint64_t *pair_ranges, uint64_t n_ranges, PairRangeFault *fault)
{
	*fault = PAIR_RANGES_OK;
	for (uint64_t i = 0; i < n_ranges; i++) {
		const uint64_t first = pair_ranges[2 * i], end = pair_ranges[2 * i + 1];
		if (end < first || ((end - first) & 1)) { *fault = PAIR_RANGE_NOT_PAIRS; return i; }
		if (i && first < pair_ranges[2 * i - 1]) { *fault = PAIR_RANGE_OVERLAPS; return i; }
	}
	return n_ranges;
}

// a stretch of units: unit unit0 + t is the read at ordinal ord0 + t * stride, and with stride == 2 its mate at the next ordinal
struct UnitStretch {
	uint64_t unit0, ord0, stride;
};

// The units of ordinals [0, n_ord) under checked pair ranges, as stretches in ascending order: single reads up to a range, the pairs
// of the range, and so on up to the last ordinal.  A range is cut at n_ord (a pair that n_ord cuts is a unit of its first mate); empty
// stretches are left out.  out holds 2 * n_ranges + 1 stretches at most (NULL: they are only counted).  Returns the stretches;
// *units: the units in them.
inline uint64_t cut_unit_stretches(const uint64_t *pair_ranges, uint64_t n_ranges, uint64_t n_ord, UnitStretch *out, uint64_t *units)
{
	uint64_t n = 0, at = 0;
	*units = 0;
	for (uint64_t i = 0; i < n_ranges && at < n_ord; i++) {
		const uint64_t first = pair_ranges[2 * i], end = pair_ranges[2 * i + 1] < n_ord ? pair_ranges[2 * i + 1] : n_ord;
		if (first >= n_ord || end == first) continue;
		if (first > at) {
			if (out) out[n] = {*units, at, 1};
			n++;
			*units += first - at;
		}
		if (out) out[n] = {*units, first, 2};
		n++;
		*units += (end - first + 1) >> 1;
		at = pair_ranges[2 * i + 1];
	}
	if (at < n_ord) {
		if (out) out[n] = {*units, at, 1};
		n++;
		*units += n_ord - at;
	}
	return n;
}

// ---- the duplicate filter (sdt_dedup.hip): a hash set of unit fingerprints, open addressing, linear probing ----
// the table for `units` units: a power of two of at least 2 * units slots (load <= 1/2: a probe ends), less than 4 * units beyond one unit
constexpr uint64_t DEDUP_SLOT_BYTES = 24;                // fingerprint, representative, copies
constexpr uint64_t DEDUP_ENT_BYTES = 24;                 // kept form, per ordinal: fingerprint, where the bases start, length
constexpr int DEDUP_MAX_ROUNDS = 64;                     // every round resolves a class per occupied slot at least; past this: SDT_ELIMIT

inline uint64_t dedup_table_slots(uint64_t units)
{
	uint64_t slots = 2;
	while (slots < 2 * units && slots < (1ULL << 62)) slots <<= 1;
	return slots;
}

// ---- adapter and tail clipping (sdt_clip.hip): what is refused before any launch, and the adapters as the kernel takes them ----
// (tools/clip_plan_check.cpp runs both checks and the split on the CPU under sanitizers)
constexpr uint32_t CLIP_MAX_ADAPTERS = 256;              // SDT_CLIP_MAX_ADAPTERS
constexpr uint32_t CLIP_MAX_ADAPTER_LEN = 128;           // SDT_CLIP_MAX_ADAPTER_LEN
constexpr uint32_t CLIP_ADAPTER_CHUNKS = CLIP_MAX_ADAPTER_LEN / 32;

struct ClipParams {                                      // == sdt_clip_params of include/sdt_gpu.h
	uint32_t min_overlap, max_err_pct, min_len, min_tail, tail_err_pct, tail3_bases, tail5_bases, flags;
};

enum ClipFault {
	CLIP_OK = 0,
	CLIP_FLAGS, CLIP_MIN_OVERLAP, CLIP_MAX_ERR_PCT, CLIP_TAIL_ERR_PCT, CLIP_TAIL3_BASES, CLIP_TAIL5_BASES, CLIP_MIN_TAIL,      // the parameters
	CLIP_TOO_MANY, CLIP_OFFSETS, CLIP_ADAPTER_EMPTY, CLIP_ADAPTER_LONG, CLIP_ADAPTER_SHORT, CLIP_ADAPTER_END                   // the adapter set
};

// the first field of the parameters that is refused, in the order of the struct's rules in include/sdt_gpu.h
inline ClipFault check_clip_params(const ClipParams &p)
{
	if (p.flags != 0) return CLIP_FLAGS;
	if (p.min_overlap == 0) return CLIP_MIN_OVERLAP;
	if (p.max_err_pct > 100) return CLIP_MAX_ERR_PCT;
	if (p.tail_err_pct > 100) return CLIP_TAIL_ERR_PCT;
	if (p.tail3_bases > 15) return CLIP_TAIL3_BASES;
	if (p.tail5_bases > 15) return CLIP_TAIL5_BASES;
	if (p.min_tail == 0 && (p.tail3_bases | p.tail5_bases)) return CLIP_MIN_TAIL;
	return CLIP_OK;
}

// n adapters of offsets[i + 1] - offsets[i] bases, ends[i] = 0 (3') or 1 (5').  *index: the adapter that is refused (n for CLIP_TOO_MANY)
inline ClipFault check_adapter_set(const uint64_t *offsets, const uint8_t *ends, uint64_t n, uint32_t min_overlap, uint64_t *index)
{
	*index = n;
	if (n > CLIP_MAX_ADAPTERS) return CLIP_TOO_MANY;
	for (uint64_t i = 0; i < n; i++) {
		*index = i;
		if (offsets[i + 1] < offsets[i]) return CLIP_OFFSETS;
		const uint64_t m = offsets[i + 1] - offsets[i];
		if (m == 0) return CLIP_ADAPTER_EMPTY;
		if (m > CLIP_MAX_ADAPTER_LEN) return CLIP_ADAPTER_LONG;
		if (m < min_overlap) return CLIP_ADAPTER_SHORT;
		if (ends[i] > 1) return CLIP_ADAPTER_END;
	}
	*index = n;
	return CLIP_OK;
}

// An adapter as the kernel takes it: 32 bases per 64-bit chunk, so that one XOR with a window of the read compares 32 bases.
//   3': chunk c holds bases [32 c, 32 c + 32), the first in the most significant pair, zero past the adapter's end
//   5': chunk c holds bases [m - 32 c - 32, m - 32 c), the LAST in the least significant pair, zero before the adapter's start
struct ClipAdapter {
	uint64_t chunk[CLIP_ADAPTER_CHUNKS];
	uint32_t m, id;                // bases; the adapter's index in the caller's set
};

// adapter `id` of a checked set (words: 16 bases per word, first base in the most significant pair)
inline ClipAdapter split_adapter(const uint32_t *words, const uint64_t *offsets, const uint8_t *ends, uint32_t id)
{
	ClipAdapter a = {{0, 0, 0, 0}, (uint32_t)(offsets[id + 1] - offsets[id]), id};
	for (uint32_t k = 0; k < a.m; k++) {
		const uint64_t pos = offsets[id] + k;
		const uint64_t b = (words[pos >> 4] >> (30 - 2 * (pos & 15))) & 3u;
		if (ends[id] == 0) a.chunk[k >> 5] |= b << (62 - 2 * (k & 31));
		else a.chunk[(a.m - 1 - k) >> 5] |= b << (2 * ((a.m - 1 - k) & 31));
	}
	return a;
}

// ---- mate overlap (sdt_overlap.hip): what is refused before any launch, and the shifts a pair is tried at ----
// (tools/overlap_plan_check.cpp runs the check and holds the span of the shifts to a walk over every shift)
struct OverlapParams {                                   // == sdt_overlap_params of include/sdt_gpu.h
	uint32_t min_overlap, max_err_pct, min_len, flags;
};

enum OverlapFault { OVERLAP_OK = 0, OVERLAP_FLAGS, OVERLAP_MIN_OVERLAP, OVERLAP_MAX_ERR_PCT, OVERLAP_ODD_READS };

// the first thing that is refused, in the order of the rules in include/sdt_gpu.h; dense_reads: the reads of a dense form, in which
// reads 2t and 2t + 1 are mates (0 for the kept form)
inline OverlapFault check_overlap_params(const OverlapParams &p, uint64_t dense_reads)
{
	if (p.flags != 0) return OVERLAP_FLAGS;
	if (p.min_overlap == 0) return OVERLAP_MIN_OVERLAP;
	if (p.max_err_pct > 100) return OVERLAP_MAX_ERR_PCT;
	if (dense_reads & 1) return OVERLAP_ODD_READS;
	return OVERLAP_OK;
}

// Mates of La and Lb bases: the shifts d whose overlap o = min(La, d + Lb) - max(0, d) is at least min_overlap (>= 1) are the
// overlap_shifts() consecutive ones from d = min_overlap - Lb, up to d = La - min_overlap; none when a mate is shorter than min_overlap.
// (constexpr: the kernel calls it too)
constexpr uint64_t overlap_shifts(uint64_t La, uint64_t Lb, uint32_t min_overlap)
{
	return La < min_overlap || Lb < min_overlap ? 0 : La + Lb - 2 * (uint64_t)min_overlap + 1;
}

// ---- merging the mates of a pair (sdt_merge.hip): what is refused before any launch, and whether a pair of overlap records merges ----
// (tools/merge_plan_check.cpp runs the check and holds the decision to the rule's four lines and to a cover of every position)
struct MergeParams {                                     // == sdt_merge_params of include/sdt_gpu.h
	uint32_t min_len, max_len, phred_offset, flags;
};

enum MergeFault { MERGE_OK = 0, MERGE_FLAGS, MERGE_MAX_LEN, MERGE_PHRED_OFFSET, MERGE_ODD_READS };

// the first thing that is refused, in the order of the rules in include/sdt_gpu.h; with_quals: qualities are given (phred_offset is
// looked at only then); dense_reads: the reads of a dense form, in which reads 2t and 2t + 1 are mates (0 for the kept form)
inline MergeFault check_merge_params(const MergeParams &p, bool with_quals, uint64_t dense_reads)
{
	if (p.flags != 0) return MERGE_FLAGS;
	if (p.max_len != 0 && p.max_len < (p.min_len > 1 ? p.min_len : 1u)) return MERGE_MAX_LEN;
	if (with_quals && p.phred_offset != 0 && p.phred_offset != 33 && p.phred_offset != 64) return MERGE_PHRED_OFFSET;
	if (dense_reads & 1) return MERGE_ODD_READS;
	return MERGE_OK;
}

// Mates of La and Lb bases whose overlap records say the inserts Fa and Fb: the length of the merged read (Fa), 0 when the pair is not
// merged (no overlap: Fa == Fb == 0, or a length that min_len or max_len refuses), MERGE_INCONSISTENT when the two records cannot
// come from one overlap of these mates: Fa != Fb, or an insert that no shift -Lb < d < La gives (F >= La + Lb).  For a merged pair
// every position of [0, F) is covered by a or by b' and at least one by both.  (constexpr: the kernel and the scans call it too)
constexpr int64_t MERGE_INCONSISTENT = -1;
constexpr int64_t merge_decide(uint64_t La, uint64_t Lb, uint32_t Fa, uint32_t Fb, uint32_t min_len, uint32_t max_len)
{
	if (Fa != Fb) return MERGE_INCONSISTENT;
	if (Fa == 0) return 0;
	if ((uint64_t)Fa >= La + Lb) return MERGE_INCONSISTENT;
	if (Fa < (min_len > 1 ? min_len : 1u)) return 0;
	if (max_len != 0 && Fa > max_len) return 0;
	return (int64_t)Fa;
}
// the 64-bit values of 32 bases that a merged read of F bases takes in the scratch stream
constexpr uint64_t merge_chunks(uint64_t F) { return (F + 31) >> 5; }

// ---- low-complexity reads (sdt_complexity.hip): what is refused before any launch, and the windows a read is scored in ----
// (tools/complexity_plan_check.cpp runs the check and holds the windows to a walk over every base)
struct ComplexityParams {                                // == sdt_complexity_params of include/sdt_gpu.h
	uint32_t max_score_pct, max_low_pct, min_len, flags;
};
constexpr uint32_t COMPLEXITY_TRIM = 1u;                 // SDT_COMPLEXITY_TRIM
constexpr uint64_t COMPLEXITY_WINDOW = 64, COMPLEXITY_STEP = 32;

enum ComplexityFault { COMPLEXITY_OK = 0, COMPLEXITY_FLAGS, COMPLEXITY_MAX_SCORE_PCT, COMPLEXITY_MAX_LOW_PCT, COMPLEXITY_TRIM_MAX_LOW_PCT };

// the first field that is refused, in the order of the rules in include/sdt_gpu.h
inline ComplexityFault check_complexity_params(const ComplexityParams &p)
{
	if (p.flags & ~COMPLEXITY_TRIM) return COMPLEXITY_FLAGS;
	if (p.max_score_pct == 0 || p.max_score_pct > 100) return COMPLEXITY_MAX_SCORE_PCT;
	if (p.max_low_pct > 100) return COMPLEXITY_MAX_LOW_PCT;
	if ((p.flags & COMPLEXITY_TRIM) && p.max_low_pct != 0) return COMPLEXITY_TRIM_MAX_LOW_PCT;
	return COMPLEXITY_OK;
}

// A read of L bases is scored in complexity_windows(L) windows of 64 bases that start every 32 bases; window j is
// [complexity_window_begin(j), complexity_window_end(j, L)).  Every base is in a window, the last window ends at L and has more than 32
// bases unless it is the only one.  Bases [32 k, 32 k + 32) are covered by the windows k - 1 and k that exist, and by no other.
// (constexpr: the kernel calls them too)
constexpr uint64_t complexity_windows(uint64_t L)
{
	return L == 0 ? 0 : (L <= 2 * COMPLEXITY_STEP ? 1 : (L + COMPLEXITY_STEP - 1) / COMPLEXITY_STEP - 1);
}
constexpr uint64_t complexity_window_begin(uint64_t j) { return j * COMPLEXITY_STEP; }
constexpr uint64_t complexity_window_end(uint64_t j, uint64_t L)
{
	return j * COMPLEXITY_STEP + COMPLEXITY_WINDOW < L ? j * COMPLEXITY_STEP + COMPLEXITY_WINDOW : L;
}

// ---- the reference screen (sdt_screen.hip): what is refused before any launch, the size of the set's table, the rule of a read and
// of a unit, and the unit verdicts of the kept form ----
// (tools/screen_plan_check.cpp runs the check and holds the unit verdicts to a walk over every ordinal)
struct ScreenParams {                                    // == sdt_screen_params of include/sdt_gpu.h
	uint32_t min_hits, min_hit_pct, flags, reserved;
};
struct ScreenRec {                                       // == sdt_read_screen of include/sdt_gpu.h
	uint32_t kmers, hits, ref, start, len, verdict;
};
constexpr uint32_t SCREEN_KEEP_MATCHED = 1u;             // SDT_SCREEN_KEEP_MATCHED
constexpr uint32_t SCREEN_PER_READ = 1u << 31;           // (internal, never a caller's: no verdicts, every record keeps len = L; the kept form)
constexpr uint32_t SCREEN_NO_REF = 0xFFFFFFFFu;          // SDT_SCREEN_NO_REF
constexpr uint32_t SCREEN_MIN_K = 11, SCREEN_MAX_K = 31;
constexpr uint64_t SCREEN_MIN_SLOTS = 1024;

enum ScreenFault { SCREEN_OK = 0, SCREEN_MIN_HIT_PCT, SCREEN_FLAGS, SCREEN_RESERVED };

// the first field that is refused, in the order of the rules in include/sdt_gpu.h
inline ScreenFault check_screen_params(const ScreenParams &p)
{
	if (p.min_hit_pct > 100) return SCREEN_MIN_HIT_PCT;
	if (p.flags & ~SCREEN_KEEP_MATCHED) return SCREEN_FLAGS;
	if (p.reserved != 0) return SCREEN_RESERVED;
	return SCREEN_OK;
}

// the k-mer start positions of a checked stream of sequences: what the table is sized for (a k-mer that occurs twice counts twice)
inline uint64_t screen_positions(const uint64_t *offsets, uint64_t nseqs, uint32_t k)
{
	uint64_t n = 0;
	for (uint64_t i = 0; i < nseqs; i++) {
		const uint64_t len = offsets[i + 1] - offsets[i];
		if (len >= k) n += len - k + 1;
	}
	return n;
}

// the table for that many positions: the power of two >= 2 * positions, SCREEN_MIN_SLOTS at least (load <= 1/2: a probe ends)
inline uint64_t screen_table_slots(uint64_t positions)
{
	uint64_t slots = SCREEN_MIN_SLOTS;
	while (slots < 2 * positions && slots < (1ULL << 62)) slots <<= 1;
	return slots;
}

// (SDT_SCREEN_SLOTS) a forced slot count holds the set iff it is a power of two with an empty slot left whatever the k-mers are
constexpr bool screen_forced_slots_ok(uint64_t forced, uint64_t positions) { return forced && !(forced & (forced - 1)) && forced > positions; }

// (constexpr: the kernel calls them too)
constexpr bool screen_read_matched(uint64_t kmers, uint64_t hits, const ScreenParams &p)
{
	return hits >= (p.min_hits > 1 ? p.min_hits : 1u) && 100 * hits >= (uint64_t)p.min_hit_pct * kmers;
}
constexpr bool screen_unit_dropped(bool matched, uint32_t flags) { return (flags & SCREEN_KEEP_MATCHED) ? !matched : matched; }

// The kept form: rec[o] for the ordinals o < n_ord with present[o] != 0 hold what SCREEN_PER_READ leaves (kmers, hits, ref, len = L).
// The units are those of cut_unit_stretches under checked pair ranges, and a pair of which one mate is present is a unit of that
// read.  Every present record gets its unit's start, len and verdict; the others are not looked at.  Returns the reads kept.
inline uint64_t screen_unit_verdicts(ScreenRec *rec, const uint8_t *present, uint64_t n_ord, const uint64_t *pair_ranges, uint64_t n_ranges,
                                     const ScreenParams &p)
{
	uint64_t kept = 0, at = 0;
	auto matched = [&](uint64_t o) { return present[o] && screen_read_matched(rec[o].kmers, rec[o].hits, p); };
	auto decide = [&](uint64_t o, bool dropped) {
		if (!present[o]) return;
		rec[o].start = 0;
		rec[o].verdict = dropped ? 1u : 0u;
		if (dropped) rec[o].len = 0; else kept++;
	};
	auto singles = [&](uint64_t a, uint64_t e) {
		for (uint64_t o = a; o < e; o++) decide(o, screen_unit_dropped(matched(o), p.flags));
	};
	for (uint64_t i = 0; i < n_ranges && at < n_ord; i++) {
		const uint64_t first = pair_ranges[2 * i], end = pair_ranges[2 * i + 1] < n_ord ? pair_ranges[2 * i + 1] : n_ord;
		if (first >= n_ord || end == first) continue;
		singles(at, first);
		for (uint64_t o = first; o < end; o += 2) {
			const bool m = matched(o) || (o + 1 < end && matched(o + 1)), d = screen_unit_dropped(m, p.flags);
			decide(o, d);
			if (o + 1 < end) decide(o + 1, d);
		}
		at = pair_ranges[2 * i + 1];
	}
	if (at < n_ord) singles(at, n_ord);
	return kept;
}

// ---- quality trimming (sdt_quality.hip): what is refused before any launch, the expected errors of a quality, and a host stream of
// quality bytes cut into pieces ----
// (tools/quality_plan_check.cpp runs the check, holds the table to the exact rounding and the pieces to a cover of every read)
struct QualityParams {                                   // == sdt_quality_params of include/sdt_gpu.h
	uint32_t phred_offset, cut_q, low_q, max_low_pct, max_ee_ppm, min_len, flags, reserved;
};
constexpr uint32_t QUALITY_MAX_Q = 93;                   // '~' - '!': the highest quality a FASTQ byte can say

enum QualityFault { QUALITY_OK = 0, QUALITY_PHRED_OFFSET, QUALITY_CUT_Q, QUALITY_LOW_Q, QUALITY_MAX_LOW_PCT, QUALITY_FLAGS, QUALITY_RESERVED };

// the first field that is refused, in the order of the rules in include/sdt_gpu.h
inline QualityFault check_quality_params(const QualityParams &p)
{
	if (p.phred_offset != 0 && p.phred_offset != 33 && p.phred_offset != 64) return QUALITY_PHRED_OFFSET;
	if (p.cut_q > QUALITY_MAX_Q) return QUALITY_CUT_Q;
	if (p.low_q > QUALITY_MAX_Q) return QUALITY_LOW_Q;
	if (p.max_low_pct > 100) return QUALITY_MAX_LOW_PCT;
	if (p.flags != 0) return QUALITY_FLAGS;
	if (p.reserved != 0) return QUALITY_RESERVED;
	return QUALITY_OK;
}

// the quality a byte says: 0 below the offset, 93 at most
constexpr uint32_t quality_of(uint32_t byte, uint32_t phred_offset)
{
	return byte < phred_offset ? 0 : (byte - phred_offset > QUALITY_MAX_Q ? QUALITY_MAX_Q : byte - phred_offset);
}

// e[q] = 10^6 * 10^(-q / 10) rounded to the nearest integer: the expected errors of a base of quality q, in millionths.  No entry is
// a tie: (2 t - 1)^10 10^q <= (2 10^6)^10 < (2 t + 1)^10 10^q holds for every entry t (the left half for t >= 1).
// (constexpr: the kernel calls it too)
constexpr uint32_t QUALITY_EE_PPM[QUALITY_MAX_Q + 1] = {
	1000000, 794328, 630957, 501187, 398107, 316228, 251189, 199526, 158489, 125893,
	100000, 79433, 63096, 50119, 39811, 31623, 25119, 19953, 15849, 12589,
	10000, 7943, 6310, 5012, 3981, 3162, 2512, 1995, 1585, 1259,
	1000, 794, 631, 501, 398, 316, 251, 200, 158, 126,
	100, 79, 63, 50, 40, 32, 25, 20, 16, 13,
	10, 8, 6, 5, 4, 3, 3, 2, 2, 1,
	1, 1, 1, 1, 0, 0, 0, 0, 0, 0,
	0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
	0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
	0, 0, 0, 0,
};

// a host stream of quality bytes: nreads reads in nbytes bytes, read i = bytes [offsets[i], offsets[i + 1]).  As check_stream, without
// pad: need_words is here the BYTES the stream takes.
inline StreamCheck check_byte_stream(const uint64_t *offsets, uint64_t nreads, uint64_t nbytes)
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
	s.need_words = nreads ? offsets[nreads] : 0;
	if (s.need_words > nbytes) s.fault = STREAM_TOO_SHORT;
	return s;
}

// The piece of a checked byte stream that starts at read r0, as next_piece with units of one read: the first read is always taken
// (so a read longer than piece_bytes is a piece of its own), further ones while the piece stays below piece_reads reads and within
// piece_bytes bytes.  The piece is staged as bytes [b0, b0 + nbytes) of the stream; b0 is the start of its first read rounded down to
// a multiple of 4, so that a read keeps its place within a 32-bit word, and the piece's offsets are rebased to b0.
struct BytePiece {
	uint64_t r1;                   // reads [r0, r1)
	uint64_t b0, nbytes;           // read i of the piece starts at byte offsets[r0 + i] - b0 of them; nbytes ends with the last read
};

inline BytePiece next_byte_piece(const uint64_t *offsets, uint64_t nreads, uint64_t r0, uint64_t piece_reads, uint64_t piece_bytes)
{
	uint64_t lo = 1, hi = piece_reads ? piece_reads : 1;
	if (hi > nreads - r0) hi = nreads - r0;
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1) / 2;
		if (offsets[r0 + mid] - offsets[r0] <= piece_bytes) lo = mid; else hi = mid - 1;
	}
	BytePiece p = {r0 + lo, offsets[r0] & ~3ULL, 0};
	p.nbytes = offsets[p.r1] - p.b0;
	return p;
}

// ---- the per-cycle QC report (sdt_qc.hip): what is refused before any launch, the layout of the report, and the grid ----
// (tools/qc_plan_check.cpp runs the check on every field and holds the layout to the table of include/sdt_gpu.h)
struct QcParams {                                        // == sdt_qc_params of include/sdt_gpu.h
	uint32_t cycles, phred_offset, flags, class_sel, reserved;
};
constexpr uint32_t QC_MAX_CYCLES = 4096;                 // SDT_QC_MAX_CYCLES
constexpr uint32_t QC_FROM_END = 1u;                     // SDT_QC_FROM_END
constexpr uint32_t QC_QUALS = QUALITY_MAX_Q + 1;         // the qualities a base can have: 0 .. 93
constexpr uint32_t QC_GC_BINS = 101;                     // 0 .. 100 percent
constexpr uint32_t QC_TOTALS = 8;

enum QcFault { QC_OK = 0, QC_CYCLES, QC_PHRED_OFFSET, QC_FLAGS, QC_CLASS_SEL, QC_RESERVED };

// the first field that is refused, in the order of the rules in include/sdt_gpu.h
inline QcFault check_qc_params(const QcParams &p)
{
	if (p.cycles == 0 || p.cycles > QC_MAX_CYCLES) return QC_CYCLES;
	if (p.phred_offset != 0 && p.phred_offset != 33 && p.phred_offset != 64) return QC_PHRED_OFFSET;
	if (p.flags & ~QC_FROM_END) return QC_FLAGS;
	if (p.class_sel > 255) return QC_CLASS_SEL;
	if (p.reserved != 0) return QC_RESERVED;
	return QC_OK;
}

// where the sections of the report start, in 64-bit words, for C cycles (R = C + 1 rows); words = 203 + 99 R
struct QcLayout {
	uint64_t rows, totals, base, qual, len, gc, meanq, words;
};
constexpr QcLayout qc_layout(uint32_t cycles)
{
	const uint64_t R = (uint64_t)cycles + 1;
	return QcLayout{R, 0, QC_TOTALS, QC_TOTALS + 4 * R, QC_TOTALS + 4 * R + QC_QUALS * R, QC_TOTALS + 4 * R + QC_QUALS * R + R,
	                QC_TOTALS + 4 * R + QC_QUALS * R + R + QC_GC_BINS, QC_TOTALS + 4 * R + QC_QUALS * R + R + QC_GC_BINS + QC_QUALS};
}
constexpr uint64_t qc_report_words(uint32_t cycles) { return cycles == 0 || cycles > QC_MAX_CYCLES ? 0 : qc_layout(cycles).words; }
static_assert(qc_layout(1).words == 203 + 99 * 2 && qc_layout(4096).words == 203 + 99 * 4097, "203 + 99 R");

// The QC kernel's workgroups: QC_WAVES wavefronts take a read each and stride over the rest, all of them counting into the one set
// of LDS histograms of their workgroup.  Every workgroup flushes its whole tile once per pass, so there are at most two per CU: the
// flush volume goes with the workgroups, not with the reads.  forced != 0 (SDT_WAVE_BLOCKS) puts that many in the place of the cap.
constexpr int QC_WAVES = 16;
// Rows of the LDS tile.  152 puts reads of 150 and 151 bases, the usual ones, through in ONE pass over the batch; the tile, len[4097], gc,
// meanq and row C are then 78 152 bytes of LDS, above the 64 KiB of the other kernels, and still two workgroups per CU (160 KiB).
constexpr int QC_TILE = 152;
constexpr uint32_t qc_blocks(uint64_t nreads, int cu_count, uint64_t forced)
{
	return wave_blocks(nreads, QC_WAVES, cu_count, forced ? forced : (uint64_t)(cu_count > 0 ? cu_count : 1) * 2);
}

} // namespace sdt
