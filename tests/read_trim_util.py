"""The trimming rule of include/sdt_gpu.h (sdt_gpu_trim_reads) and the compaction of a 2-bit stream to a range per read
(sdt_gpu_compact_trimmed) restated in plain Python: what the tests of the kernels, the ABI and `sdt-kmers trim` expect.  A table is a
function canonical k-mer (an integer) -> count.  The SDT_TRIM_CORRECTED flag composes with the restated correction rule of
read_correct_util.  Nothing here touches the library under test."""
import numpy as np

from test_kmer_search import canon_kmers
from read_correct_util import candidate_base, correct_read, runs_of
from read_select_util import LETTERS, base_at, pack_words, read_kmer_counts  # noqa: F401  (re-exported for the tests)

TRIM_FIELDS = ("kmers", "weak", "median", "start", "len", "verdict")
TRIM_DTYPE = np.dtype([(f, np.uint32) for f in TRIM_FIELDS])
WHOLE, GATED, TRIMMED, DROPPED, SHORT = range(5)
CORRECTED = 1
TOO_LONG = 0xFFFFFFFF


def weak_mask(codes, K, count, min_count, flags, c):
    """the weak k-mers that are left: c[j] < min_count, and under the flag the runs that the correction would fix cleared"""
    weak = [x < min_count for x in c]
    if flags & CORRECTED and any(weak):
        _, subs = correct_read(codes, K, count, min_count, c)
        fixed_at = {p for p, _ in subs}
        n = len(c)
        for a, b in runs_of(weak):
            if candidate_base(a, b, n, K) in fixed_at:    # (a candidate's base belongs to its run alone)
                for j in range(a, b + 1):
                    weak[j] = False
    return weak


def stretches(weak):
    """maximal runs of solid k-mers as (a, s)"""
    return [(a, b - a + 1) for a, b in runs_of([not w for w in weak])]


def trim_read(codes, K, count, params, kmer_counts=None):
    """codes: uint8 bases of one read; params = (min_count, min_cov, min_len, flags) -> (kmers, weak, median, start, len, verdict)"""
    min_count, min_cov, min_len, flags = params
    assert flags & ~CORRECTED == 0
    L = len(codes)
    n = L - K + 1
    if n <= 0:
        return (0, 0, 0, 0, 0, SHORT)
    c = kmer_counts if kmer_counts is not None else [count(k) for k in canon_kmers(codes, K)]
    assert len(c) == n
    nweak = sum(x < min_count for x in c)
    median = sorted(c)[(n - 1) // 2]
    weak = weak_mask(codes, K, count, min_count, flags, c)
    if not any(weak):
        return (n, nweak, median, 0, L, WHOLE)
    if min_cov > 0 and median < min_cov:
        return (n, nweak, median, 0, L, GATED)
    best = None
    for a, s in stretches(weak):
        if best is None or s > best[1]:                  # (strictly longer: the first among equals stays)
            best = (a, s)
    if best is None or best[1] + K - 1 < min_len:
        return (n, nweak, median, 0, 0, DROPPED)
    return (n, nweak, median, best[0], best[1] + K - 1, TRIMMED)


def expect_trim(codes, offs, K, count, params, kmer_counts=None, max_read_len=None):
    """-> (trim records as a structured array, keep uint8[], reads with len > 0).  max_read_len: the device form's promise; a longer
    read is marked and nothing else"""
    n = len(offs) - 1
    trim = np.zeros(n, dtype=TRIM_DTYPE)
    for r in range(n):
        s, e = int(offs[r]), int(offs[r + 1])
        if max_read_len is not None and e - s >= K and e - s > max(max_read_len, K):
            trim[r] = (TOO_LONG, 0, 0, 0, 0, SHORT)
            continue
        trim[r] = trim_read(codes[s:e], K, count, params, None if kmer_counts is None else kmer_counts[r])
    keep = (trim["len"] > 0).astype(np.uint8)
    return trim, keep, int(keep.sum())


def assert_trim_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == TRIM_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in TRIM_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


# ---- compaction of ranges -----------------------------------------------------------------------------------------------------------
def clamp_ranges(offs, trim):
    """(start, len) of every read as the device form's placement kernel clamps them to the read"""
    out = []
    for r in range(len(offs) - 1):
        L = int(offs[r + 1]) - int(offs[r])
        s = min(int(trim["start"][r]), L)
        out.append((s, min(int(trim["len"][r]), L - s)))
    return out


def expect_compact_trimmed(words, offs, trim):
    """the compaction as the kernel sees it: for every output word the 16 bases it holds, each found through the new offsets and the
    start of its read's range -> (out_words with 4 pad words, out_offsets)"""
    rng = clamp_ranges(offs, trim)
    kept = [r for r in range(len(offs) - 1) if rng[r][1] > 0]
    out_offs = np.zeros(len(kept) + 1, dtype=np.uint64)
    out_offs[1:] = np.cumsum([rng[r][1] for r in kept])
    total = int(out_offs[-1])
    src = np.zeros(total, dtype=np.int64)                 # where every output base comes from
    for k, r in enumerate(kept):
        a, b = int(out_offs[k]), int(out_offs[k + 1])
        src[a:b] = int(offs[r]) + rng[r][0] + np.arange(b - a)
    nw = (total + 15) // 16
    out = np.zeros(nw + 4, dtype=np.uint32)
    for w in range(nw):
        v = 0
        for i in range(16):
            g = 16 * w + i
            v = (v << 2) | (base_at(words, int(src[g])) if g < total else 0)
        out[w] = v
    return out, out_offs


def compact_trimmed_by_bases(words, offs, trim):
    """the per-base reference: unpack to a list of base lists, slice, drop the empty, repack"""
    reads = [[base_at(words, g) for g in range(int(offs[r]), int(offs[r + 1]))] for r in range(len(offs) - 1)]
    kept = [rd[int(t["start"]):int(t["start"]) + int(t["len"])] for rd, t in zip(reads, trim)]
    kept = [rd for rd in kept if rd]
    out_offs = np.zeros(len(kept) + 1, dtype=np.uint64)
    out_offs[1:] = np.cumsum([len(rd) for rd in kept])
    flat = np.array([b for rd in kept for b in rd], dtype=np.uint8)
    return pack_words(flat), out_offs


def trimmed_reads(codes, offs, trim):
    """the kept part of every read with len > 0, as code arrays"""
    return [codes[int(offs[r]) + int(trim["start"][r]):int(offs[r]) + int(trim["start"][r]) + int(trim["len"][r])]
            for r in range(len(offs) - 1) if trim["len"][r] > 0]


def cli_texts(codes, offs, trim, pair_ranges):
    """the files of `sdt-kmers trim` and its tally line for a stream in ordinal order; codes: the bases that are written (the corrected
    ones under --correct) -> (readTrim, pairs.fa, single.fa, tally)"""
    n = len(offs) - 1
    mate = {}
    for first, end in pair_ranges:
        for o in range(first, end):
            mate[o] = first + ((o - first) ^ 1)
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    trim_txt = "".join("%d %d %d %d %d %d\n" % tuple(t) for t in trim.tolist())
    pairs, single = [], []
    for r in range(n):
        ln = int(trim["len"][r])
        if not ln:
            continue
        s = int(offs[r]) + int(trim["start"][r])
        both = r in mate and mate[r] < n and trim["len"][mate[r]] > 0
        (pairs if both else single).append(f">{r + 1}\n{letters[s:s + ln]}\n")
    v = trim["verdict"]
    tally = "%d reads: %d whole, %d gated, %d trimmed, %d dropped, %d short; %d bases in, %d bases out\n" % (
        n, (v == WHOLE).sum(), (v == GATED).sum(), (v == TRIMMED).sum(), (v == DROPPED).sum(), (v == SHORT).sum(),
        int(offs[-1]) - int(offs[0]), int(trim["len"].sum()))
    return trim_txt, "".join(pairs), "".join(single), tally
