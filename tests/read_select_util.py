"""The normalisation rule of include/sdt_gpu.h (sdt_gpu_select_reads) and the compaction of a 2-bit stream (sdt_gpu_compact_reads)
restated in plain Python: what the tests of the kernels, the ABI and `sdt-kmers normalize` expect.  A table is a function canonical
k-mer (an integer) -> count; Python integers make the 128-bit comparison exact.  Nothing here touches the library under test."""
import numpy as np

from test_kmer_search import canon_kmers

PICK_FIELDS = ("kmers", "median", "cov", "verdict")
KEPT, KEPT_DRAW, DROPPED_DRAW, ABERRANT, SHORT = range(5)
OWN_ABERRANT = 1 << 4
SAT = 65535
M64 = (1 << 64) - 1
LETTERS = "ACTG"


def mix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def draw(u, seed):
    return mix64((seed ^ ((u * 0x9E3779B97F4A7C15) & M64)) & M64) >> 32


def read_stats(counts, max_cv_pct):
    """the counts of a read's k-mers -> (n, median, aberrant)"""
    n = len(counts)
    if n == 0:
        return 0, 0, False
    median = sorted(counts)[(n - 1) // 2]
    sat = [min(c, SAT) for c in counts]
    s1 = sum(sat)
    s2 = sum(c * c for c in sat)
    aberrant = max_cv_pct > 0 and 10000 * (n * s2 - s1 * s1) > max_cv_pct * max_cv_pct * s1 * s1
    return n, median, aberrant


def decide_unit(stats, u, target, seed):
    """stats: the (n, median, aberrant) of the unit's reads (one or two) -> (cov, class)"""
    assert target > 0
    with_kmers = [s for s in stats if s[0] > 0]
    if not with_kmers:
        return 0, SHORT
    cov = with_kmers[0][1] if len(with_kmers) == 1 else (with_kmers[0][1] + with_kmers[1][1] + 1) // 2
    if any(s[2] for s in with_kmers):
        return cov, ABERRANT
    if cov <= target:
        return cov, KEPT
    return cov, KEPT_DRAW if draw(u, seed) * cov < target << 32 else DROPPED_DRAW


def select_units(per_read, units, target, seed):
    """per_read: {record index: (n, median, aberrant)}; units: [(id, [record indices])] -> {record index: (kmers, median, cov, verdict)}"""
    out = {}
    for u, members in units:
        cov, cls = decide_unit([per_read[i] for i in members], u, target, seed)
        for i in members:
            n, median, ab = per_read[i]
            out[i] = (n, median, cov, cls | (OWN_ABERRANT if ab and n > 0 else 0))
    return out


def read_kmer_counts(codes, offs, K, count):
    return [[count(k) for k in canon_kmers(codes[int(offs[r]):int(offs[r + 1])], K)] for r in range(len(offs) - 1)]


def dense_units(n, paired):
    if not paired:
        return [(i, [i]) for i in range(n)]
    assert n % 2 == 0
    return [(i, [i, i + 1]) for i in range(0, n, 2)]


def ranged_units(present, pair_ranges):
    """the kept form: present = the ordinals that have a read, pair_ranges = [(first, end)]; a unit's id is its first mate's ordinal
    whether or not that mate is there"""
    present = sorted(present)
    have = set(present)
    in_pair = {}
    for first, end in pair_ranges:
        assert (end - first) % 2 == 0
        for o in range(first, end):
            in_pair[o] = first + ((o - first) & ~1)
    units, seen = [], set()
    for o in present:
        u = in_pair.get(o, o)
        if u in seen:
            continue
        seen.add(u)
        members = [x for x in ((u, u + 1) if o in in_pair else (u,)) if x in have]
        units.append((u, members))
    return units


def expect_select(codes, offs, K, count, target, max_cv_pct, seed, paired=False, kmer_counts=None, units=None, ordinals=None):
    """-> (pick records as a structured array, keep uint8[], reads kept).  units: dense by `paired` unless given (then in terms of
    the record index, which is ordinals[r] for read r when ordinals is given; the array then has max ordinal + 1 records)"""
    n = len(offs) - 1
    kc = kmer_counts if kmer_counts is not None else read_kmer_counts(codes, offs, K, count)
    idx = list(range(n)) if ordinals is None else [int(o) for o in ordinals]
    per_read = {idx[r]: read_stats(kc[r], max_cv_pct) for r in range(n)}
    if units is None:
        units = dense_units(n, paired)
    got = select_units(per_read, units, target, seed)
    size = (max(idx) + 1) if idx else 0
    pick = np.zeros(size, dtype=[(f, np.uint32) for f in PICK_FIELDS])
    keep = np.zeros(size, dtype=np.uint8)
    for i, rec in got.items():
        pick[i] = rec
        keep[i] = (rec[3] & 7) <= KEPT_DRAW
    return pick, keep, int(keep.sum())


def assert_pick_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == PICK_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in PICK_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


# ---- compaction ---------------------------------------------------------------------------------------------------------------------
def pack_words(codes, pad=4):
    """2 bits per base, 16 bases per word, first base in the most significant pair; `pad` zero words follow"""
    nw = (len(codes) + 15) // 16
    full = np.zeros(nw * 16, dtype=np.uint32)
    full[: len(codes)] = codes
    shifts = (30 - 2 * np.arange(16)).astype(np.uint32)
    words = (full.reshape(nw, 16) << shifts).sum(axis=1, dtype=np.uint64).astype(np.uint32) if nw else np.zeros(0, dtype=np.uint32)
    return np.concatenate([words, np.zeros(pad, dtype=np.uint32)])


def base_at(words, g):
    return (int(words[g >> 4]) >> (30 - 2 * (g & 15))) & 3


def expect_compact(words, offs, keep):
    """the compaction as the kernel sees it: for every output word the 16 bases it holds, each found through the new offsets
    -> (out_words with 4 pad words, out_offsets)"""
    n = len(offs) - 1
    kept = [r for r in range(n) if keep[r]]
    out_offs = np.zeros(len(kept) + 1, dtype=np.uint64)
    out_offs[1:] = np.cumsum([int(offs[r + 1]) - int(offs[r]) for r in kept])
    total = int(out_offs[-1])
    src = np.zeros(total, dtype=np.int64)                 # where every output base comes from
    for k, r in enumerate(kept):
        a, b = int(out_offs[k]), int(out_offs[k + 1])
        src[a:b] = np.arange(int(offs[r]), int(offs[r + 1]))
    nw = (total + 15) // 16
    out = np.zeros(nw + 4, dtype=np.uint32)
    for w in range(nw):
        v = 0
        for i in range(16):
            g = 16 * w + i
            v = (v << 2) | (base_at(words, int(src[g])) if g < total else 0)
        out[w] = v
    return out, out_offs


def compact_by_bases(words, offs, keep):
    """the per-base reference: unpack to a list of base lists, filter, repack"""
    reads = [[base_at(words, g) for g in range(int(offs[r]), int(offs[r + 1]))] for r in range(len(offs) - 1)]
    kept = [rd for rd, k in zip(reads, keep) if k]
    out_offs = np.zeros(len(kept) + 1, dtype=np.uint64)
    out_offs[1:] = np.cumsum([len(rd) for rd in kept])
    flat = np.array([b for rd in kept for b in rd], dtype=np.uint8)
    return pack_words(flat), out_offs


def cli_texts(codes, offs, pick, keep, pair_ranges):
    """the three files of `sdt-kmers normalize` and its tally for a stream in ordinal order: (readPick, pairs.fa, single.fa,
    (kept, reads, short, aberrant, drawn))"""
    n = len(offs) - 1
    in_pair = set()
    for first, end in pair_ranges:
        in_pair.update(range(first, end))
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    pick_txt = "".join(f"{a} {b} {c} {d}\n" for a, b, c, d in pick.tolist())
    pairs, single = [], []
    for r in range(n):
        if keep[r]:
            (pairs if r in in_pair else single).append(f">{r + 1}\n{letters[int(offs[r]):int(offs[r + 1])]}\n")
    cls = pick["verdict"] & 7
    tally = (int(keep.sum()), n, int((cls == SHORT).sum()), int((cls == ABERRANT).sum()), int((cls == DROPPED_DRAW).sum()))
    return pick_txt, "".join(pairs), "".join(single), tally
