"""The duplicate rule of include/sdt_gpu.h (sdt_gpu_dedup_reads) restated in plain Python: what the tests of the kernels, the ABI and
`sdt-kmers dedup` expect.  A class is an entry of a dictionary keyed on (kind, ((length, bases), ...)), the mates sorted under
SDT_DEDUP_MATE_SWAP; no fingerprint, no table, no rounds.  Nothing here touches the library under test.  Also the one case of
tests/test_read_dedup.py, built here so that the host tests can say that it holds what it promises."""
import functools

import numpy as np

from read_select_util import LETTERS, dense_units, ranged_units

DUP_FIELDS = ("first", "copies", "verdict")
DUP_DTYPE = np.dtype([("first", np.uint64), ("copies", np.uint32), ("verdict", np.uint32)])
KEPT, DROPPED = 0, 1
MATE_SWAP = 1
# the word, chunk and wavefront-pass boundaries of a fingerprint that takes 32 bases per lane; 5 000 is past every pass-1 limit
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 5000)


def read_key(read):
    read = np.asarray(read, dtype=np.uint8)
    return (len(read), read.tobytes())


def unit_key(reads, swap):
    keys = [read_key(r) for r in reads]
    if swap and len(keys) == 2:
        keys.sort()
    return (len(keys), tuple(keys))


def classes_of(reads, units, swap):
    """reads: {record index: bases}; units: [(id, [record indices])] -> {key: [unit ids, ascending]}"""
    classes = {}
    for u, members in sorted(units):
        if members:
            classes.setdefault(unit_key([reads[i] for i in members], swap), []).append(u)
    return classes


def expect_dedup(codes, offs, paired=False, flags=0, units=None, ordinals=None):
    """-> (dup records as a structured array, keep uint8[], reads kept).  units: dense by `paired` unless given (then in terms of the
    record index, which is ordinals[r] for read r when ordinals is given -- without units every read is then a unit of its own; the
    array has max ordinal + 1 records and the records that no read has are zero)"""
    assert flags in (0, MATE_SWAP)
    n = len(offs) - 1
    idx = list(range(n)) if ordinals is None else [int(o) for o in ordinals]
    reads = {idx[r]: codes[int(offs[r]):int(offs[r + 1])] for r in range(n)}
    if units is None:
        units = dense_units(n, paired) if ordinals is None else [(o, [o]) for o in idx]
    members_of = dict(units)
    size = (max(idx) + 1) if idx else 0
    dup = np.zeros(size, dtype=DUP_DTYPE)
    keep = np.zeros(size, dtype=np.uint8)
    for ids in classes_of(reads, units, bool(flags & MATE_SWAP)).values():
        for u in ids:
            for i in members_of[u]:
                dup[i] = (ids[0], min(len(ids), 0xFFFFFFFF), KEPT if u == ids[0] else DROPPED)
                keep[i] = u == ids[0]
    return dup, keep, int(keep.sum())


def brute_force(reads, units, swap):
    """every unit against every earlier one, base by base -> {unit id: (first, copies, verdict)}"""
    def same_read(a, b):
        return len(a) == len(b) and all(int(x) == int(y) for x, y in zip(a, b))

    def same_unit(a, b):
        if len(a) != len(b):
            return False
        if all(same_read(x, y) for x, y in zip(a, b)):
            return True
        return swap and len(a) == 2 and same_read(a[0], b[1]) and same_read(a[1], b[0])

    units = sorted((u, [reads[i] for i in m]) for u, m in units if m)
    first = {}
    for k, (u, mine) in enumerate(units):
        first[u] = next((first[v] for v, theirs in units[:k] if same_unit(mine, theirs)), u)
    sizes = {}
    for u, f in first.items():
        sizes[f] = sizes.get(f, 0) + 1
    return {u: (f, sizes[f], KEPT if f == u else DROPPED) for u, f in first.items()}


def assert_dup_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == DUP_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in DUP_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def concat(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if reads else np.zeros(0, dtype=np.uint8)
    return codes.astype(np.uint8), offs


def levels_of(dup, units):
    """the duplication levels of records by record index: [(copies, classes, reads)] ascending"""
    levels = {}
    for u, members in units:
        if not members:
            continue
        first, copies, verdict = (int(x) for x in dup[members[0]])
        lv = levels.setdefault(copies, [0, 0])
        lv[0] += verdict == KEPT
        lv[1] += len(members)
    return [(c, a, b) for c, (a, b) in sorted(levels.items())]


def cli_texts(codes, offs, dup, keep, pair_ranges):
    """the four files of `sdt-kmers dedup` for a stream in ordinal order: (readDup, pairs.fa, single.fa, dupLevels)"""
    n = len(offs) - 1
    in_pair = set()
    for first, end in pair_ranges:
        in_pair.update(range(first, end))
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    dup_txt = "".join(f"{a} {b} {c}\n" for a, b, c in dup.tolist())
    pairs, single = [], []
    for r in range(n):
        if keep[r]:
            (pairs if r in in_pair else single).append(f">{r + 1}\n{letters[int(offs[r]):int(offs[r + 1])]}\n")
    lev_txt = "".join(f"{c} {a} {b}\n" for c, a, b in levels_of(dup, ranged_units(range(n), pair_ranges)))
    return dup_txt, "".join(pairs), "".join(single), lev_txt


# ---- the case of tests/test_read_dedup.py ---------------------------------------------------------------------------------------------
COPIES = (1, 2, 3, 7)


@functools.lru_cache(maxsize=None)
def case(seed=20240917):
    """34 base sequences of the lengths above, each present 1, 2, 3 or 7 times; near misses of three of them (the last base, the first
    base, one base more, one base fewer, and base 32 of a 65-base read); a second read of length 0; filler reads of 1 .. 15 bases, so
    that copies start at every base of a word; shuffled by a fixed seed.  Built once per seed and left unchanged (another seed: another
    draw of the same generator, for the tests that need more reads)."""
    rng = np.random.default_rng(seed)
    seqs = []
    for L in LENGTHS:
        per = 1 if L in (0, 5000) else 3 if 31 <= L <= 65 else 2
        if L == 1:
            seqs += [np.array([1], dtype=np.uint8), np.array([2], dtype=np.uint8)]
        else:
            seqs += [rng.integers(0, 4, size=L, dtype=np.uint8) for _ in range(per)]
    reads, origin = [], []                                # origin: ("seq", i) | ("twin", i, what) | ("filler", L)
    for i, s in enumerate(seqs):
        c = 2 if len(s) == 0 else COPIES[i % 4]           # (two reads of length 0)
        reads += [s.copy() for _ in range(c)]
        origin += [("seq", i)] * c
    twins_of = [next(i for i, s in enumerate(seqs) if len(s) == L) for L in (17, 65, 2048)]
    for i in twins_of:
        s = seqs[i]
        last, first = s.copy(), s.copy()
        last[-1] ^= 1
        first[0] ^= 2
        more = np.concatenate([s, [s[-1]]]).astype(np.uint8)
        for what, t in (("last", last), ("first", first), ("plus", more), ("minus", s[:-1].copy())):
            reads.append(t)
            origin.append(("twin", i, what))
        if len(s) == 65:
            mid = s.copy()
            mid[32] ^= 3
            reads.append(mid)
            origin.append(("twin", i, "base 32"))
    for L in range(1, 16):
        reads.append(rng.integers(0, 4, size=L, dtype=np.uint8) if L > 1 else np.array([3], dtype=np.uint8))
        origin.append(("filler", L))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    origin = [origin[i] for i in order]
    if len(reads) & 1:                                    # (the paired run needs whole pairs)
        reads.append(seqs[twins_of[0]][:-1].copy())
        origin.append(("twin", twins_of[0], "minus"))
    codes, offs = concat(reads)
    return dict(reads=reads, origin=origin, codes=codes, offs=offs, nseqs=len(seqs))


@functools.lru_cache(maxsize=None)
def paired_case(seed=20240918):
    """pairs: (a, b) three times, (b, a), (a, c), (a, a); (p, q) seven times and (q, p) twice; a pair of two empty reads twice; the
    5 000-base read with a 2 049-base mate twice, and once with the mate one base shorter; and the first reads of case() two by
    two.  The pairs are shuffled by a fixed seed."""
    c = case() if seed == 20240918 else case(seed - 1)
    rng = np.random.default_rng(seed)
    by_len = {}
    for r in c["reads"]:
        by_len.setdefault(len(r), r)
    a, b, cc = (rng.integers(0, 4, size=L, dtype=np.uint8) for L in (33, 64, 64))
    p, q = by_len[65], by_len[31]
    empty = np.zeros(0, dtype=np.uint8)
    pairs = [(a, b)] * 3 + [(b, a), (a, cc), (a, a)] + [(p, q)] * 7 + [(q, p)] * 2 + [(empty, empty)] * 2
    pairs += [(by_len[5000], by_len[2049])] * 2 + [(by_len[5000], by_len[2049][:-1])]
    pairs += [(c["reads"][2 * t], c["reads"][2 * t + 1]) for t in range(20)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    codes, offs = concat([r for pr in pairs for r in pr])
    return dict(pairs=pairs, codes=codes, offs=offs, a=a, b=b, c=cc)
