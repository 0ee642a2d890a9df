"""The mate-overlap rule of include/sdt_gpu.h (sdt_gpu_overlap_pairs) restated in plain Python: what the tests of the kernel, the ABI
and `sdt-kmers overlap` expect.  Shifts are walked one by one and the columns of a shift compared base by base as numpy arrays; no
windows, no bit tricks, no early exit.  Nothing here touches the library under test.  Also the one case of tests/test_read_overlap.py
and the 600 pairs over two letters, built here so that the host tests can say that they hold what they promise."""
import functools

import numpy as np

from read_dedup_util import concat
from read_select_util import LETTERS

OVERLAP_FIELDS = ("overlap", "mismatches", "insert", "start", "len", "verdict")
OVERLAP_DTYPE = np.dtype([(f, np.uint32) for f in OVERLAP_FIELDS])
WHOLE, CLIPPED, DROPPED = 0, 2, 3
A, C, T, G = range(4)
PARAM_FIELDS = ("min_overlap", "max_err_pct", "min_len", "flags")
# the defaults of `sdt-kmers overlap`
DEFAULTS = dict(min_overlap=30, max_err_pct=10, min_len=0, flags=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS)
    return p


def revcomp(b):
    """the complement of code x is x ^ 2"""
    return (np.asarray(b, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def shift_stats(a, b, d):
    """(o, h) of the shift d: the columns, and those of them that differ"""
    La, Lb = len(a), len(b)
    bp = revcomp(b)
    lo, hi = max(0, d), min(La, d + Lb)
    if hi <= lo:
        return 0, 0
    return hi - lo, int((np.asarray(a)[lo:hi] != bp[lo - d:hi - d]).sum())


def pair_overlap(a, b, min_overlap, pct):
    """the pair's overlap -> (o, h, F), or (0, 0, 0) when no shift is admissible"""
    a = np.asarray(a, dtype=np.uint8)
    b = np.asarray(b, dtype=np.uint8)
    La, Lb = len(a), len(b)
    bp = revcomp(b)
    best = None
    for d in range(-Lb + 1, La):
        lo, hi = max(0, d), min(La, d + Lb)
        o = hi - lo
        if o < min_overlap:
            continue
        h = int((a[lo:hi] != bp[lo - d:hi - d]).sum())
        if 100 * h <= pct * o:
            key = (o - 3 * h, d + Lb)                     # the greatest score, the greatest insert among equals
            if best is None or key > best[0]:
                best = (key, o, h)
    return (best[1], best[2], best[0][1]) if best else (0, 0, 0)


def read_record(L, found, min_len):
    """a read of L bases in a pair whose overlap is found = (o, h, F) -> (overlap, mismatches, insert, start, len, verdict)"""
    o, h, F = found
    ln = min(L, F) if F else L
    if ln < max(min_len, 1):
        return (o, h, F, 0, 0, DROPPED)
    return (o, h, F, 0, ln, WHOLE if ln == L else CLIPPED)


def expect_overlap(codes, offs, p, pair_ranges=None, ordinals=None):
    """-> (records, keep uint8[], reads with len > 0).  Dense (pair_ranges None): reads 2t and 2t + 1 are mates.  With ordinals: record
    ordinals[r] is read r's, the others are zero; the pairs are the ordinals first + 2t, first + 2t + 1 of a range that both have a
    read, every other read is single"""
    n = len(offs) - 1
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(n)]
    idx = list(range(n)) if ordinals is None else [int(o) for o in ordinals]
    if pair_ranges is None:
        assert n % 2 == 0 and ordinals is None
        pair_ranges = [(0, n)]
    size = (max(idx) + 1) if idx else 0
    at = {o: r for r, o in enumerate(idx)}
    mate = {}
    for first, end in pair_ranges:
        for o in range(int(first), int(end), 2):
            if o in at and o + 1 in at:
                mate[o] = o + 1
    ov = np.zeros(size, dtype=OVERLAP_DTYPE)
    second = set(mate.values())
    for o, r in at.items():
        if o in second:
            continue
        if o in mate:
            a, b = reads[r], reads[at[o + 1]]
            found = pair_overlap(a, b, p["min_overlap"], p["max_err_pct"])
            ov[o] = read_record(len(a), found, p["min_len"])
            ov[o + 1] = read_record(len(b), found, p["min_len"])
        else:
            ov[o] = read_record(len(reads[r]), (0, 0, 0), p["min_len"])
    keep = (ov["len"] > 0).astype(np.uint8)
    return ov, keep, int(keep.sum())


def cut_reads(codes, offs, ov):
    """the reads that compact_trimmed makes of the records"""
    return [codes[int(offs[r]) + int(c["start"]):int(offs[r]) + int(c["start"]) + int(c["len"])] for r, c in enumerate(ov) if c["len"]]


def assert_overlap_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == OVERLAP_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in OVERLAP_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


# ---- `sdt-kmers overlap` ------------------------------------------------------------------------------------------------------------
def cli_texts(codes, offs, ov, pair_ranges):
    """the four files of `sdt-kmers overlap` for a stream in ordinal order: (readOverlap, pairs.fa, single.fa, insertHist).  A pair
    counts as clipped when its overlap cut bases from a mate: its insert is shorter than that mate"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    rec_txt = "".join(" ".join(str(int(c[f])) for f in OVERLAP_FIELDS) + "\n" for c in ov)
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if ov["len"][r]:
            s = int(offs[r]) + int(ov["start"][r])
            both = r in mate and ov["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{letters[s:s + int(ov['len'][r])]}\n")
    inserts, npairs, clipped = [], 0, 0
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            npairs += 1
            F = int(ov["insert"][r])
            if F:
                inserts.append(F)
                clipped += any(F < int(offs[m + 1]) - int(offs[m]) for m in (r, r + 1))
    inserts.sort()
    hist = "".join(f"{F} {inserts.count(F)}\n" for F in sorted(set(inserts)))
    median = inserts[(len(inserts) - 1) // 2] if inserts else 0
    hist += f"# pairs {npairs} overlapping {len(inserts)} clipped {clipped} median {median}\n"
    return rec_txt, "".join(pairs), "".join(single), hist


# ---- 600 pairs over two letters -------------------------------------------------------------------------------------------------------
AT_PARAMS = params(min_overlap=6, max_err_pct=15)


@functools.lru_cache(maxsize=None)
def at_pairs():
    """600 random pairs over A and T (closed under complement, so overlaps and ties abound), every mate of 0 .. 90 bases: built once
    from a fixed seed and left unchanged -> (reads, codes, offs)"""
    rng = np.random.default_rng(20241019)
    reads = [(rng.integers(0, 2, size=int(rng.integers(0, 91)), dtype=np.uint8) * 2).astype(np.uint8) for _ in range(1200)]
    codes, offs = concat(reads)
    return reads, codes, offs


@functools.lru_cache(maxsize=None)
def at_expect():
    """the records of the 600 pairs under AT_PARAMS, by the rule: computed once, shared by the tests, left unchanged"""
    _, codes, offs = at_pairs()
    return expect_overlap(codes, offs, AT_PARAMS)


# ---- the case of tests/test_read_overlap.py -------------------------------------------------------------------------------------------
CASE_PARAMS = params(min_overlap=30, max_err_pct=10, min_len=40)


def _mutate(a, where):
    a = np.array(a, dtype=np.uint8)
    for k in where:
        a[k] = (a[k] + 1) & 3
    return a


@functools.lru_cache(maxsize=None)
def case(seed=20241020):
    """Pairs with planted fragments, each under a name that says what it is there for; built once per seed and left unchanged
    (another seed: another draw of the same generator).  `pairs` holds (a, b) per name in the order of `names`; reads, codes and offs
    are the interleaved stream."""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *parts: np.concatenate([np.asarray(x, dtype=np.uint8) for x in parts]).astype(np.uint8)

    def planted(F, La, Lb):
        """a fragment of F bases read from both ends, La and Lb bases deep, with different random adapters past the fragment's end"""
        frag = rnd(F)
        a = cat(frag, rnd(La - F)) if La > F else frag[:La]
        b = cat(revcomp(frag), rnd(Lb - F)) if Lb > F else revcomp(frag)[:Lb]
        return a, b

    named = [
        ("fragment 100 in 150", planted(100, 150, 150)),
        ("fragment 220 in 150", planted(220, 150, 150)),
        ("fragment of exactly L", planted(150, 150, 150)),
        ("long a, short b inside it", planted(90, 150, 60)),            # b' lies at d = 30 of a: only a is clipped
        ("short a, long b", planted(90, 60, 150)),                      # only b is clipped
        ("unequal, both whole", planted(200, 150, 100)),
    ]
    frag = rnd(100)
    where = [3, 11, 19, 31, 32, 33, 47, 63, 64, 80, 99]                  # 10 of 100 columns: 1000 <= 1000; 11: not
    named.append(("mismatches on budget", (frag, _mutate(revcomp(frag), where[:10]))))
    frag = rnd(100)
    named.append(("mismatches over budget", (frag, _mutate(revcomp(frag), where))))
    for o in (31, 32, 33, 64, 65):
        named.append((f"overlap of {o}", planted(200 - o, 100, 100)))
    named.append(("third step", planted(190, 150, 150)))                # d = 40 = d_first + 160
    named.append(("2500 bases", planted(2000, 2500, 2500)))
    a = rnd(100)
    named.append(("mate shorter than min_overlap", (a, revcomp(a)[:29])))
    named.append(("mate of 0 bases", (rnd(80), np.zeros(0, dtype=np.uint8))))
    named.append(("both of 0 bases", (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))))
    named.append(("unrelated", (rnd(150), rnd(150))))
    named.append(("min_len drops b only", planted(50, 150, 32)))         # insert 50, overlap 32: a keeps 50 bases, b has 32 < min_len
    at = np.tile(np.array([A, T], dtype=np.uint8), 30)
    named.append(("A/T tie", (at, revcomp(np.roll(at, 1)))))             # b' = TATA...: d = 0 mismatches everywhere, d = -1 and d = +1 tie
    while len(named) < 40:                                               # pairs of the transcript alone
        La, Lb = int(rng.integers(40, 160)), int(rng.integers(40, 160))
        named.append(("plain", (rnd(La), rnd(Lb))))
    order = rng.permutation(len(named))
    named = [named[i] for i in order]
    names = [n for n, _ in named]
    pairs = [p for _, p in named]
    reads = [r for p in pairs for r in p]
    codes, offs = concat(reads)
    return dict(names=names, pairs=pairs, reads=reads, codes=codes, offs=offs, params=CASE_PARAMS)


@functools.lru_cache(maxsize=None)
def case_expect(min_overlap=None, max_err_pct=None):
    """the records of the case under its own parameters (or under another min_overlap and percentage), by the rule: computed once per
    parameter set, shared by the tests, left unchanged"""
    c = case()
    p = dict(c["params"])
    if min_overlap is not None:
        p.update(min_overlap=min_overlap, max_err_pct=max_err_pct)
    return expect_overlap(c["codes"], c["offs"], p)


def case_holds():
    """the case contains what its names promise, by the rule: -> the number of checks made"""
    c = case()
    ov = case_expect()[0]
    at = {n: i for i, n in enumerate(c["names"]) if n != "plain"}
    rec = lambda n, m: tuple(int(x) for x in ov[2 * at[n] + m].tolist())
    both = lambda n: (rec(n, 0), rec(n, 1))
    ml = c["params"]["min_len"]
    ta, tb = c["pairs"][at["A/T tie"]]
    checks = [
        both("fragment 100 in 150") == ((100, 0, 100, 0, 100, CLIPPED),) * 2,
        both("fragment 220 in 150") == ((80, 0, 220, 0, 150, WHOLE),) * 2,
        both("fragment of exactly L") == ((150, 0, 150, 0, 150, WHOLE),) * 2,
        both("long a, short b inside it") == ((60, 0, 90, 0, 90, CLIPPED), (60, 0, 90, 0, 60, WHOLE)),
        both("short a, long b") == ((60, 0, 90, 0, 60, WHOLE), (60, 0, 90, 0, 90, CLIPPED)),
        both("unequal, both whole") == ((50, 0, 200, 0, 150, WHOLE), (50, 0, 200, 0, 100, WHOLE)),
        both("mismatches on budget") == ((100, 10, 100, 0, 100, WHOLE),) * 2,
        both("mismatches over budget") == ((0, 0, 0, 0, 100, WHOLE),) * 2,
        shift_stats(*c["pairs"][at["mismatches over budget"]], 0) == (100, 11),
    ]
    checks += [both(f"overlap of {o}") == ((o, 0, 200 - o, 0, 100, WHOLE),) * 2 for o in (31, 32, 33, 64, 65)]
    checks += [
        both("third step") == ((110, 0, 190, 0, 150, WHOLE),) * 2,
        2 * 64 <= 190 - 150 - (c["params"]["min_overlap"] - 150) < 3 * 64,      # d - d_first lies in the third step of 64 shifts
        both("2500 bases") == ((2000, 0, 2000, 0, 2000, CLIPPED),) * 2,
        both("mate shorter than min_overlap") == ((0, 0, 0, 0, 100, WHOLE), (0, 0, 0, 0, 0, DROPPED)),
        both("mate of 0 bases") == ((0, 0, 0, 0, 80, WHOLE), (0, 0, 0, 0, 0, DROPPED)),
        both("both of 0 bases") == ((0, 0, 0, 0, 0, DROPPED),) * 2,
        both("unrelated") == ((0, 0, 0, 0, 150, WHOLE),) * 2,
        both("min_len drops b only") == ((32, 0, 50, 0, 50, CLIPPED), (32, 0, 50, 0, 0, DROPPED)) and ml == 40,
        both("A/T tie") == ((59, 0, 61, 0, 60, WHOLE),) * 2,
        shift_stats(ta, tb, -1) == (59, 0) and shift_stats(ta, tb, 1) == (59, 0) and shift_stats(ta, tb, 0) == (60, 60),
        {WHOLE, CLIPPED, DROPPED} == set(ov["verdict"].tolist()),
        all(int(ov["insert"][2 * i]) == 0 for i, n in enumerate(c["names"]) if n == "plain"),
        len({int(o) & 15 for o in c["offs"][:-1]}) >= 12,                    # reads start at most bases of a word
    ]
    bad = [i for i, ok in enumerate(checks) if not ok]
    assert not bad, f"the case does not hold checks {bad}"
    return len(checks)
