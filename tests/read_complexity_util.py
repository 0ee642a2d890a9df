"""The low-complexity rule of include/sdt_gpu.h (sdt_gpu_complexity_reads) restated in numpy: what the tests of the kernel, the ABI and
`sdt-kmers complexity` expect.  Every window is cut out of the read, its triplets are counted per kind, and the low bases are kept as
one boolean per base; no 64-bit words, no masks, no lanes.  Nothing here touches the library under test.  Also the one case of
tests/test_read_complexity.py, built here so that the host tests can say that it holds what it promises."""
import functools

import numpy as np

from read_dedup_util import concat
from read_select_util import LETTERS

CX_FIELDS = ("windows", "low", "score", "start", "len", "verdict")
CX_DTYPE = np.dtype([(f, np.uint32) for f in CX_FIELDS])
WHOLE, CLIPPED, DROPPED = 0, 2, 3
A, C, T, G = range(4)
TRIM = 1                                                  # SDT_COMPLEXITY_TRIM
PARAM_FIELDS = ("max_score_pct", "max_low_pct", "min_len", "flags")
# the defaults of `sdt-kmers complexity`
DEFAULTS = dict(max_score_pct=10, max_low_pct=50, min_len=0, flags=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS)
    return p


def windows_of(L):
    """the windows of a read of L bases as [(begin, end)]"""
    W = 0 if L == 0 else max(1, -(-L // 32) - 1)
    return [(32 * j, min(32 * j + 64, L)) for j in range(W)]


def window_pairs(w):
    """(D, l) of one window: the ordered pairs of equal triplets, and the triplets"""
    w = np.asarray(w, dtype=np.int64)
    l = max(0, len(w) - 2)
    if l == 0:
        return 0, 0
    c = np.bincount(16 * w[:-2] + 4 * w[1:-1] + w[2:], minlength=64)
    return int((c * (c - 1)).sum()), l


def low_bases(read, max_score_pct):
    """-> (one boolean per base, the LOW windows, the score, the (D, l) of every window)"""
    read = np.asarray(read, dtype=np.uint8)
    low = np.zeros(len(read), dtype=bool)
    nlow = score = 0
    stats = []
    for b, e in windows_of(len(read)):
        D, l = window_pairs(read[b:e])
        stats.append((D, l))
        if l >= 2:
            score = max(score, 100 * D // (l * (l - 1)))
            if 100 * D >= max_score_pct * l * (l - 1):
                nlow += 1
                low[b:e] = True
    return low, nlow, score, stats


def clean_stretches(low):
    """the maximal runs of bases that are not low as [(start, length)], ascending"""
    edge = np.diff(np.concatenate([[1], low.astype(np.int8), [1]]))
    starts, ends = np.nonzero(edge == -1)[0], np.nonzero(edge == 1)[0]
    return [(int(s), int(e - s)) for s, e in zip(starts, ends)]


def complexity_read(read, p):
    """-> (windows, low, score, start, len, verdict)"""
    L = len(read)
    low, nlow, score, stats = low_bases(read, p["max_score_pct"])
    if p["flags"] & TRIM:
        runs = clean_stretches(low)
        start, ln = max(runs, key=lambda r: (r[1], -r[0])) if runs else (0, 0)
    else:
        start, ln = 0, (0 if 100 * int(low.sum()) > p["max_low_pct"] * L else L)
    if ln < max(p["min_len"], 1):
        return (len(stats), nlow, score, 0, 0, DROPPED)
    return (len(stats), nlow, score, start, ln, WHOLE if ln == L else CLIPPED)


def expect_complexity(codes, offs, p, ordinals=None):
    """-> (records, keep uint8[], reads with len > 0); with ordinals: record ordinals[r] is read r's, the others are zero"""
    n = len(offs) - 1
    idx = list(range(n)) if ordinals is None else [int(o) for o in ordinals]
    size = (max(idx) + 1) if idx else 0
    cx = np.zeros(size, dtype=CX_DTYPE)
    for r in range(n):
        cx[idx[r]] = complexity_read(codes[int(offs[r]):int(offs[r + 1])], p)
    keep = (cx["len"] > 0).astype(np.uint8)
    return cx, keep, int(keep.sum())


def cut_reads(codes, offs, cx):
    """the reads that compact_trimmed makes of the records"""
    return [codes[int(offs[r]) + int(c["start"]):int(offs[r]) + int(c["start"]) + int(c["len"])] for r, c in enumerate(cx) if c["len"]]


def assert_cx_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == CX_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in CX_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def random_window_scores(n, m, seed):
    """the scores (not rounded) of n random windows of m bases, all at once"""
    w = np.random.default_rng(seed).integers(0, 4, size=(n, m), dtype=np.int64)
    t = 16 * w[:, :-2] + 4 * w[:, 1:-1] + w[:, 2:]
    D = np.zeros(n, dtype=np.int64)
    for kind in range(64):
        c = (t == kind).sum(axis=1)
        D += c * (c - 1)
    l = m - 2
    return 100.0 * D / (l * (l - 1))


# ---- `sdt-kmers complexity` -------------------------------------------------------------------------------------------------------------
def cli_texts(codes, offs, cx, pair_ranges):
    """the four files of `sdt-kmers complexity` for a stream in ordinal order: (readComplexity, pairs.fa, single.fa, scoreHist)"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    rec_txt = "".join(f"{c['windows']} {c['low']} {c['score']} {c['start']} {c['len']} {c['verdict']}\n" for c in cx)
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if cx["len"][r]:
            s = int(offs[r]) + int(cx["start"][r])
            both = r in mate and cx["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{letters[s:s + int(cx['len'][r])]}\n")
    scores = sorted(set(int(s) for s in cx["score"]))
    hist = "".join(f"{s} {int((cx['score'] == s).sum())}\n" for s in scores)
    v = cx["verdict"]
    hist += f"# reads {n} low {int((cx['low'] > 0).sum())} dropped {int((v == DROPPED).sum())} clipped {int((v == CLIPPED).sum())}\n"
    return rec_txt, "".join(pairs), "".join(single), hist


# ---- the case of tests/test_read_complexity.py ------------------------------------------------------------------------------------------
CASE_PARAMS = params(max_score_pct=10, max_low_pct=50, min_len=20)
CASE_LENGTHS = (0, 1, 2, 3, 4, 31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 127, 128, 129, 150, 250, 2100)
# One window (L = l + 2 <= 64) whose D is exactly at the threshold of 10 %: 100 D = 10 l (l - 1).  D is even, so l (l - 1) / 10 must be.
AT_THRESHOLD = ((5, 2), (16, 24), (20, 38), (21, 42), (25, 60))                 # (l, D)
# ... and one ordered pair below it: 100 (D + 1) = 10 l (l - 1), where l (l - 1) / 10 is odd
BELOW_THRESHOLD = ((6, 2), (10, 8), (11, 10), (15, 20), (30, 86), (31, 92))


def _search(rng, l, D):
    """a read of l + 2 bases whose only window has exactly D ordered pairs of equal triplets, by trial"""
    for _ in range(200000):
        letters = rng.permutation(4)[:int(rng.integers(2, 5))].astype(np.uint8)          # over two, three or all four letters
        r = letters[rng.integers(0, len(letters), size=l + 2)]
        if window_pairs(r)[0] == D:
            return r
    raise AssertionError(f"no read of {l} triplets with D = {D} found")


def debruijn3():
    """66 bases in which every triplet occurs once (the de Bruijn sequence of order 3 over four letters, opened)"""
    seq, a = [], [0] * 12

    def db(t, p):
        if t > 3:
            if 3 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return np.array(seq + seq[:2], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def case():
    """About 150 reads, each under a name that says what it is there for; built once from a fixed seed and left unchanged"""
    rng = np.random.default_rng(20241019)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    homo = lambda b, n: np.full(n, b, dtype=np.uint8)
    rep = lambda unit, n: np.resize(np.asarray(unit, dtype=np.uint8), n)
    cat = lambda *parts: np.concatenate([np.asarray(x, dtype=np.uint8) for x in parts]).astype(np.uint8)

    def planted(L, at, run):                             # a random read of L bases with `run` over bases [at, at + len(run))
        r = rnd(L)
        r[max(at - 1, 0):at + len(run) + 1] = (int(run[0]) + 2) & 3       # (the bases next to the run do not extend it)
        r[at:at + len(run)] = run
        return r

    named = [(f"random {L}", rnd(L)) for L in CASE_LENGTHS]
    named += [(f"homopolymer {LETTERS[b]} {n}", homo(b, n)) for b in range(4) for n in (64, 33)]
    named += [("homopolymer A 150", homo(A, 150)), ("homopolymer G 2100", homo(G, 2100)),
              ("period 2 64", rep([A, C], 64)), ("period 2 150", rep([T, G], 150)), ("period 3 64", rep([A, C, G], 64)),
              ("period 3 97", rep([C, A, T], 97)), ("period 4 64", rep([A, C, T, G], 64)), ("period 6 64", rep([A, A, C, T, G, C], 64))]
    for n in (25, 30):
        for at in (20, 50, 118):
            named.append((f"poly-A {n} at {at}", planted(150, at, homo(A, n))))
            named.append((f"(AC) {n} at {at}", planted(150, at, rep([A, C], n))))
    # every triplet once (a de Bruijn sequence), so that the run alone decides: 18 triplets AAA in a full window give 306 of 3 782
    named += [("poly-A 20 at 54 of 128", cat(debruijn3()[:54], homo(A, 20), debruijn3()[12:])),
              ("poly-G 30 at the start", planted(150, 0, homo(G, 30))), ("poly-T 30 at the end", planted(150, 120, homo(T, 30))),
              ("poly-G 40 at the start of 2100", planted(2100, 0, homo(G, 40))), ("poly-C 36 at the end of 2100", planted(2100, 2064, homo(C, 36))),
              ("poly-A 30 at 1000 of 2100", planted(2100, 1000, homo(A, 30))),
              # window 1 alone is low: [0, 32) and [96, 128) are clean, the first wins
              ("tie of two stretches", planted(128, 50, homo(A, 30))),
              # windows 1 and 4 are low: [0, 32), [96, 128) and [192, 224) are clean
              ("tie of three stretches", planted(224, 50, cat(homo(C, 30), rnd(66), homo(G, 30)))),
              # window 0 alone is low, 64 bases: exactly half of 128, one base more than half of 126, less than half of 129
              ("low fraction at max_low_pct", planted(128, 2, homo(T, 30))), ("low fraction one base over", planted(126, 2, homo(T, 30))),
              ("low fraction under", planted(129, 2, homo(T, 30)))]
    for i in range(12):                                  # 12 of each, the (l, D) in turn
        l, D = AT_THRESHOLD[i % len(AT_THRESHOLD)]
        named.append((f"at the threshold {i}", _search(rng, l, D)))
        l, D = BELOW_THRESHOLD[i % len(BELOW_THRESHOLD)]
        named.append((f"below the threshold {i}", _search(rng, l, D)))
    names = [n for n, _ in named]
    reads = [r for _, r in named]
    while len(reads) < 150:                               # reads of random sequence, with whatever repeats chance gives
        names.append("plain")
        reads.append(rnd(int(rng.integers(30, 200))))
    order = rng.permutation(len(reads))
    reads, names = [reads[i] for i in order], [names[i] for i in order]
    codes, offs = concat(reads)
    return dict(reads=reads, names=names, codes=codes, offs=offs, params=CASE_PARAMS)


@functools.lru_cache(maxsize=None)
def case_expect(trim=False, max_score_pct=None):
    """the records of the case under its own parameters (or under SDT_COMPLEXITY_TRIM, or another max_score_pct), by the rule:
    computed once, shared by the tests, left unchanged"""
    c = case()
    p = dict(c["params"], max_score_pct=max_score_pct or c["params"]["max_score_pct"])
    if trim:
        p.update(max_low_pct=0, flags=TRIM)
    return expect_complexity(c["codes"], c["offs"], p)


def case_holds():
    """the case contains what its names promise, by the rule: -> the number of checks made"""
    c = case()
    cx, trim = case_expect()[0], case_expect(trim=True)[0]
    at = {n: i for i, n in enumerate(c["names"]) if n != "plain"}
    rec = lambda n: tuple(int(x) for x in cx[at[n]].tolist())
    cut = lambda n: tuple(int(x) for x in trim[at[n]].tolist())
    stats = lambda n: low_bases(c["reads"][at[n]], 10)[3]
    lows = lambda n: [j for j, (D, l) in enumerate(stats(n)) if l >= 2 and 100 * D >= 10 * l * (l - 1)]
    lengths = {len(r) for r in c["reads"]}
    checks = [
        set(CASE_LENGTHS) <= lengths,
        all(len(c["reads"][at[f"random {L}"]]) == L for L in CASE_LENGTHS),
        rec("random 0") == (0, 0, 0, 0, 0, DROPPED) and rec("random 3")[:3] == (1, 0, 0) and rec("random 2")[:3] == (1, 0, 0),
        [rec(f"random {L}")[0] for L in (32, 33, 64, 65, 96, 97, 128, 129, 150, 2100)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 65],
        all(rec(f"homopolymer {b} 64") == (1, 1, 100, 0, 0, DROPPED) and rec(f"homopolymer {b} 33") == (1, 1, 100, 0, 0, DROPPED) for b in LETTERS),
        rec("homopolymer A 150") == (4, 4, 100, 0, 0, DROPPED) and cut("homopolymer A 150") == (4, 4, 100, 0, 0, DROPPED),
        rec("homopolymer G 2100") == (65, 65, 100, 0, 0, DROPPED),
        [rec(f"period {k} 64")[2] for k in (2, 3, 4, 6)] == [49, 32, 23, 15],
        rec("period 2 150")[:3] == (4, 4, 49) and rec("period 3 97")[:2] == (3, 3),
        # runs of 30 bases make every window low that holds them whole, runs of 25 at least one; 20 bases pass
        all(lows(f"poly-A 30 at {a}") == w for a, w in ((20, [0]), (50, [1]), (118, [3]))),
        all(lows(f"(AC) 30 at {a}") == w for a, w in ((20, [0]), (50, [1]), (118, [3]))),
        all(len(lows(f"poly-A 25 at {a}")) >= 1 for a in (20, 50, 118)),
        lows("poly-A 20 at 54 of 128") == [] and rec("poly-A 20 at 54 of 128") == (3, 0, 8, 0, 128, WHOLE),
        # one low window of 64 in 150 bases: 6400 <= 7500, the read stays whole; trimmed, the longer clean side is kept
        rec("poly-A 30 at 50")[3:] == (0, 150, WHOLE) and cut("poly-A 30 at 50")[3:] == (96, 54, CLIPPED),
        cut("poly-A 30 at 20")[3:] == (64, 86, CLIPPED) and cut("poly-A 30 at 118")[3:] == (0, 96, CLIPPED),
        cut("poly-G 30 at the start")[3:] == (64, 86, CLIPPED) and cut("poly-T 30 at the end")[3:] == (0, 96, CLIPPED),
        cut("poly-G 40 at the start of 2100")[3:] == (64, 2036, CLIPPED) and cut("poly-C 36 at the end of 2100")[3:] == (0, 2048, CLIPPED),
        lows("poly-A 30 at 1000 of 2100") == [30, 31] and cut("poly-A 30 at 1000 of 2100")[3:] == (1056, 1044, CLIPPED),
        lows("tie of two stretches") == [1] and cut("tie of two stretches")[3:] == (0, 32, CLIPPED),
        lows("tie of three stretches") == [1, 4] and cut("tie of three stretches")[3:] == (0, 32, CLIPPED),
        lows("low fraction at max_low_pct") == [0] and rec("low fraction at max_low_pct")[3:] == (0, 128, WHOLE),
        lows("low fraction one base over") == [0] and rec("low fraction one base over")[3:] == (0, 0, DROPPED),
        lows("low fraction under") == [0] and rec("low fraction under")[3:] == (0, 129, WHOLE),
        sum(1 for n in at if n.startswith("at the threshold") and any(l >= 2 and 100 * D == 10 * l * (l - 1) for D, l in stats(n))
            and rec(n)[1] == 1) >= 10,
        sum(1 for n in at if n.startswith("below the threshold") and any(l >= 2 and 100 * (D + 1) == 10 * l * (l - 1) for D, l in stats(n))
            and rec(n)[1] == 0) >= 10,
        {WHOLE, DROPPED} == set(cx["verdict"].tolist()) and {WHOLE, CLIPPED, DROPPED} == set(trim["verdict"].tolist()),
        int((cx["low"] == cx["windows"]).sum()) >= 15 and int((cx["low"] == 0).sum()) >= 60,
    ]
    bad = [i for i, ok in enumerate(checks) if not ok]
    assert not bad, f"the case does not hold checks {bad}"
    return len(checks)
