"""The merge rule of include/sdt_gpu.h (sdt_gpu_merge_pairs, sdt_gpu_compact_quals_trimmed) restated in plain Python: what the tests of
the kernel, the ABI and `sdt-kmers merge` expect.  A merged read is built base by base; no windows, no bit tricks.  Nothing here touches
the library under test, and the overlap records that go in come from read_overlap_util (the overlap rule restated) or are written by
hand from the planted fragment.  Also the one case of tests/test_read_merge.py and the 600 pairs over two letters, built here so that the
host tests can say that they hold what they promise."""
import functools

import numpy as np

import read_overlap_util as ro
from read_dedup_util import concat
from read_select_util import LETTERS

MERGE_FIELDS = ("merged", "mismatches", "from_b", "start", "len", "verdict")
MERGE_DTYPE = np.dtype([(f, np.uint32) for f in MERGE_FIELDS])
MERGED = 5
PARAM_FIELDS = ("min_len", "max_len", "phred_offset", "flags")
# the defaults of `sdt-kmers merge`
DEFAULTS = dict(min_len=0, max_len=0, phred_offset=33, flags=0)
INCONSISTENT = -1


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS)
    return p


def quality_of(c, phred_offset):
    """as the quality stage reads a byte"""
    c = int(c)
    return 0 if c < phred_offset else min(c - phred_offset, 93)


def merge_decide(La, Lb, Fa, Fb, min_len, max_len):
    """the merged length, 0 (not merged) or INCONSISTENT: the four lines of MERGEABLE, a pair without overlap apart"""
    if Fa != Fb:
        return INCONSISTENT
    F = Fa
    if F == 0:
        return 0
    if not 1 <= F < La + Lb:
        return INCONSISTENT
    if F < max(min_len, 1):
        return 0
    if max_len != 0 and F > max_len:
        return 0
    return F


def merge_pair(a, b, F, qa=None, qb=None, phred_offset=33):
    """the merged read of a mergeable pair, position by position -> (m, mismatch columns, from_b)"""
    La, Lb = len(a), len(b)
    d = F - Lb
    assert -Lb < d < La
    m = np.zeros(F, dtype=np.uint8)
    mism = from_b = 0
    for p in range(F):
        in_a = p < La
        in_b = 0 <= p - d < Lb
        assert in_a or in_b
        bp = (int(b[Lb - 1 - (p - d)]) ^ 2) if in_b else None
        if in_a and in_b:
            base = int(a[p])
            if base != bp:
                mism += 1
                if qa is not None and quality_of(qb[Lb - 1 - (p - d)], phred_offset) > quality_of(qa[p], phred_offset):
                    base = bp
                    from_b += 1
            m[p] = base
        else:
            m[p] = int(a[p]) if in_a else bp
    return m, mism, from_b


def expect_merge(codes, offs, ov, p, quals=None, pair_ranges=None, ordinals=None):
    """-> (records, the merged reads in output order).  Dense (pair_ranges None): reads 2t and 2t + 1 are mates, ov and the records by
    read.  With ordinals: ov and the records by ordinal (ordinals[r] is read r's, the others stay zero); the pairs are the ordinals
    first + 2t, first + 2t + 1 of a range that both have a read, every other read is single.  ValueError for inconsistent records"""
    n = len(offs) - 1
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(n)]
    qs = [quals[int(offs[r]):int(offs[r + 1])] for r in range(n)] if quals is not None else None
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
    second = set(mate.values())
    mg = np.zeros(size, dtype=MERGE_DTYPE)
    out = []
    for o in sorted(at):
        if o in second:
            continue
        r = at[o]
        F = 0
        if o in mate:
            rb = at[o + 1]
            F = merge_decide(len(reads[r]), len(reads[rb]), int(ov["insert"][o]), int(ov["insert"][o + 1]), p["min_len"], p["max_len"])
            if F == INCONSISTENT:
                raise ValueError(f"pair at {o}: inserts {int(ov['insert'][o])} and {int(ov['insert'][o + 1])}")
        if F:
            m, h, fb = merge_pair(reads[r], reads[rb], F, qs[r] if qs else None, qs[rb] if qs else None, p["phred_offset"])
            mg[o] = mg[o + 1] = (F, h, fb, 0, 0, MERGED)
            out.append(m)
        else:
            for x in (o, o + 1) if o in mate else (o,):
                mg[x] = (0, 0, 0, int(ov["start"][x]), int(ov["len"][x]), int(ov["verdict"][x]))
    return mg, out


def rest_reads(codes, offs, mg):
    """the reads that compact_trimmed makes of the merge records: what is left of the pairs that did not merge"""
    return ro.cut_reads(codes, offs, mg)


def pack_stream(reads):
    """reads -> (words with the 4 pad words, offsets) as the library packs a stream"""
    codes, offs = concat(reads)
    n = len(codes)
    buf = np.zeros((n + 15) // 16 * 16, dtype=np.uint32)
    buf[:n] = codes
    shifts = (30 - 2 * np.arange(16)).astype(np.uint32)
    words = np.bitwise_or.reduce(buf.reshape(-1, 16) << shifts, axis=1).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    return np.concatenate([words, np.zeros(4, dtype=np.uint32)]), offs


def compact_bytes(quals, offs, recs):
    """compact_quals_trimmed by slicing -> the kept bytes, zero-padded to a multiple of 4, and their number"""
    parts = [quals[int(offs[r]) + int(c["start"]):int(offs[r]) + int(c["start"]) + int(c["len"])] for r, c in enumerate(recs) if c["len"]]
    out = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, dtype=np.uint8)
    return np.concatenate([out, np.zeros(-len(out) % 4, dtype=np.uint8)]), len(out)


def assert_merge_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == MERGE_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in MERGE_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def assert_stream_equal(got_words, got_offs, reads, what=""):
    """every output word, the zero tail bits and the four zero pad words"""
    words, offs = pack_stream(reads)
    assert np.asarray(got_offs).tolist() == offs.tolist(), f"{what}: out_offsets differ"
    assert len(got_words) == len(words), f"{what}: {len(got_words)} words, {len(words)} expected"
    bad = np.nonzero(np.asarray(got_words) != words)[0]
    assert bad.size == 0, f"{what}: words differ at {bad[:8].tolist()}"


# ---- `sdt-kmers merge` ----------------------------------------------------------------------------------------------------------------
def cli_texts(codes, offs, ov, mg, merged_reads, pair_ranges):
    """the files of `sdt-kmers merge` for a stream in ordinal order: (readMerge, merge.fa, merge.pairs.fa, merge.single.fa, insertHist,
    the summary line)"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    text = lambda c: letters[np.asarray(c, dtype=np.uint8)].tobytes().decode()
    rec_txt = "".join(" ".join(str(int(c[f])) for f in MERGE_FIELDS) + "\n" for c in mg)
    firsts = [r for first, end in pair_ranges for r in range(first, end, 2) if mg["merged"][r]]
    assert len(firsts) == len(merged_reads)
    merged_txt = "".join(f">{r + 1}\n{text(m)}\n" for r, m in zip(firsts, merged_reads))
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if mg["len"][r]:
            s = int(offs[r]) + int(mg["start"][r])
            both = r in mate and mg["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{text(codes[s:s + int(mg['len'][r])])}\n")
    hist = ro.cli_texts(codes, offs, ov, pair_ranges)[3]
    npairs = sum((end - first) // 2 for first, end in pair_ranges)
    overlapping = sum(1 for first, end in pair_ranges for r in range(first, end, 2) if ov["insert"][r])
    cols = sum(int(mg["mismatches"][r]) for r in firsts)
    bases_out = sum(len(m) for m in merged_reads) + int(mg["len"].astype(np.int64).sum())
    summary = (f"merge: reads {n} pairs {npairs} overlapping {overlapping} merged {len(firsts)} mismatch columns {cols} "
               f"bases in {int(offs[-1])} bases out {bases_out}")
    return rec_txt, merged_txt, "".join(pairs), "".join(single), hist, summary


# ---- 600 pairs over two letters -------------------------------------------------------------------------------------------------------
AT_PARAMS = params()


@functools.lru_cache(maxsize=None)
def at_quals():
    """random quality bytes for the 600 pairs of read_overlap_util.at_pairs(), under phred 33: built once from a fixed seed"""
    _, codes, _ = ro.at_pairs()
    return np.random.default_rng(20250611).integers(33, 75, size=len(codes), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def at_expect(with_quals):
    """the merge of the 600 pairs by the overlap records of the overlap rule -> (records, merged reads); asserts of itself that at least
    100 pairs merge and that under the qualities at least 50 have from_b > 0"""
    _, codes, offs = ro.at_pairs()
    ov = ro.at_expect()[0]
    mg, out = expect_merge(codes, offs, ov, AT_PARAMS, at_quals() if with_quals else None)
    assert len(out) >= 100, len(out)
    if with_quals:
        assert int((mg["from_b"][0::2] > 0).sum()) >= 50, int((mg["from_b"][0::2] > 0).sum())
    else:
        assert not mg["from_b"].any()
    return mg, out


# ---- the case of tests/test_read_merge.py ---------------------------------------------------------------------------------------------
CASE_OVERLAP = ro.params(min_overlap=1, max_err_pct=100, min_len=40)      # (min_len 40: the overlap records drop short mates)
CASE_PARAMS = params(min_len=2, max_len=4100)
MATE_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 150, 250)
# quality bytes planted at mismatch columns, (mate 1, mate 2): under phred 33 qb > qa, a tie, qb < qa, a byte below the offset, bytes
# past offset + 93 (both saturate: a tie), and a pair that phred 64 decides the other way round than phred 33
PLANTED_QUALS = ((40, 70), (60, 60), (70, 40), (20, 50), (200, 130), (130, 200), (70, 90), (100, 63))


@functools.lru_cache(maxsize=None)
def case(seed=20250610):
    """Pairs with planted fragments and hand-written overlap records, each under a name that says what it is there for; built once and
    left unchanged.  `pairs` holds (a, b) per name in the order of `names`, `inserts` the planted insert (0: no overlap), `columns` the
    planted mismatch columns (positions of the merged read); reads, codes, offs and quals are the interleaved stream, ov its overlap
    records."""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *parts: np.concatenate([np.asarray(x, dtype=np.uint8) for x in parts]).astype(np.uint8)
    named = []

    def planted(name, F, La, Lb, columns=()):
        """a fragment of F bases read from both ends, La and Lb bases deep, with different random adapters past the fragment's end;
        mate 2 then gets another base at the given columns of the overlap"""
        frag = rnd(F)
        a = cat(frag, rnd(La - F)) if La > F else frag[:La]
        b = cat(ro.revcomp(frag), rnd(Lb - F)) if Lb > F else ro.revcomp(frag)[:Lb]
        b = np.array(b, dtype=np.uint8)
        d = F - Lb
        for p in columns:
            assert max(0, d) <= p < min(La, F)
            b[Lb - 1 - (p - d)] = (b[Lb - 1 - (p - d)] + 1 + p % 3) & 3
        named.append((name, (a, b), F, tuple(columns)))

    for L in MATE_LENGTHS[1:]:
        planted(f"F = La = Lb = {L}", L, L, L)
    planted("read-through, F < La", 100, 150, 150, (0, 50, 99))
    planted("La < F < La + Lb", 220, 150, 150, (70, 149))                # the first and the last column of the overlap
    planted("one column", 199, 100, 100)
    planted("one column, a mismatch", 199, 100, 100, (99,))
    planted("long a, short b inside it", 90, 150, 60, (30, 89))
    planted("short a, long b", 90, 60, 150, (0, 59))
    planted("unequal, a longer", 200, 150, 100)
    planted("unequal, b longer", 200, 100, 150, (63, 64))
    planted("mates of 250", 333, 250, 250, (83, 249))
    planted("columns 31 / 32, two in one window", 100, 100, 100, (31, 32, 40, 41, 95, 96))
    planted("F = 2047", 2047, 1200, 1200, (847, 1199))
    planted("F = 2048", 2048, 1200, 1200, (848, 1023, 1024))
    planted("F = 2049", 2049, 1200, 1200, (1199,))
    planted("F = 4100, columns 2047 / 2048", 4100, 2100, 2100, (2000, 2047, 2048, 2099))
    planted("max_len refuses", 4101, 2100, 2100)
    planted("min_len refuses", 1, 1, 1)
    planted("the overlap record dropped b", 50, 150, 32, (20, 49))       # b has 32 < 40 bases: its record has len = 0, the pair merges
    a = rnd(100)
    named.append(("no overlap, b dropped by the overlap stage", (a, rnd(29)), 0, ()))
    named.append(("mate of 0 bases", (rnd(80), np.zeros(0, dtype=np.uint8)), 0, ()))
    named.append(("both of 0 bases", (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)), 0, ()))
    for i in range(4):
        named.append(("no overlap", (rnd(int(rng.integers(40, 160))), rnd(int(rng.integers(40, 160)))), 0, ()))
    order = rng.permutation(len(named))
    named = [named[i] for i in order]
    names = [x[0] for x in named]
    pairs = [x[1] for x in named]
    inserts = [x[2] for x in named]
    columns = [x[3] for x in named]
    reads = [r for pr in pairs for r in pr]
    codes, offs = concat(reads)
    # the overlap records, written by hand from what was planted: o and h of the planted shift counted base by base
    ov = np.zeros(len(reads), dtype=ro.OVERLAP_DTYPE)
    for t, ((a, b), F) in enumerate(zip(pairs, inserts)):
        found = ro.shift_stats(a, b, F - len(b)) + (F,) if F else (0, 0, 0)
        ov[2 * t] = ro.read_record(len(a), found, CASE_OVERLAP["min_len"])
        ov[2 * t + 1] = ro.read_record(len(b), found, CASE_OVERLAP["min_len"])
    # the qualities: random bytes of phred 33, the planted pairs at the planted columns in turn
    quals = rng.integers(35, 75, size=len(codes), dtype=np.uint8)
    k = 0
    for t, ((a, b), F, cols) in enumerate(zip(pairs, inserts, columns)):
        for p in cols:
            qa, qb = PLANTED_QUALS[k % len(PLANTED_QUALS)]
            k += 1
            quals[int(offs[2 * t]) + p] = qa
            quals[int(offs[2 * t + 1]) + (F - 1 - p)] = qb
    return dict(names=names, pairs=pairs, inserts=inserts, columns=columns, reads=reads, codes=codes, offs=offs, quals=quals, ov=ov,
                params=CASE_PARAMS)


@functools.lru_cache(maxsize=None)
def case_expect(phred=None):
    """the records and the merged reads of the case, without qualities (None) or with them under phred 33 / 64: computed once per
    setting, shared by the tests, left unchanged"""
    c = case()
    p = dict(c["params"], phred_offset=phred if phred is not None else 33)
    return expect_merge(c["codes"], c["offs"], c["ov"], p, c["quals"] if phred is not None else None)


def case_holds():
    """the case contains what its names promise, by the rule: -> the number of checks made"""
    c = case()
    names, pairs, inserts, ov = c["names"], c["pairs"], c["inserts"], c["ov"]
    at = {n: i for i, n in enumerate(names) if n != "no overlap"}
    plain, q33, q64 = case_expect(None), case_expect(33), case_expect(64)
    rec = lambda e, n, m=0: tuple(int(x) for x in e[0][2 * at[n] + m].tolist())
    lens = {len(r) for r in c["reads"]}
    sit = lambda n: (len(pairs[at[n]][0]), len(pairs[at[n]][1]), inserts[at[n]])
    merged_of = lambda e, n: e[1][sorted(i for i in range(len(names)) if e[0]["merged"][2 * i]).index(at[n])]
    big = at["F = 4100, columns 2047 / 2048"]
    checks = [
        set(MATE_LENGTHS) <= lens,
        all(rec(plain, f"F = La = Lb = {L}") == (L, 0, 0, 0, 0, MERGED) for L in MATE_LENGTHS[2:]),
        rec(plain, "min_len refuses") == rec(plain, "F = La = Lb = 1") == (0, 0, 0, 0, 0, ro.DROPPED),       # (1 < 40: the overlap stage dropped both)
        rec(plain, "max_len refuses") == (0, 0, 0, 0, 2100, ro.WHOLE) and inserts[at["max_len refuses"]] == c["params"]["max_len"] + 1,
        sit("read-through, F < La")[2] < sit("read-through, F < La")[0],
        sit("La < F < La + Lb") == (150, 150, 220),
        sit("one column")[2] == sum(sit("one column")[:2]) - 1 and rec(plain, "one column") == (199, 0, 0, 0, 0, MERGED),
        rec(plain, "one column, a mismatch") == (199, 1, 0, 0, 0, MERGED),
        sit("long a, short b inside it") == (150, 60, 90) and sit("short a, long b") == (60, 150, 90),
        rec(plain, "unequal, a longer")[0] == rec(plain, "unequal, b longer")[0] == 200,
        [rec(plain, f"F = {F}")[0] for F in (2047, 2048, 2049)] == [2047, 2048, 2049],
        rec(plain, "F = 4100, columns 2047 / 2048") == (4100, 4, 0, 0, 0, MERGED) and 4100 > 2 * 2048,
        rec(plain, "read-through, F < La")[:3] == (100, 3, 0),
        rec(plain, "La < F < La + Lb")[:3] == (220, 2, 0) and c["columns"][at["La < F < La + Lb"]] == (220 - 150, 150 - 1),
        rec(plain, "columns 31 / 32, two in one window")[:3] == (100, 6, 0),
        {2047, 2048} <= set(c["columns"][big]),
        rec(plain, "the overlap record dropped b") == (50, 2, 0, 0, 0, MERGED) and tuple(ov[2 * at["the overlap record dropped b"] + 1].tolist())[3:] == (0, 0, ro.DROPPED),
        rec(plain, "no overlap, b dropped by the overlap stage", 0) == (0, 0, 0, 0, 100, ro.WHOLE),
        rec(plain, "no overlap, b dropped by the overlap stage", 1) == (0, 0, 0, 0, 0, ro.DROPPED),
        rec(plain, "mate of 0 bases", 0) == (0, 0, 0, 0, 80, ro.WHOLE) and rec(plain, "both of 0 bases") == (0, 0, 0, 0, 0, ro.DROPPED),
        all(int(plain[0]["merged"][2 * i]) == 0 and int(plain[0]["len"][2 * i]) > 0 for i, n in enumerate(names) if n == "no overlap"),
        # without qualities a mismatch column is mate 1's base; with them the two phred offsets decide differently
        (plain[0]["mismatches"] == q33[0]["mismatches"]).all() and (plain[0]["mismatches"] == q64[0]["mismatches"]).all(),
        not plain[0]["from_b"].any() and q33[0]["from_b"].sum() > 0 and q64[0]["from_b"].sum() > 0,
        (q33[0]["from_b"] != q64[0]["from_b"]).any(),
        any((m33 != m0).any() for m33, m0 in zip(q33[1], plain[1])) and any((m64 != m33).any() for m64, m33 in zip(q64[1], q33[1])),
        (merged_of(plain, "La < F < La + Lb")[:150] == pairs[at["La < F < La + Lb"]][0]).all(),
        # every situation of PLANTED_QUALS occurs under phred 33: qb > qa, a tie, qb < qa, a byte below the offset, bytes past offset + 93
        _situations(c, 33) >= {"b", "tie", "a", "below", "above"} and _situations(c, 64) >= {"b", "tie", "a", "below", "above"},
        len({int(o) & 15 for o in c["offs"][:-1]}) >= 12,                    # reads start at most bases of a word
    ]
    try:                                                                     # records that are not one overlap are refused
        bad = ov.copy()
        bad["insert"][1] += 1
        expect_merge(c["codes"], c["offs"], bad, c["params"])
        checks.append(False)
    except ValueError:
        checks.append(True)
    bad = [i for i, ok in enumerate(checks) if not ok]
    assert not bad, f"the case does not hold checks {bad}"
    return len(checks)


def _situations(c, phred):
    found = set()
    for t, (F, cols) in enumerate(zip(c["inserts"], c["columns"])):
        for p in cols:
            ca, cb = int(c["quals"][int(c["offs"][2 * t]) + p]), int(c["quals"][int(c["offs"][2 * t + 1]) + (F - 1 - p)])
            qa, qb = quality_of(ca, phred), quality_of(cb, phred)
            found.add("b" if qb > qa else ("tie" if qb == qa else "a"))
            if ca < phred or cb < phred:
                found.add("below")
            if ca > phred + 93 or cb > phred + 93:
                found.add("above")
    return found
