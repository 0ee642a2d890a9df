"""The quality rule of include/sdt_gpu.h (sdt_gpu_quality_reads) restated in numpy, in the scan form: what the tests of the kernel, the
ABI and `sdt-kmers qtrim` expect.  Prefix sums, a running minimum with the first place that attains it, and one pick by the key; no
words, no masks, no lanes.  Nothing here touches the library under test.  Also the one case of tests/test_read_quality.py, built here
so that the host tests can say that it holds what it promises."""
import functools

import numpy as np

from read_select_util import LETTERS

Q_FIELDS = ("span", "low", "ee_ppm", "start", "len", "verdict")
Q_DTYPE = np.dtype([(f, np.uint32) for f in Q_FIELDS])
WHOLE, CLIPPED, DROPPED = 0, 2, 3
PARAM_FIELDS = ("phred_offset", "cut_q", "low_q", "max_low_pct", "max_ee_ppm", "min_len", "flags", "reserved")
# the defaults of `sdt-kmers qtrim`
DEFAULTS = dict(phred_offset=33, cut_q=20, low_q=15, max_low_pct=40, max_ee_ppm=0, min_len=0, flags=0, reserved=0)
MAX_Q = 93


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS)
    return p


def _ee(q):
    """10^6 * 10^(-q / 10) rounded to the nearest integer, exactly: the t with (2t - 1)^10 10^q <= (2 10^6)^10 < (2t + 1)^10 10^q"""
    top = (2 * 10 ** 6) ** 10
    t = int(round(1e6 * 10 ** (-q / 10)))
    while (2 * t + 1) ** 10 * 10 ** q <= top:
        t += 1
    while t > 0 and (2 * t - 1) ** 10 * 10 ** q > top:
        t -= 1
    assert (2 * t + 1) ** 10 * 10 ** q != top and (t == 0 or (2 * t - 1) ** 10 * 10 ** q != top), "a tie"
    return t


EE_PPM = np.array([_ee(q) for q in range(MAX_Q + 1)], dtype=np.int64)


def quality_of(c, phred_offset):
    """the qualities that the bytes c say"""
    c = np.asarray(c, dtype=np.int64)
    return np.where(c < phred_offset, 0, np.minimum(c - phred_offset, MAX_Q))


def segment_scan(q, cut_q):
    """[a, b) of the qualities q by the scan form of the rule"""
    P = np.concatenate([[0], np.cumsum(np.asarray(q, dtype=np.int64) - cut_q)])
    M = np.minimum.accumulate(P)
    idx = np.arange(len(P))
    new = np.concatenate([[True], P[1:] < M[:-1]])                    # a strictly lower prefix sum: the first place that attains M
    a = np.maximum.accumulate(np.where(new, idx, 0))
    b = np.lexsort((idx, -a, P - M))[-1]                              # gain descending, a ascending, b descending: the last under the sort
    return int(a[b]), int(b)


def segment_brute(q, cut_q):
    """[a, b) by the search over all of them"""
    s = [int(x) - cut_q for x in q]
    best = None
    for a in range(len(s) + 1):
        for b in range(a, len(s) + 1):
            key = (sum(s[a:b]), -a, b)
            if best is None or key > best:
                best = key
    return -best[1], best[2]


def segment_loop(q, cut_q):
    """[a, b) by a plain loop over b"""
    P = m = am = 0
    best = (0, 0, 0)
    for b in range(1, len(q) + 1):
        P += int(q[b - 1]) - cut_q
        if P < m:
            m, am = P, b
        best = max(best, (P - m, -am, b))
    return -best[1], best[2]


def optimal_segments(q, cut_q):
    """how many [a, b) have the greatest sum"""
    P = np.concatenate([[0], np.cumsum(np.asarray(q, dtype=np.int64) - cut_q)])
    d = P[None, :] - P[:, None]
    d[np.tril_indices(len(P), -1)] = np.iinfo(np.int64).min
    return int((d == d.max()).sum())


def measures(c, p):
    """-> (a, b, low, ee_ppm) of the bytes of one read"""
    q = quality_of(c, p["phred_offset"])
    a, b = segment_scan(q, p["cut_q"])
    seg = q[a:b]
    return a, b, int((seg < p["low_q"]).sum()), (int(EE_PPM[seg].sum()) // (b - a) if b > a else 0)


def drop_cause(span, low, ee_ppm, p):
    """the line of the verdict that drops a read with these measures: 'short', 'low', 'errors', or None"""
    if span < max(p["min_len"], 1):
        return "short"
    if 100 * low > p["max_low_pct"] * span:
        return "low"
    if p["max_ee_ppm"] != 0 and ee_ppm > p["max_ee_ppm"]:
        return "errors"
    return None


def quality_read(c, p):
    """-> (span, low, ee_ppm, start, len, verdict)"""
    a, b, low, ee = measures(c, p)
    n = b - a
    if drop_cause(n, low, ee, p):
        return (n, low, ee, 0, 0, DROPPED)
    return (n, low, ee, 0, n, WHOLE) if n == len(c) else (n, low, ee, a, n, CLIPPED)


def expect_quality(quals, offs, p):
    """-> (records, keep uint8[], reads with len > 0)"""
    n = len(offs) - 1
    out = np.zeros(n, dtype=Q_DTYPE)
    for r in range(n):
        out[r] = quality_read(quals[int(offs[r]):int(offs[r + 1])], p)
    keep = (out["len"] > 0).astype(np.uint8)
    return out, keep, int(keep.sum())


def causes(out, p):
    return [drop_cause(int(r["span"]), int(r["low"]), int(r["ee_ppm"]), p) if r["verdict"] == DROPPED else None for r in out]


def cut_reads(codes, offs, out):
    """the reads that compact_trimmed makes of the records"""
    return [codes[int(offs[r]) + int(c["start"]):int(offs[r]) + int(c["start"]) + int(c["len"])] for r, c in enumerate(out) if c["len"]]


def assert_q_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == Q_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in Q_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def concat_bytes(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    quals = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if reads else np.zeros(0, dtype=np.uint8)
    return quals.astype(np.uint8), offs


def realistic(rng, L, i=0):
    """the qualities of one read as a sequencer gives them: a plateau of 30 to 40 that falls to 2 to 15 from a random base on; low 5'
    ends in one read in seven, a run of quality 2 inside one read in eleven (i: the read's number)"""
    if L == 0:
        return np.zeros(0, dtype=np.int64)
    base = int(rng.integers(30, 41))
    drop = int(rng.integers(L // 3, L + 40))
    q = np.where(np.arange(L) < drop, base + rng.integers(-6, 3, L), rng.integers(2, 16, L))
    if i % 7 == 0:
        q[:int(rng.integers(1, 8))] = 2
    if i % 11 == 0 and L > 10:
        a = int(rng.integers(0, L - 10))
        q[a:a + int(rng.integers(1, 10))] = 2
    return np.clip(q, 0, 41)


# ---- `sdt-kmers qtrim` ---------------------------------------------------------------------------------------------------------------------
def cli_texts(codes, offs, out, pair_ranges, p):
    """the four files of `sdt-kmers qtrim` for a stream in ordinal order: (readQual, pairs.fa, single.fa, lenHist)"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    rec_txt = "".join(f"{c['span']} {c['low']} {c['ee_ppm']} {c['start']} {c['len']} {c['verdict']}\n" for c in out)
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if out["len"][r]:
            s = int(offs[r]) + int(out["start"][r])
            both = r in mate and out["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{letters[s:s + int(out['len'][r])]}\n")
    kept = out["len"][out["len"] > 0]
    hist = "".join(f"{ln} {int((kept == ln).sum())}\n" for ln in sorted(set(int(x) for x in kept)))
    v, why = out["verdict"], causes(out, p)
    hist += (f"# reads {n} whole {int((v == WHOLE).sum())} clipped {int((v == CLIPPED).sum())} dropped {int((v == DROPPED).sum())} "
             f"short {why.count('short')} low {why.count('low')} errors {why.count('errors')} "
             f"bases_in {int(offs[-1]) - int(offs[0])} bases_out {int(out['len'].sum())}\n")
    return rec_txt, "".join(pairs), "".join(single), hist


# ---- the case of tests/test_read_quality.py -------------------------------------------------------------------------------------------------
CASE_PARAMS = params(max_ee_ppm=30000, min_len=20)
CASE_LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 5000)


@functools.lru_cache(maxsize=None)
def case():
    """About 150 reads of quality bytes (offset 33), each under a name that says what it is there for; built once from a fixed seed and
    left unchanged"""
    rng = np.random.default_rng(20261019)
    Q = lambda *parts: (np.concatenate([np.asarray(x, dtype=np.int64).ravel() for x in parts]) + 33).astype(np.uint8)
    flat = lambda q, n: np.full(n, q, dtype=np.int64)
    named = []
    for L in CASE_LENGTHS:
        named += [(f"above {L}", Q(flat(35, L))), (f"below {L}", Q(flat(12, L))), (f"equal {L}", Q(flat(20, L))),
                  (f"realistic {L}", Q(realistic(rng, L, L)))]
    named += [
        # two maxima of 25 * 10, the trough between them weighs more: the first wins
        ("two maxima", Q(flat(30, 25), flat(2, 20), flat(30, 25))),
        # -10 then +10 behind the maximum: the same sum two bases further, the greatest b wins
        ("extension to the right", Q(flat(30, 25), [10, 30], flat(2, 10))),
        # the same in front of it: +10 then -10 before the maximum starts: the smallest a wins, and takes both along
        ("extension to the left", Q(flat(2, 10), [30, 10], flat(30, 25), flat(2, 5))),
        ("straddles base 256", Q(flat(5, 100), flat(36, 250), flat(5, 50))),
        ("straddles bases 256 and 512", Q(flat(5, 200), flat(36, 400), flat(5, 100))),
        ("minimum in step 0, end in step 3", Q(flat(5, 50), flat(36, 850), flat(5, 100))),
        ("starts at its last base", Q(flat(2, 39), [40])),
        ("starts at its last base, 257", Q(flat(2, 256), [40])),
        ("ends at its first base", Q([40], flat(2, 39))),
        # bytes below the offset are quality 0, bytes above offset + 93 are quality 93
        ("bytes below the offset", np.concatenate([Q(flat(35, 30)), np.arange(0, 33, dtype=np.uint8), Q(flat(35, 30))])),
        ("bytes above 93", np.concatenate([Q(flat(12, 10)), np.arange(126, 256, dtype=np.uint8), Q(flat(12, 10))])),
        ("byte 255", np.full(40, 255, dtype=np.uint8)),
        ("byte 0", np.zeros(40, dtype=np.uint8)),
        ("min_len less one", Q(flat(5, 30), flat(35, 19), flat(5, 30))),
        ("min_len exactly", Q(flat(5, 30), flat(35, 20), flat(5, 30))),
        ("quality 2 inside", Q(flat(36, 60), flat(2, 5), flat(36, 60))),
        ("quality 2 at both ends", Q(flat(2, 7), flat(36, 100), flat(2, 9))),
        ("quality 2 inside and at both ends", Q(flat(2, 3), flat(36, 50), flat(2, 4), flat(36, 50), flat(2, 12))),
        ("quality 2 inside, 600", Q(flat(36, 250), flat(2, 12), flat(36, 338))),
        # 40 low bases of 100 pass, 41 do not
        ("low share at max_low_pct", Q(np.resize([40, 14, 14, 40, 40], 100))),
        ("low share one base over", Q([40, 14, 14, 40, 14], np.resize([40, 14, 14, 40, 40], 95))),
    ]
    for i in range(12):
        n = int(rng.integers(1, 20))
        named.append((f"short {i}", Q(flat(4, int(rng.integers(0, 30))), flat(38, n), flat(4, int(rng.integers(1, 30))))))
        # 9 bases in 19 at quality 14, between high ones: the share of low bases drops it, 0.47 * 39 811 expected errors per million do not
        named.append((f"low {i}", Q([40, 40], np.resize([14] * 9 + [40] * 10, 19 * (2 + i)))))
        # 3 bases in 10 at quality 5: not too many low bases, but 0.3 * 316 228 expected errors per million
        named.append((f"errors {i}", Q([40, 40], np.resize([5] * 3 + [40] * 7, 10 * (4 + i)))))
    names = [n for n, _ in named]
    reads = [r for _, r in named]
    i = 0
    while len(reads) < 150:
        names.append("plain")
        reads.append(Q(realistic(rng, int(rng.integers(30, 200)), i)))
        i += 1
    order = rng.permutation(len(reads))
    reads, names = [reads[i] for i in order], [names[i] for i in order]
    quals, offs = concat_bytes(reads)
    # bases for the reads: the stage does not look at them, compaction and the command line do
    codes = rng.integers(0, 4, size=len(quals), dtype=np.uint8)
    return dict(reads=reads, names=names, quals=quals, offs=offs, codes=codes, params=CASE_PARAMS)


@functools.lru_cache(maxsize=None)
def case_expect(**kw):
    """the records of the case under its own parameters with the fields of kw changed, by the rule: computed once per set of
    parameters, shared by the tests, left unchanged"""
    c = case()
    return expect_quality(c["quals"], c["offs"], dict(c["params"], **kw))


def case_holds():
    """the case contains what its names promise, by the rule: -> the number of checks made"""
    c = case()
    p = c["params"]
    out = case_expect()[0]
    at = {n: i for i, n in enumerate(c["names"]) if n != "plain"}
    rec = lambda n: tuple(int(x) for x in out[at[n]].tolist())
    why = causes(out, p)
    cause = lambda n: why[at[n]]
    L = lambda n: len(c["reads"][at[n]])
    kinds = ("above", "below", "equal", "realistic")
    checks = [
        len(at) + c["names"].count("plain") == len(c["reads"]) >= 150,
        all(L(f"{k} {n}") == n for k in kinds for n in CASE_LENGTHS),
        all(rec(f"above {n}") == ((n, 0, 316, 0, n, WHOLE) if n >= 20 else (n, 0, 316 if n else 0, 0, 0, DROPPED)) for n in CASE_LENGTHS),
        all(rec(f"below {n}") == (0, 0, 0, 0, 0, DROPPED) for n in CASE_LENGTHS),
        all(rec(f"equal {n}")[0] == n and rec(f"equal {n}")[2] == (10000 if n else 0) for n in CASE_LENGTHS),
        rec("equal 1000") == (1000, 0, 10000, 0, 1000, WHOLE),
        rec("two maxima")[3:] == (0, 25, CLIPPED),
        rec("extension to the right")[3:] == (0, 27, CLIPPED) and rec("extension to the right")[1] == 1,
        rec("extension to the left")[3:] == (10, 27, CLIPPED),
        rec("straddles base 256")[3:] == (100, 250, CLIPPED) and rec("straddles bases 256 and 512")[3:] == (200, 400, CLIPPED),
        rec("minimum in step 0, end in step 3")[3:] == (50, 850, CLIPPED),
        rec("starts at its last base") == (1, 0, 100, 0, 0, DROPPED) and cause("starts at its last base") == "short",
        measures(c["reads"][at["starts at its last base"]], p)[:2] == (39, 40),
        measures(c["reads"][at["starts at its last base, 257"]], p)[:2] == (256, 257),
        measures(c["reads"][at["ends at its first base"]], p)[:2] == (0, 1),
        # 30 + 33 + 30 bytes: the 33 bytes below the offset are quality 0 and split the read; the first side wins
        rec("bytes below the offset")[3:] == (0, 30, CLIPPED),
        # bytes 126 to 255: quality 93 from byte 126 on
        rec("bytes above 93") == (130, 0, 0, 10, 130, CLIPPED),
        rec("byte 255") == (40, 0, 0, 0, 40, WHOLE) and rec("byte 0") == (0, 0, 0, 0, 0, DROPPED),
        rec("min_len less one") == (19, 0, 316, 0, 0, DROPPED) and cause("min_len less one") == "short",
        rec("min_len exactly") == (20, 0, 316, 30, 20, CLIPPED),
        rec("quality 2 inside")[:2] == (125, 5) and rec("quality 2 inside")[3:] == (0, 125, WHOLE),
        rec("quality 2 at both ends") == (100, 0, 251, 7, 100, CLIPPED),
        rec("quality 2 inside and at both ends")[:2] == (104, 4) and rec("quality 2 inside and at both ends")[3:] == (3, 104, CLIPPED),
        rec("quality 2 inside, 600")[:2] == (600, 12) and rec("quality 2 inside, 600")[5] == WHOLE,
        rec("low share at max_low_pct")[:2] == (100, 40) and rec("low share at max_low_pct")[3:] == (0, 100, WHOLE),
        rec("low share one base over")[:2] == (100, 41) and cause("low share one base over") == "low",
        sum(1 for n in at if n.startswith("short ") and cause(n) == "short" and rec(n)[0] >= 1) >= 10,
        # dropped by their line and by no other: under the rule with that line switched off they stay
        sum(1 for n in at if n.startswith("low ") and cause(n) == "low" and rec(n)[0] >= 20 and rec(n)[2] <= p["max_ee_ppm"]) >= 10,
        sum(1 for n in at if n.startswith("errors ") and cause(n) == "errors" and rec(n)[0] >= 20 and 100 * rec(n)[1] <= 40 * rec(n)[0]) >= 10,
        all(int((out["verdict"] == v).sum()) >= 10 for v in (WHOLE, CLIPPED, DROPPED)),
        all(why.count(k) >= 10 for k in ("short", "low", "errors")),
        int((out["start"] > 0).sum()) >= 10,
    ]
    bad = [i for i, ok in enumerate(checks) if not ok]
    assert not bad, f"the case does not hold checks {bad}"
    return len(checks)
