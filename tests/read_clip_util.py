"""The clipping rule of include/sdt_gpu.h (sdt_gpu_clip_reads) restated in plain Python: what the tests of the kernel, the ABI and
`sdt-kmers clip` expect.  Positions are walked one by one and compared base by base as numpy arrays; no windows, no chunks, no
ballots.  Nothing here touches the library under test.  Also the one case of tests/test_read_clip.py, built here so that the host
tests can say that it holds what it promises."""
import functools

import numpy as np

from read_dedup_util import concat
from read_select_util import LETTERS

CLIP_FIELDS = ("adapters", "tail3", "tail5", "start", "len", "verdict")
CLIP_DTYPE = np.dtype([(f, np.uint32) for f in CLIP_FIELDS])
WHOLE, CLIPPED, DROPPED = 0, 2, 3
A, C, T, G = range(4)
PARAM_FIELDS = ("min_overlap", "max_err_pct", "min_len", "min_tail", "tail_err_pct", "tail3_bases", "tail5_bases", "flags")
# the defaults of `sdt-kmers clip`
DEFAULTS = dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=0, tail5_bases=0, flags=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS)
    return p


def hit3(read, a, min_overlap, pct):
    """the smallest p at which 3' adapter a hits, or None"""
    L, m = len(read), len(a)
    for p in range(L):
        o = min(m, L - p)
        if o < min_overlap:
            break                                         # (o only shrinks from here)
        if 100 * int((read[p:p + o] != a[:o]).sum()) <= pct * o:
            return p
    return None


def hit5(read, a, min_overlap, pct):
    """the largest e at which 5' adapter a hits, or None"""
    m = len(a)
    for e in range(len(read), 0, -1):
        o = min(m, e)
        if o < min_overlap:
            break
        if 100 * int((read[e - o:e] != a[m - o:]).sum()) <= pct * o:
            return e
    return None


def tail(seg, b, min_tail, pct):
    """the 3' tail of base b on the segment (for the 5' tail: on the reversed segment)"""
    n, x, best = len(seg), 0, None
    for t in range(1, n + 1):
        c = int(seg[n - t])
        x += c != b
        if c == b and t >= min_tail and 100 * x <= pct * t:
            score = t - 3 * x
            if best is None or score > best[0]:
                best = (score, t)
    return best[1] if best else 0


def clip_read(read, adapters, p):
    """-> (adapters, tail3, tail5, start, len, verdict)"""
    read = np.asarray(read, dtype=np.uint8)
    L = len(read)
    s0, e0, a3, a5 = 0, L, 0, 0
    for i, (a, end) in enumerate(adapters):
        a = np.asarray(a, dtype=np.uint8)
        if end == 0:
            h = hit3(read, a, p["min_overlap"], p["max_err_pct"])
            if h is not None and (a3 == 0 or h < e0):
                e0, a3 = h, i + 1
        else:
            h = hit5(read, a, p["min_overlap"], p["max_err_pct"])
            if h is not None and (a5 == 0 or h > s0):
                s0, a5 = h, i + 1
    t3 = t5 = 0
    if s0 < e0:
        t3 = max([tail(read[s0:e0], b, p["min_tail"], p["tail_err_pct"]) for b in range(4) if p["tail3_bases"] >> b & 1], default=0)
        t5 = max([tail(read[s0:e0 - t3][::-1], b, p["min_tail"], p["tail_err_pct"]) for b in range(4) if p["tail5_bases"] >> b & 1], default=0)
    start = s0 + t5
    ln = max(0, e0 - t3 - start)
    if ln < max(p["min_len"], 1):
        return (a3 | a5 << 16, t3, t5, 0, 0, DROPPED)
    return (a3 | a5 << 16, t3, t5, start, ln, WHOLE if ln == L else CLIPPED)


def expect_clip(codes, offs, adapters, p, ordinals=None):
    """-> (records, keep uint8[], reads with len > 0); with ordinals: record ordinals[r] is read r's, the others are zero"""
    n = len(offs) - 1
    idx = list(range(n)) if ordinals is None else [int(o) for o in ordinals]
    size = (max(idx) + 1) if idx else 0
    clip = np.zeros(size, dtype=CLIP_DTYPE)
    for r in range(n):
        clip[idx[r]] = clip_read(codes[int(offs[r]):int(offs[r + 1])], adapters, p)
    keep = (clip["len"] > 0).astype(np.uint8)
    return clip, keep, int(keep.sum())


def clipped_reads(codes, offs, clip):
    """the reads that compact_trimmed makes of the records"""
    return [codes[int(offs[r]) + int(c["start"]):int(offs[r]) + int(c["start"]) + int(c["len"])] for r, c in enumerate(clip) if c["len"]]


def assert_clip_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names == CLIP_FIELDS
    assert got.shape == want.shape, f"{what}: {got.shape} records, {want.shape} expected"
    for f in CLIP_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def shift_adapter_ids(clip, by):
    """the records as they are when `by` adapters stand in front of the set (and bound no read themselves)"""
    out = clip.copy()
    a3, a5 = clip["adapters"] & 0xFFFF, clip["adapters"] >> 16
    out["adapters"] = np.where(a3 > 0, a3 + by, 0) | np.where(a5 > 0, a5 + by, 0) << 16
    return out


# ---- `sdt-kmers clip` ---------------------------------------------------------------------------------------------------------------
def fasta_of(named):
    """adapters [(name, codes)] as a FASTA text"""
    return "".join(f">{name}\n{''.join(LETTERS[int(b)] for b in a)}\n" for name, a in named)


def cli_texts(codes, offs, clip, pair_ranges, names, ends):
    """the four files of `sdt-kmers clip` for a stream in ordinal order: (readClip, pairs.fa, single.fa, clipStats)"""
    n = len(offs) - 1
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
    rec_txt = "".join(f"{int(c['adapters']) & 0xFFFF} {int(c['adapters']) >> 16} {c['tail3']} {c['tail5']} {c['start']} {c['len']} {c['verdict']}\n"
                      for c in clip)
    mate = {}
    for first, end in pair_ranges:
        for r in range(first, end, 2):
            mate[r], mate[r + 1] = r + 1, r
    pairs, single = [], []
    for r in range(n):
        if clip["len"][r]:
            s = int(offs[r]) + int(clip["start"][r])
            both = r in mate and clip["len"][mate[r]] > 0
            (pairs if both else single).append(f">{r + 1}\n{letters[s:s + int(clip['len'][r])]}\n")
    reads, bases = [0] * len(names), [0] * len(names)
    tails = {"tail3": [0, 0], "tail5": [0, 0]}
    for r, c in enumerate(clip):
        L = int(offs[r + 1]) - int(offs[r])
        a3, a5 = int(c["adapters"]) & 0xFFFF, int(c["adapters"]) >> 16
        # what the adapters left is [s0, e0); the record of a dropped read does not say it, so its bases are not counted
        live = c["verdict"] != DROPPED
        e0 = int(c["start"]) + int(c["len"]) + int(c["tail3"]) if live else L
        s0 = int(c["start"]) - int(c["tail5"]) if live else 0
        if a3:
            reads[a3 - 1] += 1
            bases[a3 - 1] += L - e0
        if a5:
            reads[a5 - 1] += 1
            bases[a5 - 1] += s0
        for f in ("tail3", "tail5"):
            if c[f]:
                tails[f][0] += 1
                tails[f][1] += int(c[f])
    stats = "".join(f"{i + 1} {names[i]} {3 if ends[i] == 0 else 5} {reads[i]} {bases[i]}\n" for i in range(len(names)))
    stats += "".join(f"{f} {tails[f][0]} {tails[f][1]}\n" for f in ("tail3", "tail5"))
    v = clip["verdict"]
    stats += f"whole {int((v == WHOLE).sum())}\nclipped {int((v == CLIPPED).sum())}\ndropped {int((v == DROPPED).sum())}\n"
    return rec_txt, "".join(pairs), "".join(single), stats


def expect_cli(codes, offs, named, ends, p, pair_ranges):
    """the records and the four texts from the rule alone"""
    clip = expect_clip(codes, offs, [(a, e) for (_, a), e in zip(named, ends)], p)[0]
    return clip, cli_texts(codes, offs, clip, pair_ranges, [n for n, _ in named], ends)


# ---- the case of tests/test_read_clip.py ----------------------------------------------------------------------------------------------
CASE_PARAMS = params(min_overlap=5, max_err_pct=10, min_len=20, min_tail=6, tail_err_pct=20, tail3_bases=1 << A, tail5_bases=1 << T)


def _mutate(a, where):
    a = np.array(a, dtype=np.uint8)
    for k in where:
        a[k] = (a[k] + 1) & 3
    return a


@functools.lru_cache(maxsize=None)
def case():
    """About 120 reads with planted adapters and tails, each under a name that says what it is there for; built once from a fixed
    seed and left unchanged.  3' adapters start with C or G and 5' adapters end with C or G, so that a planted tail next to an adapter
    cannot be taken for a part of it."""
    rng = np.random.default_rng(20241018)

    def rnd(n):                                           # bases that end and start away from A and T: no chance tail joins a planted one
        r = rng.integers(0, 4, size=n, dtype=np.uint8)
        if n:
            r[0], r[-1] = (C, G)[int(rng.integers(0, 2))], (C, G)[int(rng.integers(0, 2))]
        return r

    def adapter(n):
        return rnd(n)

    a3 = {m: adapter(m) for m in (31, 32, 33, 64, 65, 128)}
    b5 = {m: adapter(m) for m in (31, 33, 64, 128)}
    adapters = [(a3[m], 0) for m in (31, 32, 33, 64, 65, 128)]                 # 0 .. 5
    adapters.append((a3[33][:20].copy(), 0))                                   # 6: hits wherever adapter 2 hits with >= 20 bases: the lower index wins
    adapters += [(b5[m], 1) for m in (31, 33, 64, 128)]                        # 7 .. 10
    adapters.append((b5[33][-15:].copy(), 1))                                  # 11: the same for adapter 8
    mo, ml = CASE_PARAMS["min_overlap"], CASE_PARAMS["min_len"]
    As, Ts = (lambda n: np.full(n, A, dtype=np.uint8)), (lambda n: np.full(n, T, dtype=np.uint8))
    cat = lambda *parts: np.concatenate([np.asarray(x, dtype=np.uint8) for x in parts]).astype(np.uint8)
    named = [
        ("3' at p=0", cat(a3[31], rnd(20))),
        ("3' at p=1", cat(rnd(1), a3[32], rnd(5))),
        ("3' at p=63", cat(rnd(63), a3[33][:30])),
        ("3' at p=64", cat(rnd(64), a3[64])),
        ("3' at p=65", cat(rnd(65), a3[65], rnd(3))),
        ("3' at L-min_overlap", cat(rnd(80), a3[128][:mo])),
        ("3' at L-min_overlap+1", cat(rnd(80), a3[128][:mo - 1])),
        ("3' on budget", cat(rnd(40), _mutate(a3[64], (3, 17, 31, 32, 40, 63)))),                # 6 of 64: 600 <= 640
        ("3' over budget", cat(rnd(40), _mutate(a3[64], (3, 17, 31, 32, 40, 50, 63)))),          # 7 of 64
        ("3' o=9 one mismatch", cat(rnd(70), _mutate(a3[65][:9], (4,)))),                        # budget 0
        ("3' o=10 one mismatch", cat(rnd(70), _mutate(a3[65][:10], (4,)))),                      # budget 1
        ("3' tie of adapters", cat(rnd(50), a3[33])),
        ("5' at e=min_overlap-1", cat(b5[33][-(mo - 1):], rnd(80))),
        ("5' at e=min_overlap", cat(b5[33][-mo:], rnd(80))),
        ("5' at e=64", cat(b5[64], rnd(60))),
        ("5' at e=65", cat(b5[128][-65:], rnd(50))),
        ("5' at e=L", cat(rnd(7), b5[31])),
        ("5' tie of adapters", cat(b5[33][-20:], rnd(60))),
        ("crossing", cat(rnd(10), a3[31], rnd(10), b5[31], rnd(10))),
        ("empty", np.zeros(0, dtype=np.uint8)),
        ("one base", np.array([G], dtype=np.uint8)),
        ("shorter than min_overlap", rnd(mo - 1)),
        ("min_len-1 left", cat(rnd(ml - 1), a3[32])),
        ("min_len left", cat(rnd(ml), a3[32])),
        ("5000 bases", cat(rnd(4700), a3[33], rnd(267))),
        ("pure A tail", cat(rnd(80), As(15))),
        ("A tail, tie in score", cat(rnd(70), [C], [A, A, C], As(7))),
        ("A tail of 70", cat(rnd(40), As(70))),
        ("A tail of 141", cat(rnd(40), As(60), [G], As(80))),
        ("all A", As(90)),
        ("T head before 5' remnant", cat(b5[33][-12:], Ts(9), rnd(70))),
        ("A tail before 3' adapter", cat(rnd(60), As(20), a3[33][:25])),
        ("both ends", cat(b5[64][-30:], Ts(12), rnd(50), As(11), a3[128][:40])),
    ]
    names = [n for n, _ in named]
    reads = [r for _, r in named]
    while len(reads) < 120:                               # reads of the transcript alone, with whatever 5-base overlaps chance gives
        names.append("plain")
        reads.append(rnd(int(rng.integers(30, 160))))
    order = rng.permutation(len(reads))
    reads, names = [reads[i] for i in order], [names[i] for i in order]
    codes, offs = concat(reads)
    return dict(reads=reads, names=names, codes=codes, offs=offs, adapters=adapters, params=CASE_PARAMS)


@functools.lru_cache(maxsize=None)
def case_expect():
    """the records of the case under its own parameters, by the rule: computed once, shared by the tests, left unchanged"""
    c = case()
    return expect_clip(c["codes"], c["offs"], c["adapters"], c["params"])


def case_holds():
    """the case contains what its names promise, by the rule: -> the number of checks made"""
    c = case()
    clip = case_expect()[0]
    rec = {n: clip[i] for i, n in enumerate(c["names"]) if n != "plain"}
    L = {n: len(c["reads"][i]) for i, n in enumerate(c["names"]) if n != "plain"}
    mo, ml = c["params"]["min_overlap"], c["params"]["min_len"]
    a3 = lambda n: int(rec[n]["adapters"]) & 0xFFFF
    a5 = lambda n: int(rec[n]["adapters"]) >> 16
    end = lambda n: int(rec[n]["start"]) + int(rec[n]["len"]) + int(rec[n]["tail3"])     # e0 of a read that is not dropped
    checks = [
        a3("3' at p=0") == 1 and rec["3' at p=0"]["verdict"] == DROPPED,
        a3("3' at p=1") == 2 and rec["3' at p=1"]["verdict"] == DROPPED,
        (a3("3' at p=63"), end("3' at p=63")) == (3, 63),
        (a3("3' at p=64"), end("3' at p=64")) == (4, 64),
        (a3("3' at p=65"), end("3' at p=65")) == (5, 65),
        (a3("3' at L-min_overlap"), end("3' at L-min_overlap")) == (6, L["3' at L-min_overlap"] - mo),
        a3("3' at L-min_overlap+1") == 0 and rec["3' at L-min_overlap+1"]["verdict"] == WHOLE,
        (a3("3' on budget"), end("3' on budget")) == (4, 40),
        a3("3' over budget") == 0,
        a3("3' o=9 one mismatch") == 0,
        (a3("3' o=10 one mismatch"), end("3' o=10 one mismatch")) == (5, 70),
        (a3("3' tie of adapters"), end("3' tie of adapters")) == (3, 50),
        hit3(c["reads"][c["names"].index("3' tie of adapters")], c["adapters"][6][0], mo, 10) == 50,
        a5("5' at e=min_overlap-1") == 0,
        (a5("5' at e=min_overlap"), int(rec["5' at e=min_overlap"]["start"])) == (9, mo),
        (a5("5' at e=64"), int(rec["5' at e=64"]["start"])) == (10, 64),
        (a5("5' at e=65"), int(rec["5' at e=65"]["start"])) == (11, 65),
        a5("5' at e=L") == 8 and rec["5' at e=L"]["verdict"] == DROPPED,
        (a5("5' tie of adapters"), int(rec["5' tie of adapters"]["start"])) == (9, 20),
        hit5(c["reads"][c["names"].index("5' tie of adapters")], c["adapters"][11][0], mo, 10) == 20,
        (a3("crossing"), a5("crossing")) == (1, 8) and rec["crossing"].tolist() == (1 | 8 << 16, 0, 0, 0, 0, DROPPED),
        rec["empty"].tolist() == (0, 0, 0, 0, 0, DROPPED),
        rec["one base"].tolist() == (0, 0, 0, 0, 0, DROPPED),                    # (1 base, min_len = 20)
        rec["shorter than min_overlap"]["verdict"] == DROPPED,
        rec["min_len-1 left"].tolist() == (2, 0, 0, 0, 0, DROPPED),
        rec["min_len left"].tolist() == (2, 0, 0, 0, ml, CLIPPED),
        rec["5000 bases"].tolist()[3:] == (0, 4700, CLIPPED) and a3("5000 bases") == 3,
        rec["pure A tail"].tolist() == (0, 15, 0, 0, 80, CLIPPED),
        rec["A tail, tie in score"].tolist() == (0, 7, 0, 0, 74, CLIPPED),
        rec["A tail of 70"].tolist() == (0, 70, 0, 0, 40, CLIPPED),
        rec["A tail of 141"].tolist() == (0, 141, 0, 0, 40, CLIPPED),
        rec["all A"].tolist() == (0, 90, 0, 0, 0, DROPPED),
        rec["T head before 5' remnant"].tolist() == (9 << 16, 0, 9, 21, 70, CLIPPED),
        rec["A tail before 3' adapter"].tolist() == (3, 20, 0, 0, 60, CLIPPED),
        rec["both ends"].tolist() == (6 | 10 << 16, 11, 12, 42, 50, CLIPPED),
        {WHOLE, CLIPPED, DROPPED} == set(clip["verdict"].tolist()),
        int((clip["verdict"] == WHOLE).sum()) >= 60,
    ]
    bad = [i for i, ok in enumerate(checks) if not ok]
    assert not bad, f"the case does not hold checks {bad}"
    return len(checks)
