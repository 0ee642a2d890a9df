"""The rule of sdt_gpu_qc_reads (include/sdt_gpu.h) restated in numpy: a loop over the reads, np.add.at per read, nothing from the
library.  expect_loop is a second restatement, one base at a time in plain Python, which the first is held to on the CPU
(test_read_qc_host.py).  The case the GPU tests share is built here once and left unchanged."""
import functools

import numpy as np

import __graft_entry__ as ge
import read_quality_util as qu
from read_dedup_util import concat

TILE = ge.load_package().QC_TILE                         # rows of the kernel's LDS tile (the binding only: no library is loaded here)
QUALS, GC_BINS, TOTALS = 94, 101, 8
FROM_END = 1
RANGE_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "weak", "median", "start", "len", "verdict")])   # sdt_read_trim
CASE_C = 150
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, CASE_C - 1, CASE_C, CASE_C + 1, CASE_C + 300)


def report_words(cycles):
    return 203 + 99 * (cycles + 1)


def sections(report, cycles):
    """views into a flat report, by the table of the rule"""
    R = cycles + 1
    assert report.dtype == np.uint64 and report.size >= report_words(cycles)
    cuts = np.cumsum([0, TOTALS, 4 * R, QUALS * R, R, GC_BINS, QUALS])
    names = ("totals", "base", "qual", "len", "gc", "meanq")
    shapes = ((TOTALS,), (R, 4), (R, QUALS), (R,), (GC_BINS,), (QUALS,))
    return {n: report[a:b].reshape(s) for n, a, b, s in zip(names, cuts[:-1], cuts[1:], shapes)}


def quality_of(byte, phred_offset):
    byte = np.asarray(byte, dtype=np.int64)
    return np.where(byte < phred_offset, 0, np.minimum(byte - phred_offset, 93))


def counted_range(L, ranges, r, clamp):
    """(s, n, whether the range had to be clamped)"""
    if ranges is None:
        return 0, L, False
    s, n, clamped = int(ranges["start"][r]), int(ranges["len"][r]), False
    if not clamp:
        assert s + n <= L, f"read {r}: the host form refuses this range"
        return s, n, False
    if s > L:
        s, clamped = L, True
    if n > L - s:
        n, clamped = L - s, True
    return s, n, clamped


def expect(codes, offs, quals=None, ranges=None, classes=None, cycles=CASE_C, phred_offset=33, flags=0, class_sel=0, clamp=False, report=None,
           reads=None):
    """the report after the call: `report` (or zeros) plus the batch; clamp: the device form's treatment of a range; reads: only these"""
    C = cycles
    rep = np.zeros(report_words(C), dtype=np.uint64) if report is None else report.copy()
    sec = sections(rep, C)
    codes = np.asarray(codes, dtype=np.int64)
    for r in (range(len(offs) - 1) if reads is None else reads):
        if classes is not None and int(classes[r]) != class_sel:
            sec["totals"][3] += 1
            continue
        o0, L = int(offs[r]), int(offs[r + 1]) - int(offs[r])
        s, n, clamped = counted_range(L, ranges, r, clamp)
        sec["totals"][4] += int(clamped)
        sec["totals"][0] += 1
        sec["totals"][2] += n
        if n == 0:
            sec["totals"][1] += 1
            sec["len"][0] += 1
            continue
        b = codes[o0 + s:o0 + s + n]
        i = np.arange(n, dtype=np.int64)
        row = np.minimum(n - 1 - i if flags & FROM_END else i, C)
        np.add.at(sec["base"], (row, b), 1)
        sec["len"][min(n, C)] += 1
        sec["gc"][100 * int(((b == 1) | (b == 3)).sum()) // n] += 1
        if quals is not None:
            q = quality_of(quals[o0 + s:o0 + s + n], phred_offset)
            np.add.at(sec["qual"], (row, q), 1)
            sec["meanq"][int(q.sum()) // n] += 1
    return rep


def expect_loop(codes, offs, quals=None, ranges=None, classes=None, cycles=CASE_C, phred_offset=33, flags=0, class_sel=0, clamp=False):
    """the same one base at a time, in plain integers"""
    C, R = cycles, cycles + 1
    totals, base, qual = [0] * TOTALS, [[0] * 4 for _ in range(R)], [[0] * QUALS for _ in range(R)]
    lens, gc, meanq = [0] * R, [0] * GC_BINS, [0] * QUALS
    for r in range(len(offs) - 1):
        if classes is not None and int(classes[r]) != class_sel:
            totals[3] += 1
            continue
        o0, L = int(offs[r]), int(offs[r + 1]) - int(offs[r])
        s, n, clamped = counted_range(L, ranges, r, clamp)
        totals[4] += int(clamped)
        totals[0] += 1
        totals[2] += n
        lens[min(n, C)] += 1
        if n == 0:
            totals[1] += 1
            continue
        cg = sq = 0
        for i in range(n):
            row = min(n - 1 - i if flags & FROM_END else i, C)
            code = int(codes[o0 + s + i])
            base[row][code] += 1
            cg += code in (1, 3)
            if quals is not None:
                byte = int(quals[o0 + s + i])
                q = 0 if byte < phred_offset else min(byte - phred_offset, 93)
                qual[row][q] += 1
                sq += q
        gc[100 * cg // n] += 1
        if quals is not None:
            meanq[sq // n] += 1
    flat = totals + [x for row in base for x in row] + [x for row in qual for x in row] + lens + gc + meanq
    return np.array(flat, dtype=np.uint64)


def identities(report, cycles, with_quals, forward_lengths=None):
    """what holds for any input, asserted on a report that started from zero; forward_lengths: the n of the counted reads (flags = 0)"""
    s = sections(report, cycles)
    t = s["totals"]
    assert int(s["base"].sum()) == int(t[2])
    assert int(s["qual"].sum()) == (int(t[2]) if with_quals else 0)
    assert int(s["len"].sum()) == int(t[0])
    assert int(s["gc"].sum()) == int(t[0]) - int(t[1])
    assert int(s["meanq"].sum()) == (int(t[0]) - int(t[1]) if with_quals else 0)
    assert t[5:].tolist() == [0, 0, 0]
    if forward_lengths is not None:
        n = np.asarray(forward_lengths, dtype=np.int64)
        assert s["base"][:cycles].sum(axis=1).tolist() == [int((n > c).sum()) for c in range(cycles)]


def assert_report(got, want, cycles, what=""):
    assert got.dtype == np.uint64 and got.shape == want.shape, f"{what}: {got.shape} words, {want.shape} expected"
    if (got == want).all():
        return
    g, w = sections(got, cycles), sections(want, cycles)
    for name in g:
        bad = np.argwhere(g[name] != w[name])
        assert bad.size == 0, (f"{what}: section {name} differs at {bad[:6].tolist()}: got {[int(g[name][tuple(i)]) for i in bad[:6]]} "
                               f"want {[int(w[name][tuple(i)]) for i in bad[:6]]}")


def pack(synth, codes):
    """the 2-bit words of a stream, with the pad words every host form asks for"""
    return synth.pack_2bit(np.asarray(codes, dtype=np.uint8))


def case_quals(rng, L, i):
    """realistic qualities at offset 33, with bytes below the offset and above offset + 93 in some reads"""
    q = (qu.realistic(rng, L, i) + 33).astype(np.uint8)
    if L and i % 5 == 0:
        q[rng.integers(0, L, 1 + L // 40)] = rng.integers(0, 33, 1 + L // 40)
    if L and i % 6 == 0:
        q[rng.integers(0, L, 1 + L // 40)] = rng.integers(33 + 94, 256, 1 + L // 40)
    return q


@functools.lru_cache(maxsize=None)
def case():
    """about 400 reads: every length of LENGTHS several times, one read of 1 000 and one of 5 000 bases; ranges with start > 0, with
    len = 0 and whole; classes 0, 1, 2"""
    rng = np.random.default_rng(20)
    lens = list(LENGTHS) * 19 + [int(x) for x in rng.choice(LENGTHS, 18)]
    rng.shuffle(lens)
    lens[37], lens[211] = 1000, 5000
    reads = [rng.integers(0, 4, L).astype(np.uint8) for L in lens]
    quals = [case_quals(rng, L, i) for i, L in enumerate(lens)]
    codes, offs = concat(reads)
    qbytes, qoffs = qu.concat_bytes(quals)
    assert qoffs.tolist() == offs.tolist()
    ranges = np.zeros(len(lens), dtype=RANGE_DTYPE)
    ranges["kmers"], ranges["weak"], ranges["median"], ranges["verdict"] = 0xDEADBEEF, 0xFFFFFFFF, 7, 9      # never read
    for r, L in enumerate(lens):
        kind = r % 4
        if kind == 0 or L == 0:
            s, n = 0, L                                    # whole
        elif kind == 1:
            s, n = int(rng.integers(0, L + 1)), 0          # nothing kept
        elif kind == 2:
            s = int(rng.integers(1, L + 1))                # a start inside the read, up to its end
            n = int(rng.integers(0, L - s + 1))
        else:
            s = int(rng.integers(0, min(L, 8) + 1))        # both ends cut a little
            n = L - s - int(rng.integers(0, min(L - s, 8) + 1))
        ranges["start"][r], ranges["len"][r] = s, n
    classes = rng.integers(0, 3, len(lens)).astype(np.uint8)
    for a in (codes, offs, qbytes, ranges, classes):
        a.setflags(write=False)
    return dict(codes=codes, offs=offs, quals=qbytes, ranges=ranges, classes=classes, reads=reads, qreads=quals, lens=np.array(lens))


def case_holds():
    c = case()
    lens, rg = c["lens"], c["ranges"]
    for L in LENGTHS + (1000, 5000):
        assert (lens == L).sum() >= 1, L
    assert len(lens) >= 390
    assert (rg["len"] == 0).sum() >= 20 and (rg["start"] > 0).sum() >= 50 and ((rg["start"] == 0) & (rg["len"] == lens) & (lens > 0)).sum() >= 50
    assert (rg["len"] > CASE_C).sum() >= 30 and (lens > CASE_C).sum() >= 30                # reach row C, with and without the ranges
    q = c["quals"]
    assert (q < 33).sum() >= 20 and (q > 33 + 93).sum() >= 20
    assert all((c["classes"] == k).sum() >= 100 for k in (0, 1, 2))
    return int((rg["len"] == 0).sum())


@functools.lru_cache(maxsize=None)
def _case_expect(with_quals, with_ranges, with_classes, cycles, phred_offset, flags, class_sel):
    c = case()
    rep = expect(c["codes"], c["offs"], c["quals"] if with_quals else None, c["ranges"] if with_ranges else None,
                 c["classes"] if with_classes else None, cycles, phred_offset, flags, class_sel)
    rep.setflags(write=False)
    return rep


def case_expect(quals=True, ranges=True, classes=False, cycles=CASE_C, phred_offset=33, flags=0, class_sel=0):
    return _case_expect(quals, ranges, classes, cycles, phred_offset, flags, class_sel)


def case_args(quals=True, ranges=True, classes=False):
    c = case()
    return dict(quals=c["quals"] if quals else None, ranges=c["ranges"] if ranges else None, classes=c["classes"] if classes else None)


# ---- the kernel's walk, restated: what a lane loads and counts, pass by pass (csrc/sdt_qc_kernels.cuh) ---------------------------------
def lane_walk(words, qbuf, offs, ranges=None, classes=None, cycles=CASE_C, phred_offset=33, flags=0, class_sel=0, delta=0, blocks=2, waves=16,
              tile=TILE, touched=None):
    """The report of k_qc_reads as its lanes compute it: a workgroup's reads by the stride, one pass per tile of rows, a lane's 4 bytes
    from an aligned 32-bit word with the edges masked, its bases from one or two 2-bit words, the tile flushed after every pass and the
    loop left at min(longest n, C).  touched: a dict that collects the indices of the words and quality words that were loaded"""
    C = cycles
    rep = np.zeros(report_words(C), dtype=np.uint64)
    sec = sections(rep, C)
    from_end = bool(flags & FROM_END)
    nreads = len(offs) - 1
    words = [int(x) for x in words]
    for blk in range(blocks):
        t0, lds_longest = 0, 0
        rowC = [0] * 98
        while True:
            t1 = C if C - t0 < tile else t0 + tile
            lds = np.zeros((tile, 99), dtype=np.int64)
            for r in range(blk * waves, nreads, blocks * waves):
                for r in range(r, min(r + waves, nreads)):                  # the wavefronts of the workgroup
                    if classes is not None and int(classes[r]) != class_sel:
                        sec["totals"][3] += t0 == 0
                        continue
                    o0, L = int(offs[r]), int(offs[r + 1]) - int(offs[r])
                    s, n, clamped = counted_range(L, ranges, r, True)
                    if t0 == 0:
                        sec["totals"][4] += int(clamped)
                        sec["totals"][0] += 1
                        sec["totals"][2] += n
                        if n == 0:
                            sec["totals"][1] += 1
                            sec["len"][0] += 1
                            continue
                        i_lo, i_hi = 0, n
                    elif n > t0:
                        i_lo, i_hi = ((n - t1 if n > t1 else 0), n - t0) if from_end else (t0, min(n, t1))
                    else:
                        continue
                    assert i_lo < i_hi
                    b0 = o0 + s
                    q0 = b0 + delta
                    lo, hi = q0 + i_lo, q0 + i_hi
                    gc = sq = 0
                    for lane in range(64):
                        p = (lo & ~3) + 4 * lane
                        while p < hi:
                            kf, kl = (lo - p if p < lo else 0), (hi - p if hi - p < 4 else 4)
                            assert 0 <= kf < kl <= 4 and p % 4 == 0 and p >= 0
                            w = 0
                            if qbuf is not None:
                                w = int.from_bytes(bytes(qbuf[p:p + 4]), "little")
                                if touched is not None:
                                    touched.setdefault("quals", set()).add(p // 4)
                            bb = p - delta
                            wlo, whi = (bb + kf) >> 4, (bb + kl - 1) >> 4
                            xlo = words[wlo]
                            xhi = words[whi] if whi != wlo else xlo
                            if touched is not None:
                                touched.setdefault("words", set()).update((wlo, whi))
                            for k in range(kf, kl):
                                b, i = bb + k, p + k - q0
                                code = ((xlo if (b >> 4) == wlo else xhi) >> (30 - 2 * (b & 15))) & 3
                                byte = (w >> (8 * k)) & 255
                                q = 0 if byte < phred_offset else min(byte - phred_offset, 93)
                                rw = n - 1 - i if from_end else i
                                if t0 == 0:
                                    gc += code & 1
                                    sq += q
                                    if rw >= C:
                                        rowC[code] += 1
                                        if qbuf is not None:
                                            rowC[4 + q] += 1
                                        continue
                                    if rw >= tile:
                                        continue
                                assert 0 <= rw - t0 < tile
                                lds[rw - t0, code] += 1
                                if qbuf is not None:
                                    lds[rw - t0, 4 + q] += 1
                            p += 256
                    if t0 == 0:
                        nc = min(n, C)
                        lds_longest = max(lds_longest, nc)
                        sec["len"][nc] += 1
                        sec["gc"][100 * gc // n] += 1
                        if qbuf is not None:
                            sec["meanq"][sq // n] += 1
            lim = lds_longest
            rows = 0 if lim <= t0 else min(lim - t0, tile)
            assert int(lds[rows:].sum()) == 0 and int(lds[:, 98].sum()) == 0, "a counter outside the rows that are flushed"
            for rr in range(rows):
                sec["base"][t0 + rr] += lds[rr, :4].astype(np.uint64)
                sec["qual"][t0 + rr] += lds[rr, 4:98].astype(np.uint64)
            if t0 == 0:
                sec["base"][C] += np.array(rowC[:4], dtype=np.uint64)
                sec["qual"][C] += np.array(rowC[4:], dtype=np.uint64)
            if t1 >= lim:
                break
            t0 += tile
    return rep


# ---- `sdt-kmers qc` ---------------------------------------------------------------------------------------------------------------------
def percentile(hist, p):
    """the smallest q whose cumulative count is >= ceil(p N / 100)"""
    n = int(hist.sum())
    need = max(-(-p * n // 100), 1)
    return int(np.nonzero(np.cumsum(hist.astype(object)) >= need)[0][0])


def cli_texts(reports, with_quals, cycles):
    """reports: {class: report}, with_quals: {class: bool} -> (qcBases, qcQuals, qcReads, the stdout lines) as `sdt-kmers qc` writes them"""
    C = cycles
    name = lambda r: f"{r}+" if r == C else f"{r}"
    bases, quals, reads, lines = ["# class row reads A C T G\n"], ["# class row bases mean_x100 min q10 q25 median q75 q90 max\n"], ["# hist class bin reads\n"], []
    hist = {"len": [], "gc": [], "meanq": []}
    for k in sorted(reports):
        s = {n: v.astype(object) for n, v in sections(reports[k], C).items()}
        for r in range(C + 1):
            b = s["base"][r]
            if b.sum():
                bases.append(f"{k} {name(r)} {b.sum()} {b[0]} {b[1]} {b[2]} {b[3]}\n")
        if not with_quals[k]:
            quals.append(f"# class {k}: no qualities\n")
        for r in range(C + 1 if with_quals[k] else 0):
            h = s["qual"][r]
            n = h.sum()
            if n:
                nz = np.nonzero(h)[0]
                mean = 100 * int((h * np.arange(QUALS)).sum()) // int(n)
                quals.append(f"{k} {name(r)} {n} {mean} {nz[0]} " + " ".join(str(percentile(h, p)) for p in (10, 25, 50, 75, 90)) + f" {nz[-1]}\n")
        hist["len"] += [f"len {k} {name(i)} {v}\n" for i, v in enumerate(s["len"]) if v]
        hist["gc"] += [f"gc {k} {i} {v}\n" for i, v in enumerate(s["gc"]) if v]
        hist["meanq"] += [f"meanq {k} {i} {v}\n" for i, v in enumerate(s["meanq"]) if v] if with_quals[k] else [f"# meanq class {k}: no qualities\n"]
        t, nq = s["totals"], int(s["qual"].sum())
        cg = int(s["base"][:, 1].sum() + s["base"][:, 3].sum())
        line = f"qc: class {k} reads {t[0]} empty {t[1]} bases {t[2]} gc {10000 * cg // int(t[2]) if t[2] else 0}"
        if with_quals[k] and nq:
            line += f" q20 {10000 * int(s['qual'][:, 20:].sum()) // nq} q30 {10000 * int(s['qual'][:, 30:].sum()) // nq}\n"
        else:
            line += " q20 - q30 -\n"
        lines.append(line)
    return "".join(bases), "".join(quals), "".join(reads + hist["len"] + hist["gc"] + hist["meanq"]), "".join(lines)
