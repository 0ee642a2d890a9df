"""GPU (-m gpu): sdt_gpu_qc_reads and its device form against the numpy restatement of the rule (read_qc_util.py).  Every count is
compared for exact equality; no expectation comes from the library under test."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import read_qc_util as qc
import read_quality_util as qu
from read_dedup_util import concat
from test_read_stage_strides import WAVE_BLOCKS, assert_strides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31
CYCLES = (1, 7, 150, 151, 1024, 4096)
WAVES = 16                                               # wavefronts of a workgroup of k_qc_reads (csrc/sdt_read_plan.h: QC_WAVES)


def dev(a):
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(np.array(a).view(signed)).cuda()                # (a copy: the case's arrays are read-only)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).copy()


def case_words(synth):
    return qc.pack(synth, qc.case()["codes"])


def run_case(g, synth, report=None, reads=None, **kw):
    """the host form on the case (or on reads [a, b) of it) under the variant kw of read_qc_util.case_expect"""
    c = qc.case()
    sel = {k: kw.pop(k, d) for k, d in (("quals", True), ("ranges", True), ("classes", False))}
    a = qc.case_args(**sel)
    offs = c["offs"]
    if reads is not None:
        lo, hi = reads
        offs = offs[lo:hi + 1]
        a = {k: (v if v is None or k == "quals" else v[lo:hi]) for k, v in a.items()}
    return g.qc_reads(case_words(synth), offs, params=kw, report=report, **a)


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
def test_qc_equals_the_rule(pkg, synth):
    """the case under six numbers of cycles in both directions; without qualities, without ranges, by class, under the three offsets"""
    assert qc.case_holds() >= 20 and pkg.QC_TILE == qc.TILE
    c = qc.case()
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for C in CYCLES:
            assert pkg.qc_report_words(C) == qc.report_words(C)
            for flags in (0, qc.FROM_END):
                got = run_case(g, synth, cycles=C, flags=flags)
                qc.assert_report(got, qc.case_expect(cycles=C, flags=flags), C, f"cycles = {C}, flags = {flags}")
                qc.identities(got, C, True, None if flags else c["ranges"]["len"])
        for flags in (0, qc.FROM_END):
            for C in (150, 7):
                for v in (dict(quals=False), dict(ranges=False), dict(quals=False, ranges=False), dict(phred_offset=0), dict(phred_offset=64),
                          dict(classes=True, class_sel=0), dict(classes=True, class_sel=1), dict(classes=True, class_sel=2),
                          dict(classes=True, class_sel=3)):
                    got = run_case(g, synth, cycles=C, flags=flags, **v)
                    qc.assert_report(got, qc.case_expect(cycles=C, flags=flags, **v), C, f"cycles = {C}, flags = {flags}, {v}")
                    qc.identities(got, C, v.get("quals", True))
        # the sections of the binding are the sections of the rule
        mine, theirs = pkg.qc_sections(got, 7), qc.sections(got, 7)
        assert list(mine) == list(theirs) and all(mine[k].shape == theirs[k].shape and (mine[k] == theirs[k]).all() for k in mine)
        mine["totals"][7] += np.uint64(5)
        assert got[7] == 5                                # views, not copies


# ---- 2. the call adds -----------------------------------------------------------------------------------------------------------------
def test_qc_adds_to_the_report(pkg, synth):
    c = qc.case()
    n = len(c["offs"]) - 1
    C = 150
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for v in (dict(), dict(quals=False), dict(flags=qc.FROM_END)):
            pattern = (np.arange(qc.report_words(C), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(8)
            got = run_case(g, synth, report=pattern.copy(), cycles=C, **v)
            assert (got == pattern + qc.case_expect(cycles=C, **v)).all(), f"{v}: pattern + expected"
            if not v.get("quals", True):                  # untouched, not rewritten
                s, p = qc.sections(got, C), qc.sections(pattern, C)
                assert (s["qual"] == p["qual"]).all() and (s["meanq"] == p["meanq"]).all()
        # two halves into one report
        half = n // 2 + 1
        for flags in (0, qc.FROM_END):
            rep = run_case(g, synth, reads=(0, half), cycles=C, flags=flags, classes=True, class_sel=1)
            rep = run_case(g, synth, report=rep, reads=(half, n), cycles=C, flags=flags, classes=True, class_sel=1)
            qc.assert_report(rep, qc.case_expect(cycles=C, flags=flags, classes=True, class_sel=1), C, "two halves")
        # three classes into one report: the call without classes, and every read passed over twice
        rep = None
        for k in (0, 1, 2):
            rep = run_case(g, synth, report=rep, cycles=C, classes=True, class_sel=k)
        whole = qc.case_expect(cycles=C).copy()
        assert rep[3] == 2 * n and whole[3] == 0
        whole[3] = 2 * n
        qc.assert_report(rep, whole, C, "three classes")


# ---- 3. where the reads start ---------------------------------------------------------------------------------------------------------
def test_qc_is_alignment_independent(pkg, synth):
    """one filler read of 0 .. 15 bases in front: every 2-bit phase and every byte phase; the host form with offsets[0] = 5; the device
    form on streams that start 1, 2 and 3 bases and bytes into their buffers"""
    import torch
    c = qc.case()
    n = len(c["offs"]) - 1
    C = 150
    rng = np.random.default_rng(3)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            filler, fq = rng.integers(0, 4, f).astype(np.uint8), rng.integers(33, 74, f).astype(np.uint8)
            codes, offs = concat([filler] + c["reads"])
            quals, _ = qu.concat_bytes([fq] + c["qreads"])
            ranges = np.concatenate([np.zeros(1, dtype=qc.RANGE_DTYPE), c["ranges"]])
            ranges["len"][0] = f
            flags = qc.FROM_END if f % 2 else 0
            first = qc.expect(filler, np.array([0, f], dtype=np.uint64), fq, cycles=C, flags=flags)
            want = first + qc.case_expect(cycles=C, flags=flags)
            got = g.qc_reads(qc.pack(synth, codes), offs, quals, ranges, params=dict(cycles=C, flags=flags))
            qc.assert_report(got, want, C, f"{f} filler bases")
        junk = rng.integers(0, 4, 5).astype(np.uint8)
        got = g.qc_reads(qc.pack(synth, np.concatenate([junk, c["codes"]])), c["offs"] + np.uint64(5), np.concatenate([np.full(5, 255, dtype=np.uint8), c["quals"]]),
                         c["ranges"], params=dict(cycles=C))
        qc.assert_report(got, qc.case_expect(cycles=C), C, "offsets[0] = 5")
        for lead in (1, 2, 3):
            d_w = dev(qc.pack(synth, np.concatenate([np.full(lead, 3, dtype=np.uint8), c["codes"]])))
            d_q = dev(np.concatenate([np.full(lead, 255, dtype=np.uint8), c["quals"], np.full(8, 255, dtype=np.uint8)]))
            d_o = dev(c["offs"] + np.uint64(lead))
            d_r = dev(np.ascontiguousarray(c["ranges"]).view(np.uint32))
            d_c = dev(c["classes"])
            d_rep = torch.zeros(qc.report_words(C), dtype=torch.int64, device="cuda:0")
            assert d_q.data_ptr() % 4 == 0 and d_rep.data_ptr() % 8 == 0
            torch.cuda.synchronize()
            g.qc_reads_device(d_w, d_o, n, d_rep, d_q, d_r, d_c, dict(cycles=C, class_sel=2, flags=qc.FROM_END))
            qc.assert_report(host(d_rep), qc.case_expect(cycles=C, classes=True, class_sel=2, flags=qc.FROM_END), C, f"device form, {lead} into a word")
        # refused by the address, nothing read or written
        before = host(d_rep)
        for kw, say in ((dict(d_quals=d_q.data_ptr() + 1), "d_quals"), (dict(d_quals=d_q.data_ptr() + 2), "d_quals")):
            with pytest.raises(pkg.SdtError) as e:
                g.qc_reads_device(d_w, d_o, n, d_rep, params=dict(cycles=C), **kw)
            assert e.value.code == pkg.SDT_EINVAL and say in str(e.value) and "4-byte aligned" in str(e.value)
        with pytest.raises(pkg.SdtError) as e:
            g.qc_reads_device(d_w, d_o, n, d_rep.data_ptr() + 4, d_q, params=dict(cycles=C))
        assert e.value.code == pkg.SDT_EINVAL and "d_report" in str(e.value) and "8-byte aligned" in str(e.value)
        assert (host(d_rep) == before).all()


# ---- 4. a host batch in pieces, 5. many reads per wavefront -------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import test_read_qc as me
np.save({path!r}, me.RUNS[{run!r}](pkg, synth))
"""


def run_pieces(pkg, synth):
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        return np.concatenate([run_case(g, synth, cycles=150, flags=flags, classes=True, class_sel=1) for flags in (0, qc.FROM_END)])


def strides_case():
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 41, 20000)
    reads = [rng.integers(0, 4, L).astype(np.uint8) for L in lens]
    quals = [rng.integers(33, 75, L).astype(np.uint8) for L in lens]
    return concat(reads) + (qu.concat_bytes(quals)[0], lens)


def run_strides(pkg, synth):
    codes, offs, quals, _ = strides_case()
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        return np.concatenate([g.qc_reads(qc.pack(synth, codes), offs, quals, params=dict(cycles=C, flags=flags))
                               for C, flags in ((30, 0), (30, qc.FROM_END), (150, 0))])


RUNS = dict(pieces=run_pieces, strides=run_strides)


def run_child(tmp_path, run, **env):
    path = str(tmp_path / f"{run}.npy")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path, run=run)],
                       env=dict(os.environ, SDT_TEST_HOOKS="1", **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


def test_qc_in_pieces(pkg, synth, tmp_path):
    """SDT_SEARCH_CHUNK = 7: the host form stages pieces of 7 reads, the words of each from a multiple of 16 bases, its bytes from a
    multiple of 4, so the kernel runs under many deltas between the two; the reads of 1 000 and 5 000 bases are among them"""
    starts = qc.case()["offs"][:-1:7].astype(np.int64)
    assert ((starts % 16 != 0) & (starts % 4 != 0)).sum() >= 10 and len(set((starts % 16 // 4).tolist())) == 4
    assert "SDT_SEARCH_CHUNK" not in os.environ
    hooked = run_child(tmp_path, "pieces", SDT_SEARCH_CHUNK="7")
    want = np.concatenate([qc.case_expect(cycles=150, flags=flags, classes=True, class_sel=1) for flags in (0, qc.FROM_END)])
    assert (hooked == want).all(), "pieces of 7 reads against the restatement"
    assert (hooked == run_pieces(pkg, synth)).all(), "pieces against the unhooked run"


@pytest.mark.parametrize("blocks", WAVE_BLOCKS)
def test_qc_strides(pkg, synth, tmp_path, blocks):
    """20 000 reads of 0 .. 40 bases in SDT_WAVE_BLOCKS workgroups: a wavefront takes hundreds of reads in turn, shorter ones after
    longer ones and normal ones after empty ones, and every workgroup flushes into the same report"""
    codes, offs, quals, lens = strides_case()
    reached = {}
    assert_strides("qc", lens, lens == 0, 1, WAVES, reached)
    assert min(reached.values()) >= 8, reached
    assert "SDT_WAVE_BLOCKS" not in os.environ
    want = np.concatenate([qc.expect(codes, offs, quals, cycles=C, flags=flags) for C, flags in ((30, 0), (30, qc.FROM_END), (150, 0))])
    hooked = run_child(tmp_path, "strides", SDT_WAVE_BLOCKS=str(blocks))
    assert (hooked == want).all(), f"{blocks} workgroups against the restatement"
    assert (run_strides(pkg, synth) == want).all(), "no hooks against the restatement"


# ---- 6. long reads ----------------------------------------------------------------------------------------------------------------
def test_qc_of_long_reads(pkg, synth):
    """a read of 20 000 and one of 3 000 000 bases under 64 cycles: row C holds nearly everything, more than any 32-bit counter of a
    tile could be trusted with from one read, and the first and the last 64 rows are exact"""
    rng = np.random.default_rng(9)
    lens = (20000, 3000000)
    codes, offs = concat([rng.integers(0, 4, L).astype(np.uint8) for L in lens])
    quals = rng.integers(33, 75, int(offs[-1])).astype(np.uint8)
    words = qc.pack(synth, codes)
    C = 64
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for flags in (0, qc.FROM_END):
            for q in (quals, None):
                got = g.qc_reads(words, offs, q, params=dict(cycles=C, flags=flags))
                want = qc.expect(codes, offs, q, cycles=C, flags=flags)
                s = qc.sections(want, C)
                assert int(s["base"][C].sum()) == sum(lens) - 2 * C and (s["base"][:C].sum(axis=1) == 2).all()
                qc.assert_report(got, want, C, f"long reads, flags = {flags}, quals {q is not None}")


# ---- 7. what is refused ---------------------------------------------------------------------------------------------------------------
def test_qc_refusals(pkg, synth):
    import torch
    c = qc.case()
    words, offs, quals, ranges, classes = case_words(synth), c["offs"], c["quals"], c["ranges"], c["classes"]
    n = len(offs) - 1
    good = dict(cycles=150)
    nrep = qc.report_words(150)
    report = np.full(nrep + 16, 0xABABABABABABABAB, dtype=np.uint64)       # the tail is the canary

    def call(prm, nwords=words.size, nbytes=quals.size, o=offs, rg=ranges, rw=nrep, q=quals, nreads=n):
        code = g.lib.sdt_gpu_qc_reads(g._ctx, words.ctypes.data, nwords, q.ctypes.data if q is not None else None, nbytes, o.ctypes.data, nreads,
                                      rg.ctypes.data if rg is not None else None, classes.ctypes.data, ctypes.addressof(prm) if prm is not None else None,
                                      report.ctypes.data, rw)
        return code, g.lib.sdt_gpu_last_error().decode()

    def refused(p, *say, **kw):
        code, msg = call(pkg.QcParams(**p) if p is not None else None, **kw)
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (report == 0xABABABABABABABAB).all()

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(None, "sdt_qc_params is NULL")
        refused(dict(good, cycles=0), "cycles", "= 0")
        refused(dict(good, cycles=4097), "cycles", "= 4097")
        for v in (1, 32, 34, 63, 65, 0xFFFFFFFF):
            refused(dict(good, phred_offset=v), "phred_offset", f"= {v}")
            refused(dict(good, phred_offset=v), "phred_offset", f"= {v}", q=None, nbytes=0)       # also without qualities
        refused(dict(good, flags=2), "flags", "0x2")
        refused(dict(good, flags=0x80000001), "flags", "0x80000001")
        refused(dict(good, class_sel=256), "class_sel", "= 256")
        refused(dict(good, reserved=1), "reserved", "= 1")
        bad = offs.copy()
        bad[5] = bad[6] + np.uint64(1)
        refused(good, "offsets not monotonic", "read 5", o=bad, rg=None)
        refused(good, "packed_words too short", nwords=(int(offs[-1]) + 15) // 16 + 3)
        refused(good, "quals too short", f"{int(offs[-1])} bytes", nbytes=int(offs[-1]) - 1)
        long = ranges.copy()
        r = int(np.nonzero(c["lens"] == 64)[0][0])
        long["start"][r], long["len"][r] = 60, 5
        refused(good, f"ranges[{r}]", "start = 60", "len = 5", "64 bases", rg=long)
        refused(good, "report_words", f"= {nrep - 1}", f"{nrep} words", rw=nrep - 1)
        # the boundary values pass, and a call without reads whatever the rest says
        for p in (dict(cycles=1), dict(cycles=4096, class_sel=255), dict(cycles=7, phred_offset=0, flags=1), dict(cycles=7, phred_offset=64)):
            rep = np.zeros(qc.report_words(p["cycles"]), dtype=np.uint64)
            got = g.qc_reads(words, offs, quals, ranges, classes, params=p, report=rep)
            qc.assert_report(got, qc.case_expect(classes=True, **p), p["cycles"], f"{p}")
        code, _ = call(pkg.QcParams(cycles=0, phred_offset=7, flags=6, class_sel=999, reserved=1), nreads=0, rw=0)
        assert code == pkg.SDT_OK and (report == 0xABABABABABABABAB).all()
        assert g.lib.sdt_gpu_qc_reads_device(g._ctx, None, None, None, 0, None, None, None, None) == pkg.SDT_OK
        # the device form cannot refuse a range: it clamps it, counts it, and counts nothing outside the read.  The two reads with
        # overlong ranges come last, and behind them the buffers go on with bases of code 3 and bytes of quality 60
        rng = np.random.default_rng(4)
        reads = [rng.integers(0, 3, L).astype(np.uint8) for L in (40, 0, 33, 21, 70)]             # (no code 3 in the reads)
        codes, o = concat(reads)
        q = rng.integers(33, 60, int(o[-1])).astype(np.uint8)
        rg = np.zeros(5, dtype=qc.RANGE_DTYPE)
        rg["start"], rg["len"] = (3, 0, 0, 30, 10), (30, 0, 33, 5, 0xFFFFFFFF)
        d_w = dev(qc.pack(synth, np.concatenate([codes, np.full(200, 3, dtype=np.uint8)])))
        d_q = dev(np.concatenate([q, np.full(200, 33 + 60, dtype=np.uint8)]))
        for flags in (0, qc.FROM_END):
            for starts in ((3, 0, 0, 30, 10), (3, 0, 0, 30, 0xFFFFFFFF)):
                rg["start"] = starts
                d_rep = torch.zeros(qc.report_words(16) + 8, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                g.qc_reads_device(d_w, dev(o), 5, d_rep, d_q, dev(rg.view(np.uint32)), None, dict(cycles=16, flags=flags))
                got = host(d_rep)
                want = qc.expect(codes, o, q, rg, cycles=16, flags=flags, clamp=True)
                assert want[4] == 2 and int(qc.sections(want, 16)["base"][:, 3].sum()) == 0
                qc.assert_report(got[:-8], want, 16, f"clamped ranges, flags = {flags}")
                assert (got[-8:] == 0).all()


# ---- 8. chained on the device -----------------------------------------------------------------------------------------------------------
def test_qc_takes_the_records_of_the_quality_stage(pkg, synth):
    """quality_reads_device -> qc_reads_device(ranges = its records) counts what qc_reads_device counts on the stream that the two
    compactions make from the same records; the reads the records drop are the empty reads of the first and absent from the second"""
    import torch
    rng = np.random.default_rng(12)
    reads = [rng.integers(0, 4, 150).astype(np.uint8) for _ in range(240)]
    codes, offs = concat(reads)
    quals, _ = qu.concat_bytes([(qu.realistic(rng, 150, i) + 33).astype(np.uint8) for i in range(240)])
    n, C = 240, 150
    p = qu.params(min_len=80, max_ee_ppm=20000)
    wout, wkeep, wkept = qu.expect_quality(quals, offs, p)
    dropped = n - wkept
    assert dropped >= 10 and (wout["start"] > 0).sum() >= 20 and (wout["len"] < 150).sum() >= 60
    words = qc.pack(synth, codes)
    d_w, d_o, d_q = dev(words), dev(offs), dev(quals)
    d_out = torch.full((n, 6), -3, dtype=torch.int32, device="cuda:0")
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device="cuda:0")
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device="cuda:0")
    d_oq = torch.full((len(quals) + 8,), 7, dtype=torch.uint8, device="cuda:0")
    reps = [torch.zeros(qc.report_words(C), dtype=torch.int64, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        assert g.quality_reads_device(d_q, d_o, n, d_out, None, p) == wkept
        nr, nw = g.compact_trimmed_device(d_w, d_o, n, d_out, d_ow, len(words), d_oo)
        nb = g.compact_quals_trimmed_device(d_q, d_o, n, d_out, d_oq, len(quals) + 8)
        assert nr == wkept and nb == int(wout["len"].sum())
        for i, flags in enumerate((0, qc.FROM_END)):
            g.qc_reads_device(d_w, d_o, n, reps[2 * i], d_q, d_out, None, dict(cycles=C, flags=flags))
            g.qc_reads_device(d_ow, d_oo, nr, reps[2 * i + 1], d_oq, None, None, dict(cycles=C, flags=flags))
    for i, flags in enumerate((0, qc.FROM_END)):
        by_ranges, compacted = host(reps[2 * i]), host(reps[2 * i + 1])
        qc.assert_report(by_ranges, qc.expect(codes, offs, quals, wout, cycles=C, flags=flags), C, "by the records")
        s = qc.sections(by_ranges, C)
        assert s["totals"][1] == dropped and s["len"][0] == dropped
        s["totals"][0] -= np.uint64(dropped)
        s["totals"][1] -= np.uint64(dropped)
        s["len"][0] -= np.uint64(dropped)
        qc.assert_report(compacted, by_ranges, C, "the compacted stream against the records")
