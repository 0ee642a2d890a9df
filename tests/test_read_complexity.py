"""GPU (-m gpu): sdt_gpu_complexity_reads and its siblings against the numpy restatement of the rule (read_complexity_util.py).
Expectations never come from the library under test: the triplets of every window are counted per kind on the CPU, the counts of the
compacted stream are the oracle's, and every output is compared for exact equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_complexity_util as cu
from test_kmer_search import keys_to_int, node_dict_oracle, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31
TRIM = dict(max_low_pct=0, flags=cu.TRIM)


def assert_cx(pkg, got, want, what):
    cx, keep, kept = got
    wcx, wkeep, wkept = want
    assert cx.dtype == pkg.READ_COMPLEXITY_DTYPE
    cu.assert_cx_equal(cx, wcx, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
def test_complexity_equals_the_rule(pkg, synth):
    """the case under its own parameters; under SDT_COMPLEXITY_TRIM; under max_score_pct 100 (only windows whose triplets are all equal
    are low) and under 1 (every window with a repeated triplet is)"""
    c = cu.case()
    assert cu.case_holds() >= 25                          # the case contains what its names promise
    words = synth.pack_2bit(c["codes"])
    p = c["params"]
    runs = [(p, cu.case_expect()), (dict(p, **TRIM), cu.case_expect(trim=True)), (dict(p, max_score_pct=100), cu.case_expect(max_score_pct=100)),
            (dict(p, max_score_pct=1), cu.case_expect(max_score_pct=1)), (dict(p, max_score_pct=1, min_len=0, **TRIM), None)]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for i, (q, want) in enumerate(runs):
            want = want or cu.expect_complexity(c["codes"], c["offs"], q)
            assert_cx(pkg, g.complexity_reads(words, c["offs"], q), want, f"run {i}")
        cx, keep, kept = g.complexity_reads(words, c["offs"][:1], p)
        assert len(cx) == 0 and len(keep) == 0 and kept == 0


# ---- 2. what is refused ---------------------------------------------------------------------------------------------------------------
def test_complexity_refusals(pkg, synth):
    c = cu.case()
    words = synth.pack_2bit(c["codes"])
    offs = c["offs"]
    n = len(offs) - 1
    good = c["params"]
    untouched = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_COMPLEXITY_DTYPE)

    def refused(p, *say):
        prm = pkg.ComplexityParams(**p)
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_complexity_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, ctypes.addressof(prm), untouched.ctypes.data,
                                              None, ctypes.byref(kept))
        msg = g.lib.sdt_gpu_last_error().decode()
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and kept.value == 0

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(dict(good, flags=2), "flags", "0x2")
        refused(dict(good, flags=0x80000001), "flags", "0x80000001")
        refused(dict(good, max_score_pct=0), "max_score_pct", "= 0")
        refused(dict(good, max_score_pct=101), "max_score_pct", "101")
        refused(dict(good, max_low_pct=101), "max_low_pct", "101")
        refused(dict(good, max_low_pct=5, flags=cu.TRIM), "max_low_pct", "= 5", "SDT_COMPLEXITY_TRIM")
        # NULL params
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_complexity_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, None, untouched.ctypes.data, None,
                                              ctypes.byref(kept))
        assert code == pkg.SDT_EINVAL and "params" in g.lib.sdt_gpu_last_error().decode()
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and kept.value == 0
        # the boundaries pass, and so does a NULL keep
        for q in (dict(good, max_score_pct=100, max_low_pct=100), dict(good, max_score_pct=1, **TRIM), dict(good, max_low_pct=0)):
            prm = pkg.ComplexityParams(**q)
            out = np.zeros(n, dtype=pkg.READ_COMPLEXITY_DTYPE)
            kept = ctypes.c_uint64()
            assert g.lib.sdt_gpu_complexity_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, ctypes.addressof(prm), out.ctypes.data,
                                                  None, ctypes.byref(kept)) == pkg.SDT_OK
            want = cu.expect_complexity(c["codes"], offs, q)
            cu.assert_cx_equal(out, want[0], f"{q}")
            assert kept.value == want[2]
        # no reads: SDT_OK whatever the rest says
        cx, keep, kept = g.complexity_reads(words, offs[:1], dict(good, flags=6, max_score_pct=0))
        assert len(cx) == 0 and kept == 0


# ---- 3. where the reads start ---------------------------------------------------------------------------------------------------------
def test_complexity_is_alignment_independent(pkg, synth):
    """the same reads behind one filler read of 0 .. 15 bases, and with offsets[0] = 7: every read starts at another base of its word.
    A read is judged on its own, so its record is the one it had"""
    c = cu.case()
    p = dict(c["params"], **TRIM)
    base = cu.case_expect(trim=True)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            filler = np.full(f, cu.G, dtype=np.uint8)
            filler[::2] = cu.C                                                # CGCG...
            codes, offs = cu.concat([filler] + c["reads"])
            first = cu.expect_complexity(filler, np.array([0, f], dtype=np.uint64), p)
            want = tuple(np.concatenate([a, b]) for a, b in zip(first[:2], base[:2])) + (first[2] + base[2],)
            assert_cx(pkg, g.complexity_reads(synth.pack_2bit(codes), offs, p), want, f"{f} filler bases")
        shifted = np.concatenate([np.full(7, cu.T, dtype=np.uint8), c["codes"]])
        assert_cx(pkg, g.complexity_reads(synth.pack_2bit(shifted), c["offs"] + np.uint64(7), p), base, "offsets[0] = 7")
        assert_cx(pkg, g.complexity_reads(synth.pack_2bit(shifted), c["offs"] + np.uint64(7), c["params"]), cu.case_expect(), "offsets[0] = 7, filter")


# ---- 4. a host batch in pieces --------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_complexity_util as cu
c = cu.case()
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    cx, keep, kept = g.complexity_reads(synth.pack_2bit(c["codes"]), c["offs"], dict(c["params"], max_low_pct=0, flags=cu.TRIM))
np.savez({path!r}, cx=cx, keep=keep, kept=np.uint64(kept))
"""


def test_complexity_in_pieces(pkg, synth, tmp_path):
    """SDT_SEARCH_CHUNK = 7: the host form stages 22 pieces of 7 reads (the last of fewer), each rebased to its first word"""
    c = cu.case()
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SEARCH_CHUNK="7")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    got = (hooked["cx"], hooked["keep"], int(hooked["kept"]))
    assert_cx(pkg, got, cu.case_expect(trim=True), "pieces of 7 reads")
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert_cx(pkg, got, g.complexity_reads(synth.pack_2bit(c["codes"]), c["offs"], dict(c["params"], **TRIM)), "pieces against the unhooked run")


# ---- 5. complexity, compact, count: nothing crosses to the host -----------------------------------------------------------------------
def test_complexity_device_form_and_compaction(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    _, codes, offs = workload(synth, K, 150, n_reads=300)
    rng = np.random.default_rng(12)
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    reads = [r.copy() for r in reads if len(r) >= K + 1][:240]
    assert len(reads) == 240
    for i in range(0, 240, 3):                            # a third of the reads carry a run of 28 .. 70 bases: poly-A, poly-G or (AC)n
        n = min(int(rng.integers(28, 71)), len(reads[i]))
        at = int(rng.integers(0, len(reads[i]) - n + 1))
        reads[i][at:at + n] = (np.full(n, cu.A), np.full(n, cu.G), np.resize([cu.A, cu.C], n))[i // 3 % 3]
    codes, offs = cu.concat(reads)
    n = len(offs) - 1
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    for mode, p in (("filter", cu.params(min_len=K + 1)), ("trim", cu.params(min_len=K + 1, **TRIM))):
        wcx, wkeep, wkept = cu.expect_complexity(codes, offs, p)
        assert {cu.WHOLE, cu.DROPPED} <= set(wcx["verdict"].tolist()) and (wcx["low"] > 0).sum() >= 60 and (wcx["verdict"] == cu.DROPPED).sum() >= 10
        assert mode == "filter" or ((wcx["verdict"] == cu.CLIPPED).sum() >= 20 and (wcx["start"] > 0).sum() >= 5)
        kcodes, koffs = cu.concat(cu.cut_reads(codes, offs, wcx))
        o2 = ob.Oracle(K, nsets=5)
        o2.add_reads(kcodes, koffs)
        want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
        d_cx = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
        d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
        d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # the filter runs on a context that never counts (a contig index) and before any count: it needs no table
        with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
            assert a.complexity_reads_device(d_w, d_o, n, d_cx, d_keep, p) == wkept
            assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
            assert a.complexity_reads_device(d_w, d_o, n, d_cx, None, p) == wkept                   # d_keep may be NULL
            assert a.complexity_reads_device(d_w, d_o, 0, None) == 0
            nr, nw = a.compact_trimmed_device(d_w, d_o, n, d_cx, d_ow, len(words), d_oo)
            assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
            b.count_reads_device(d_ow, nw + 4, d_oo, nr, int(np.diff(koffs.astype(np.int64)).max()))
            assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
            keys, l, rf, cnt = b.export_nodes()[:4]
            # the host form on the same kind of context
            assert_cx(pkg, a.complexity_reads(words, offs, p), (wcx, wkeep, wkept), f"{mode}: a contig index, host form")
        got_cx = d_cx.cpu().numpy().view(np.uint8).copy().view(pkg.READ_COMPLEXITY_DTYPE).reshape(-1)
        cu.assert_cx_equal(got_cx, wcx, f"{mode}: device form")
        assert d_oo.cpu().numpy()[: nr + 1].tolist() == koffs.tolist()
        got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
        assert len(got) == len(want) and got == want, mode


# ---- 6. kept reads ----------------------------------------------------------------------------------------------------------------
def test_complexity_kept_reads(pkg, synth):
    """the layout of the host program: the read-1 file as one kept batch (ordinals base, base + 2, ...), the read-2 file as another
    (base + 1, base + 3, ...); no read has ordinals 0 .. 2, and the read-2 file is one read short"""
    c = cu.case()
    rng = np.random.default_rng(79)
    pool = [r for r, n in zip(c["reads"], c["names"]) if 40 <= len(r) <= 250]
    P, base = 14, 3
    r1 = [pool[int(i)] for i in rng.permutation(len(pool))[:P + 1]]
    r2 = [pool[int(i)] for i in rng.permutation(len(pool))[:P]]
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)]
    codes, offs = cu.concat(r1 + r2)
    total = base + 2 * (P + 1)
    absent = np.ones(total, dtype=bool)
    absent[ords] = False
    assert absent.sum() == 4
    p = dict(c["params"], **TRIM)
    wcx, wkeep, wkept = cu.expect_complexity(codes, offs, p, ordinals=ords)
    assert len(wcx) == total - 1 and {cu.WHOLE, cu.CLIPPED} <= set(wcx["verdict"][~absent[:-1]].tolist())
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for batch, b in ((r1, base), (r2, base + 1)):
            g.set_read_ordinal(b, 2)
            bc, bo = cu.concat(batch)
            g.push_reads(synth.pack_2bit(bc), bo)
        # batches were pushed and not drained
        with pytest.raises(pkg.SdtError) as e:
            g.complexity_kept_reads(total, p)
        assert e.value.code == pkg.SDT_ESTATE and "finish_count" in str(e.value)
        g.finish_count()
        out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_COMPLEXITY_DTYPE)
        cx, n, kept = g.complexity_kept_reads(total, p, out=out)
        assert n == len(ords) and kept == wkept
        assert (np.ascontiguousarray(cx[absent]).view(np.uint32) == 0xABABABAB).all()
        cu.assert_cx_equal(cx[:-1][~absent[:-1]], wcx[~absent[:-1]], "kept reads")
        # the filter on the same kept reads; exactly the records up to the highest ordinal fit
        cx, n, kept = g.complexity_kept_reads(total - 1, c["params"])
        want = cu.expect_complexity(codes, offs, c["params"], ordinals=ords)
        cu.assert_cx_equal(cx, want[0], "kept reads, out_capacity = highest ordinal + 1")
        assert kept == want[2]
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 2, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_COMPLEXITY_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.complexity_kept_reads(total - 2, p, out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.complexity_kept_reads(total, dict(p, flags=3))
        assert e.value.code == pkg.SDT_EINVAL
        # the kept reads are as they were
        for i, (batch, b) in enumerate(((r1, base), (r2, base + 1))):
            bc, bo = cu.concat(batch)
            w, o, got_base, stride = g.fetch_kept_batch(i)
            assert (got_base, stride) == (b, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        with pytest.raises(pkg.SdtError) as e:
            g.complexity_kept_reads(total, p)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
