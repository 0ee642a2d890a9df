"""GPU (-m gpu): sdt_gpu_overlap_pairs and its siblings against the Python restatement of the rule (read_overlap_util.py).
Expectations never come from the library under test: the overlap of a pair is found by walking every shift and comparing base by base,
the counts of the compacted stream are the oracle's, and every output is compared for exact equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_overlap_util as ru
from test_kmer_search import keys_to_int, node_dict_oracle, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31


def assert_overlap(pkg, got, want, what):
    ov, keep, kept = got
    wov, wkeep, wkept = want
    assert ov.dtype == pkg.READ_OVERLAP_DTYPE
    ru.assert_overlap_equal(ov, wov, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
def test_overlap_equals_the_rule(pkg, synth):
    """the case under its own parameters; under min_overlap 1 with 100 % (every shift is admissible, none is left early: the score
    alone decides); and under 0 % (one mismatch ends a shift)"""
    c = ru.case()
    assert ru.case_holds() >= 25                          # the case contains what its names promise
    words = synth.pack_2bit(c["codes"])
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for mo, pct in ((None, None), (1, 100), (30, 0)):
            want = ru.case_expect(mo, pct)
            p = dict(c["params"]) if mo is None else dict(c["params"], min_overlap=mo, max_err_pct=pct)
            assert_overlap(pkg, g.overlap_pairs(words, c["offs"], p), want, f"min_overlap {p['min_overlap']}, {p['max_err_pct']} %")
            if mo == 1:                                   # every pair with two mates of a base or more has an overlap now
                assert all((want[0]["insert"][2 * i] > 0) == (len(a) > 0 and len(b) > 0) for i, (a, b) in enumerate(c["pairs"]))
            if pct == 0:
                at = c["names"].index("mismatches on budget")
                assert want[0]["insert"][2 * at] == 0 and want[0]["insert"][2 * c["names"].index("fragment 100 in 150")] == 100
        ov, keep, kept = g.overlap_pairs(words, c["offs"][:1], c["params"])
        assert len(ov) == 0 and len(keep) == 0 and kept == 0


# ---- 2. what is refused ---------------------------------------------------------------------------------------------------------------
def test_overlap_refusals(pkg, synth):
    c = ru.case()
    words = synth.pack_2bit(c["codes"])
    offs = c["offs"]
    n = len(offs) - 1
    good = c["params"]
    untouched = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_OVERLAP_DTYPE)
    keep = np.full(n, 0xAB, dtype=np.uint8)

    def refused(p, nreads, *say):
        prm = pkg.OverlapParams(**p) if p is not None else None
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_overlap_pairs(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, nreads, ctypes.addressof(prm) if prm else None,
                                           untouched.ctypes.data, keep.ctypes.data, ctypes.byref(kept))
        msg = g.lib.sdt_gpu_last_error().decode()
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and (keep == 0xAB).all() and kept.value == 0

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(dict(good, flags=1), n, "flags", "0x1")
        refused(dict(good, min_overlap=0), n, "min_overlap", "0")
        refused(dict(good, max_err_pct=101), n, "max_err_pct", "101")
        refused(None, n, "params", "NULL")
        refused(good, n - 1, "nreads", str(n - 1), "odd")
        # the device form refuses the same before it touches a buffer (the pointers are never followed)
        prm = pkg.OverlapParams(**good)
        for p, nreads, say in ((pkg.OverlapParams(**dict(good, max_err_pct=200)), n, "200"), (prm, 3, "nreads = 3")):
            kept = ctypes.c_uint64(99)
            assert g.lib.sdt_gpu_overlap_pairs_device(g._ctx, 64, 64, nreads, ctypes.addressof(p), 64, None, ctypes.byref(kept)) == pkg.SDT_EINVAL
            assert say in g.lib.sdt_gpu_last_error().decode() and kept.value == 0
        # the boundaries pass
        assert_overlap(pkg, g.overlap_pairs(words, offs, dict(good, max_err_pct=100, min_overlap=1)), ru.case_expect(1, 100), "100 %")
        # no reads: SDT_OK whatever the rest says
        ov, kp, kept = g.overlap_pairs(words, offs[:1], dict(good, flags=7, min_overlap=0, max_err_pct=1000))
        assert len(ov) == 0 and kept == 0
        kept = ctypes.c_uint64(99)
        assert g.lib.sdt_gpu_overlap_pairs(g._ctx, None, 0, None, 0, None, None, None, ctypes.byref(kept)) == pkg.SDT_OK and kept.value == 0
    # the kept form: the parameters and the pair ranges are refused before the state is looked at
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        out = np.full(8, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_OVERLAP_DTYPE)
        for p, ranges, say in ((dict(good, flags=2), [], "flags"), (dict(good, min_overlap=0), [], "min_overlap"), (dict(good, max_err_pct=101), [], "101"),
                               (good, [(0, 3)], "range 0"), (good, [(0, 4), (2, 6)], "range 1"), (good, [(4, 2)], "range 0")):
            with pytest.raises(pkg.SdtError) as e:
                g.overlap_kept_pairs(8, ranges, p, out=out)
            assert e.value.code == pkg.SDT_EINVAL and say in str(e.value), str(e.value)
        assert (out.view(np.uint32) == 0xABABABAB).all()


# ---- 3. where the reads start ---------------------------------------------------------------------------------------------------------
def test_overlap_is_alignment_independent(pkg, synth):
    """the same pairs behind one filler pair of (f, 15 - f) bases, f = 0 .. 15, and with offsets[0] = 7: every read starts at another
    base of its word.  A pair is judged on its own, so its records are the ones it had"""
    c = ru.case()
    base = ru.case_expect()
    p = c["params"]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            fa = np.full(f, ru.G, dtype=np.uint8)
            fb = np.full(15 - f, ru.C, dtype=np.uint8)
            codes, offs = ru.concat([fa, fb] + c["reads"])
            first = ru.expect_overlap(*ru.concat([fa, fb]), p)
            want = tuple(np.concatenate([a, b]) for a, b in zip(first[:2], base[:2])) + (first[2] + base[2],)
            assert_overlap(pkg, g.overlap_pairs(synth.pack_2bit(codes), offs, p), want, f"a filler pair of ({f}, {15 - f}) bases")
        shifted = np.concatenate([np.full(7, ru.T, dtype=np.uint8), c["codes"]])
        assert_overlap(pkg, g.overlap_pairs(synth.pack_2bit(shifted), c["offs"] + np.uint64(7), p), base, "offsets[0] = 7")


# ---- 4. 600 pairs over two letters: host form, device form, a host batch in pieces ----------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_overlap_util as ru
_, codes, offs = ru.at_pairs()
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    ov, keep, kept = g.overlap_pairs(synth.pack_2bit(codes), offs, ru.AT_PARAMS)
np.savez({path!r}, ov=ov, keep=keep, kept=np.uint64(kept))
"""


def test_overlap_at_pairs_host_and_device_forms(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    _, codes, offs = ru.at_pairs()
    want = ru.at_expect()
    n = len(offs) - 1
    words = synth.pack_2bit(codes)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        host = g.overlap_pairs(words, offs, ru.AT_PARAMS)
        assert_overlap(pkg, host, want, "600 A/T pairs, host form")
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_ov = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
        d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kept = g.overlap_pairs_device(d_w, d_o, n, d_ov, d_keep, ru.AT_PARAMS)
        got = d_ov.cpu().numpy().view(np.uint8).copy().view(pkg.READ_OVERLAP_DTYPE).reshape(-1)
        assert_overlap(pkg, (got, d_keep.cpu().numpy(), kept), want, "600 A/T pairs, device form")
        assert g.overlap_pairs_device(d_w, d_o, n, d_ov, None, ru.AT_PARAMS) == want[2]           # d_keep may be NULL
        assert g.overlap_pairs_device(d_w, d_o, 0, None) == 0


@pytest.mark.parametrize("chunk", [2, 7, 5000])
def test_overlap_in_pieces(pkg, synth, tmp_path, chunk):
    """SDT_SEARCH_CHUNK = 2: every pair is a piece of its own; 7: pieces of 6 reads, three whole pairs (a pair is never split); 5000: one
    piece.  Every piece is rebased to its first word"""
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SEARCH_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    assert_overlap(pkg, (hooked["ov"], hooked["keep"], int(hooked["kept"])), ru.at_expect(), f"pieces of {chunk} reads")


# ---- 5. kept reads --------------------------------------------------------------------------------------------------------------------
def test_overlap_kept_pairs(pkg, synth):
    """the layout of the host program: the read-1 file as one kept batch (ordinals base, base + 2, ...), the read-2 file as another
    (base + 1, base + 3, ...), so the mates of every pair sit in different batches; a batch of single reads behind them, outside the
    pair range; no read has ordinals 0 .. 2, and the read-2 file is one read short: the last pair has one mate only"""
    c = ru.case()
    at = {n: i for i, n in enumerate(c["names"])}
    pool = [pr for pr, n in zip(c["pairs"], c["names"]) if n != "2500 bases" and "0 bases" not in n]
    P, base = 14, 3
    r1 = [pool[t][0] for t in range(P)] + [c["pairs"][at["fragment 100 in 150"]][0]]
    r2 = [pool[t][1] for t in range(P)]
    singles = list(c["pairs"][at["fragment 100 in 150"]]) + list(c["pairs"][at["mate shorter than min_overlap"]])      # mates side by side, outside the range
    first, end = base, base + 2 * (P + 1)
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)] + [end + i for i in range(len(singles))]
    codes, offs = ru.concat(r1 + r2 + singles)
    total = end + len(singles)
    absent = np.ones(total, dtype=bool)
    absent[ords] = False
    assert absent.sum() == 4
    p = c["params"]
    wov, wkeep, wkept = ru.expect_overlap(codes, offs, p, pair_ranges=[(first, end)], ordinals=ords)
    assert (wov["insert"][first:end] > 0).sum() >= 6 and {ru.WHOLE, ru.CLIPPED, ru.DROPPED} == set(wov["verdict"][~absent].tolist())
    assert wov[end - 2].tolist() == (0, 0, 0, 0, 150, ru.WHOLE)                  # a read-through mate whose mate is not kept: nothing is known
    assert wov[end].tolist() == wov[end + 1].tolist() == (0, 0, 0, 0, 150, ru.WHOLE) and wov[end + 3].tolist() == (0, 0, 0, 0, 0, ru.DROPPED)
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for batch, b, stride in ((r1, base, 2), (r2, base + 1, 2), (singles, end, 1)):
            g.set_read_ordinal(b, stride)
            bc, bo = ru.concat(batch)
            g.push_reads(synth.pack_2bit(bc), bo)
        g.finish_count()
        out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_OVERLAP_DTYPE)
        ov, n, kept = g.overlap_kept_pairs(total, [(first, end)], p, out=out)
        assert n == len(ords) and kept == wkept
        assert (np.ascontiguousarray(ov[absent]).view(np.uint32) == 0xABABABAB).all()
        ru.assert_overlap_equal(ov[~absent], wov[~absent], "kept reads")
        # the same range in two halves that touch; a range that reaches past the last ordinal
        ov2, n, kept = g.overlap_kept_pairs(total, [(first, first + 8), (first + 8, end)], p)
        ru.assert_overlap_equal(ov2[~absent], wov[~absent], "kept reads, two ranges")
        # no ranges: every read is single, nothing is cut
        wnone = ru.expect_overlap(codes, offs, p, pair_ranges=[], ordinals=ords)
        ov3, n, kept = g.overlap_kept_pairs(total, (), p)
        ru.assert_overlap_equal(ov3[~absent], wnone[0][~absent], "kept reads, no pair ranges")
        assert kept == wnone[2] and (wnone[0]["insert"] == 0).all()
        # the singles as a second range: now they are pairs
        wtwo = ru.expect_overlap(codes, offs, p, pair_ranges=[(first, end), (end, total)], ordinals=ords)
        ov4, n, kept = g.overlap_kept_pairs(total, [(first, end), (end, total)], p)
        ru.assert_overlap_equal(ov4[~absent], wtwo[0][~absent], "kept reads, the singles as pairs")
        assert wtwo[0][end].tolist() == (100, 0, 100, 0, 100, ru.CLIPPED)
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_OVERLAP_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.overlap_kept_pairs(total - 1, [(first, end)], p, out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        # the kept reads are as they were
        bc, bo = ru.concat(r2)
        w, o, b, stride = g.fetch_kept_batch(1)
        assert (b, stride) == (base + 1, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        with pytest.raises(pkg.SdtError) as e:
            g.overlap_kept_pairs(total, [(first, end)], p)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)


# ---- 6. overlap, compact, count: nothing crosses to the host ----------------------------------------------------------------------------
def test_overlap_device_form_and_compaction(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    L = 100
    _, codes, offs = workload(synth, K, L, n_reads=400)
    rng = np.random.default_rng(12)
    frags = [codes[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    frags = [r for r in frags if len(r) >= 70][:120]      # (the workload's reads are ragged)
    assert len(frags) == 120
    rnd = lambda m: rng.integers(0, 4, size=m, dtype=np.uint8)
    reads = []
    for i, fr in enumerate(frags):                        # a third read through into adapter, some down to a fragment shorter than a k-mer
        n = len(fr)
        F = (n, n, int(rng.integers(40, n - 5)))[i % 3] if i % 12 != 5 else 31
        a = np.concatenate([fr[:F], rnd(n - F)]).astype(np.uint8)
        b = np.concatenate([ru.revcomp(fr[:F]), rnd(n - F)]).astype(np.uint8)
        reads += [a, b] if i % 3 != 1 else [a, rnd(n)]    # (a third of the pairs: unrelated mates)
    codes, offs = ru.concat(reads)
    n = len(offs) - 1
    p = ru.params(min_len=K + 1)
    wov, wkeep, wkept = ru.expect_overlap(codes, offs, p)
    assert {ru.WHOLE, ru.CLIPPED, ru.DROPPED} == set(wov["verdict"].tolist()) and (wov["verdict"] == ru.CLIPPED).sum() >= 60
    assert (wov["insert"] == 0).sum() >= 60 and (wov["verdict"] == ru.DROPPED).sum() >= 10
    kcodes, koffs = ru.concat(ru.cut_reads(codes, offs, wov))
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_ov = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    # the overlap runs on a context that never counts (a contig index) and before any count: it needs no table
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        assert a.overlap_pairs_device(d_w, d_o, n, d_ov, d_keep, p) == wkept
        assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
        nr, nw = a.compact_trimmed_device(d_w, d_o, n, d_ov, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, int(np.diff(koffs.astype(np.int64)).max()))
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
        # the host form on the same kind of context, and its records through the host compaction
        host = a.overlap_pairs(words, offs, p)
        assert_overlap(pkg, host, (wov, wkeep, wkept), "a contig index, host form")
        hw, ho = a.compact_trimmed(words, offs, host[0].view(pkg.READ_TRIM_DTYPE))
        assert ho.tolist() == koffs.tolist() and hw[:len(hw) - 4].tolist() == synth.pack_2bit(kcodes)[:len(hw) - 4].tolist()
    got_ov = d_ov.cpu().numpy().view(np.uint8).copy().view(pkg.READ_OVERLAP_DTYPE).reshape(-1)
    ru.assert_overlap_equal(got_ov, wov, "device form")
    assert d_oo.cpu().numpy()[: nr + 1].tolist() == koffs.tolist()
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want
