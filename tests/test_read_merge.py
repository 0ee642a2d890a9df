"""GPU (-m gpu): sdt_gpu_merge_pairs, sdt_gpu_compact_quals_trimmed and their siblings against the Python restatement of the rule
(read_merge_util.py).  Expectations never come from the library under test: a merged read is built base by base, the overlap records
that go in are written by hand or come from the overlap rule restated, the counts of the streams are the oracle's, and every output
is compared for exact equality."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_merge_util as mu
import read_overlap_util as ro
import read_quality_util as rq
from test_kmer_search import keys_to_int, node_dict_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31


def records(pkg, t):
    return t.cpu().numpy().view(np.uint8).copy().view(pkg.READ_MERGE_DTYPE).reshape(-1)


def assert_merge(pkg, got, want, what):
    mg, words, offs = got
    wmg, wreads = want
    assert mg.dtype == pkg.READ_MERGE_DTYPE
    mu.assert_merge_equal(mg, wmg, what)
    mu.assert_stream_equal(words, offs, wreads, what)


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
def test_merge_equals_the_rule(pkg, synth):
    """the case without qualities, with them under phred 33 and under phred 64: records, out_offsets, every output word, the zero tail
    bits and the pad words"""
    c = mu.case()
    assert mu.case_holds() >= 25                          # the case contains what its names promise
    words = synth.pack_2bit(c["codes"])
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for phred in (None, 33, 64):
            p = dict(c["params"], phred_offset=phred if phred is not None else 33)
            got = g.merge_pairs(words, c["offs"], c["ov"], c["quals"] if phred is not None else None, p)
            assert_merge(pkg, got, mu.case_expect(phred), f"phred {phred}")
        # without qualities the offset is not looked at
        assert_merge(pkg, g.merge_pairs(words, c["offs"], c["ov"], None, dict(c["params"], phred_offset=7)), mu.case_expect(None), "phred 7, no qualities")
        # the records through the compaction: the stream of the pairs that did not merge
        mg = got[0]
        rw, roffs = g.compact_trimmed(words, c["offs"], mg.view(pkg.READ_TRIM_DTYPE))
        mu.assert_stream_equal(rw, roffs, mu.rest_reads(c["codes"], c["offs"], mu.case_expect(64)[0]), "the rest")
        # no reads
        mg, w, o = g.merge_pairs(words, c["offs"][:1], c["ov"][:0], None, c["params"])
        assert len(mg) == 0 and o.tolist() == [0] and w.tolist() == [0xABABABAB] * 4       # (nothing is written for no reads)


# ---- 2. where the reads start, in the input and in the output ------------------------------------------------------------------------
def test_merge_is_alignment_independent(pkg, synth):
    """the case behind one filler pair of (f, 15 - f) bases that does not merge, f = 0 .. 15, and with offsets[0] = 7: every read starts
    at another base of its word; and behind a filler pair that MERGES into g = 1 .. 16 bases: every merged read starts at every base of
    its output word, where a direct store would race and a shift would slip"""
    c = mu.case()
    p = dict(c["params"], min_len=1)
    base_mg, base_out = mu.expect_merge(c["codes"], c["offs"], c["ov"], p, c["quals"])
    rng = np.random.default_rng(5)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            fa, fb = np.full(f, ro.G, dtype=np.uint8), np.full(15 - f, ro.C, dtype=np.uint8)
            codes, offs = ro.concat([fa, fb] + c["reads"])
            first = np.array([ro.read_record(len(fa), (0, 0, 0), 0), ro.read_record(len(fb), (0, 0, 0), 0)], dtype=ro.OVERLAP_DTYPE)
            quals = np.concatenate([np.full(15, 50, dtype=np.uint8), c["quals"]])
            want = (np.concatenate([mu.expect_merge(*ro.concat([fa, fb]), first, p)[0], base_mg]), base_out)
            got = g.merge_pairs(synth.pack_2bit(codes), offs, np.concatenate([first, c["ov"]]), quals, p)
            assert_merge(pkg, got, want, f"a filler pair of ({f}, {15 - f}) bases")
        shifted = np.concatenate([np.full(7, ro.T, dtype=np.uint8), c["codes"]])
        quals = np.concatenate([np.full(7, 99, dtype=np.uint8), c["quals"]])
        got = g.merge_pairs(synth.pack_2bit(shifted), c["offs"] + np.uint64(7), c["ov"], quals, p)
        assert_merge(pkg, got, (base_mg, base_out), "offsets[0] = 7")
        for gl in range(1, 17):
            frag = rng.integers(0, 4, size=gl, dtype=np.uint8)
            fa, fb = frag, ro.revcomp(frag)
            codes, offs = ro.concat([fa, fb] + c["reads"])
            first = np.array([ro.read_record(gl, (gl, 0, gl), 0)] * 2, dtype=ro.OVERLAP_DTYPE)
            quals = np.concatenate([np.full(2 * gl, 50, dtype=np.uint8), c["quals"]])
            want = (np.concatenate([np.array([(gl, 0, 0, 0, 0, mu.MERGED)] * 2, dtype=mu.MERGE_DTYPE), base_mg]), [frag] + base_out)
            got = g.merge_pairs(synth.pack_2bit(codes), offs, np.concatenate([first, c["ov"]]), quals, p)
            assert_merge(pkg, got, want, f"a merged filler of {gl} bases in front")


# ---- 3. 600 pairs over two letters: host form, device form, another launch geometry ---------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_overlap_util as ro
import read_merge_util as mu
_, codes, offs = ro.at_pairs()
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    mg, words, oo = g.merge_pairs(synth.pack_2bit(codes), offs, ro.at_expect()[0], mu.at_quals(), mu.AT_PARAMS)
np.savez({path!r}, mg=mg, words=words, offs=oo)
"""


def test_merge_at_pairs_host_and_device_forms(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    _, codes, offs = ro.at_pairs()
    ov = ro.at_expect()[0]
    n = len(offs) - 1
    words = synth.pack_2bit(codes)
    quals = mu.at_quals()
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_ov = torch.from_numpy(ov.view(np.int32).reshape(n, 6)).to(dev)
        d_q = torch.from_numpy(np.concatenate([quals, np.zeros(-len(quals) % 4, dtype=np.uint8)])).to(dev)
        for with_quals in (False, True):
            want = mu.at_expect(with_quals)              # (asserts that at least 100 pairs merge and 50 have from_b > 0)
            assert_merge(pkg, g.merge_pairs(words, offs, ov, quals if with_quals else None, mu.AT_PARAMS), want, f"600 A/T pairs, host form, qualities {with_quals}")
            d_mg = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
            d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
            d_oo = torch.full((n // 2 + 1,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            nm, nw = g.merge_pairs_device(d_w, d_o, n, d_ov, d_mg, d_ow, len(words), d_oo, d_q if with_quals else None, mu.AT_PARAMS)
            assert nm == len(want[1]) and nw == (sum(len(m) for m in want[1]) + 15) // 16
            got = (records(pkg, d_mg), d_ow.cpu().numpy().view(np.uint32)[: nw + 4], d_oo.cpu().numpy().view(np.uint64)[: nm + 1])
            assert_merge(pkg, got, want, f"600 A/T pairs, device form, qualities {with_quals}")
            assert (d_ow.cpu().numpy()[nw + 4:] == -1).all() and (d_oo.cpu().numpy()[nm + 1:] == -1).all()       # nothing behind the outputs


def test_merge_does_not_depend_on_the_launch_geometry(pkg, synth, tmp_path):
    """two workgroups of wavefronts and one workgroup of lanes do all the work: a wavefront takes pair after pair"""
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_WAVE_BLOCKS="2", SDT_SCAN_BLOCKS="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    assert_merge(pkg, (hooked["mg"], hooked["words"], hooked["offs"]), mu.at_expect(True), "two workgroups")


# ---- 4. what is refused ---------------------------------------------------------------------------------------------------------------
def test_merge_refusals(pkg, synth):
    c = mu.case()
    words = synth.pack_2bit(c["codes"])
    offs, ov, quals = c["offs"], c["ov"], c["quals"]
    n = len(offs) - 1
    good = c["params"]
    mg = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_MERGE_DTYPE)
    ow = np.full(len(words), 0xABABABAB, dtype=np.uint32)
    oo = np.full(n // 2 + 1, 0xABABABABABABABAB, dtype=np.uint64)

    def call(p, nreads, with_quals, records=ov, cap=None):
        prm = pkg.MergeParams(**p) if p is not None else None
        nm, nw = ctypes.c_uint64(99), ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_merge_pairs(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, nreads, records.ctypes.data,
                                         quals.ctypes.data if with_quals else None, ctypes.addressof(prm) if prm else None, mg.ctypes.data, ow.ctypes.data,
                                         len(ow) if cap is None else cap, oo.ctypes.data, ctypes.byref(nm), ctypes.byref(nw))
        return code, g.lib.sdt_gpu_last_error().decode(), nm.value, nw.value

    def untouched():
        return (mg.view(np.uint32) == 0xABABABAB).all() and (ow == 0xABABABAB).all() and (oo == 0xABABABABABABABAB).all()

    def refused(p, nreads, with_quals, *say, records=ov):
        code, msg, nm, nw = call(p, nreads, with_quals, records)
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert untouched() and nm == 0 and nw == 0

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(None, n, False, "params", "NULL")
        refused(dict(good, flags=1), n, False, "flags", "0x1")
        refused(dict(good, min_len=30, max_len=29), n, False, "max_len", "29")
        refused(dict(good, min_len=0, max_len=0, phred_offset=32), n, True, "phred_offset", "32")
        refused(good, n - 1, False, "nreads", str(n - 1), "odd")
        # records that are not one overlap of their mates: the inserts differ; an insert that no shift gives
        bad = ov.copy()
        t = c["names"].index("read-through, F < La")
        bad["insert"][2 * t + 1] += 1
        refused(good, n, False, f"pair {t}", "100", "101", records=bad)
        bad = ov.copy()
        t = c["names"].index("no overlap")
        bad["insert"][2 * t] = bad["insert"][2 * t + 1] = len(c["pairs"][t][0]) + len(c["pairs"][t][1])
        refused(good, n, False, f"pair {t}", str(int(bad["insert"][2 * t])), records=bad)
        # the boundaries pass: phred 32 without qualities, max_len == min_len
        code, msg, nm, nw = call(dict(good, phred_offset=32, min_len=100, max_len=100), n, False)
        assert code == pkg.SDT_OK and nm == sum(1 for F in c["inserts"] if F == 100)
        # out_words one word short: SDT_EFULL with both counts set, nothing written
        mg[:] = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_MERGE_DTYPE)
        ow[:] = 0xABABABAB
        oo[:] = 0xABABABABABABABAB
        want = mu.case_expect(None)
        need = (sum(len(m) for m in want[1]) + 15) // 16
        code, msg, nm, nw = call(good, n, False, cap=need + 3)
        assert code == pkg.SDT_EFULL and (nm, nw) == (len(want[1]), need) and untouched(), msg
        with pytest.raises(pkg.SdtError) as e:
            g.merge_pairs(words, offs, ov, None, good, out_words_cap=need + 3)
        assert e.value.code == pkg.SDT_EFULL and e.value.needed == need and e.value.n_merged == len(want[1])
        assert_merge(pkg, g.merge_pairs(words, offs, ov, None, good, out_words_cap=need + 4), want, "exactly the words it takes")
        # no reads: SDT_OK whatever the rest says, *n_merged = 0 and out_offsets[0] = 0
        nm, nw = ctypes.c_uint64(99), ctypes.c_uint64(99)
        assert g.lib.sdt_gpu_merge_pairs(g._ctx, None, 0, None, 0, None, None, None, None, None, 0, oo.ctypes.data, ctypes.byref(nm), ctypes.byref(nw)) == pkg.SDT_OK
        assert (nm.value, nw.value) == (0, 0) and oo[0] == 0 and oo[1] == 0xABABABABABABABAB
        assert g.lib.sdt_gpu_merge_pairs(g._ctx, None, 0, None, 0, None, None, None, None, None, 0, None, None, None) == pkg.SDT_OK


def test_merge_device_form_refusals_and_inconsistent_records(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    c = mu.case()
    words = synth.pack_2bit(c["codes"])
    offs, n, good = c["offs"], len(c["offs"]) - 1, c["params"]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        # refused before a buffer is touched (the pointers are never followed)
        for p, nreads, dq, say in ((dict(good, flags=4), n, None, "flags"), (dict(good, min_len=9, max_len=8), n, None, "max_len = 8"),
                                   (dict(good, phred_offset=1), n, 64, "phred_offset = 1"), (good, 3, None, "nreads = 3"), (good, n, 66, "4-byte aligned")):
            prm = pkg.MergeParams(**p)
            nm, nw = ctypes.c_uint64(99), ctypes.c_uint64(99)
            assert g.lib.sdt_gpu_merge_pairs_device(g._ctx, 64, 64, nreads, 64, dq, ctypes.addressof(prm), 64, 64, 1 << 20, 64, ctypes.byref(nm),
                                                    ctypes.byref(nw)) == pkg.SDT_EINVAL
            assert say in g.lib.sdt_gpu_last_error().decode() and (nm.value, nw.value) == (0, 0), g.lib.sdt_gpu_last_error().decode()
        # a pair of inconsistent records counts as not merged: its reads keep what their overlap records keep
        bad = c["ov"].copy()
        t = c["names"].index("read-through, F < La")
        u = c["names"].index("La < F < La + Lb")
        bad["insert"][2 * t + 1] += 1
        bad["insert"][2 * u] = bad["insert"][2 * u + 1] = 300                 # = La + Lb: no shift gives it
        fixed = bad.copy()
        fixed["insert"][[2 * t, 2 * t + 1, 2 * u, 2 * u + 1]] = 0
        want = mu.expect_merge(c["codes"], offs, fixed, good, c["quals"])
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_ov = torch.from_numpy(bad.view(np.int32).reshape(n, 6)).to(dev)
        d_q = torch.from_numpy(np.concatenate([c["quals"], np.zeros(-len(c["quals"]) % 4, dtype=np.uint8)])).to(dev)
        d_mg = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
        d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
        d_oo = torch.full((n // 2 + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        nm, nw = g.merge_pairs_device(d_w, d_o, n, d_ov, d_mg, d_ow, len(words), d_oo, d_q, good)
        assert nm == len(want[1]) == len(mu.case_expect(33)[1]) - 2
        assert_merge(pkg, (records(pkg, d_mg), d_ow.cpu().numpy().view(np.uint32)[: nw + 4], d_oo.cpu().numpy().view(np.uint64)[: nm + 1]), want, "device form")
        # SDT_EFULL: both counts, nothing written
        d_mg.fill_(-3)
        d_ow.fill_(-1)
        d_oo.fill_(-1)
        torch.cuda.synchronize()
        with pytest.raises(pkg.SdtError) as e:
            g.merge_pairs_device(d_w, d_o, n, d_ov, d_mg, d_ow, nw + 3, d_oo, d_q, good)
        assert e.value.code == pkg.SDT_EFULL and (e.value.n_merged, e.value.needed) == (nm, nw)
        assert (d_mg.cpu().numpy() == -3).all() and (d_ow.cpu().numpy() == -1).all() and (d_oo.cpu().numpy() == -1).all()
        # no reads
        assert g.merge_pairs_device(None, None, 0, None, None, None, 0, d_oo) == (0, 0) and d_oo.cpu().numpy()[:2].tolist() == [0, -1]


# ---- 5. kept reads --------------------------------------------------------------------------------------------------------------------
def test_merge_kept_pairs(pkg, synth):
    """the layout of the host program: the read-1 file as one kept batch (ordinals base, base + 2, ...: an odd base, stride 2), the
    read-2 file as another, so the mates of every pair sit in different batches; a batch of single reads behind them, outside the pair
    range; no read has ordinals 0 .. 2, and the read-2 file is one read short: the last pair has one mate only"""
    c = mu.case()
    pool = [i for i, nm in enumerate(c["names"]) if "0 bases" not in nm and len(c["pairs"][i][0]) < 2000]
    P, base = 16, 3
    last = c["names"].index("read-through, F < La")
    r1 = [c["pairs"][i][0] for i in pool[:P]] + [c["pairs"][last][0]]
    r2 = [c["pairs"][i][1] for i in pool[:P]]
    singles = list(c["pairs"][last])                                         # mates side by side, outside the range
    first, end = base, base + 2 * (P + 1)
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)] + [end + i for i in range(len(singles))]
    codes, offs = ro.concat(r1 + r2 + singles)
    total = end + len(singles)
    absent = np.ones(total, dtype=bool)
    absent[ords] = False
    # the overlap records by ordinal: those of the case's pairs; the mate without a mate and the singles as the overlap stage leaves them
    ov = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_OVERLAP_DTYPE).copy()
    for t, i in enumerate(pool[:P]):
        ov[base + 2 * t], ov[base + 2 * t + 1] = c["ov"][2 * i], c["ov"][2 * i + 1]
    for o, L in ((end - 2, 150), (end, 150), (end + 1, 150)):
        ov[o] = ro.read_record(L, (0, 0, 0), 0)
    p = c["params"]
    wmg, wout = mu.expect_merge(codes, offs, ov, p, pair_ranges=[(first, end)], ordinals=ords)
    assert len(wout) >= 8 and wmg["mismatches"].sum() > 0 and wmg[end - 2].tolist() == (0, 0, 0, 0, 150, ro.WHOLE) == wmg[end].tolist()
    cap = (sum(len(m) for m in wout) + 15) // 16 + 4
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for batch, b, stride in ((r1, base, 2), (r2, base + 1, 2), (singles, end, 1)):
            g.set_read_ordinal(b, stride)
            bc, bo = ro.concat(batch)
            g.push_reads(synth.pack_2bit(bc), bo)
        g.finish_count()
        out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_MERGE_DTYPE)
        mg, words, oo, n = g.merge_kept_pairs(total, ov, [(first, end)], p, out=out, out_words_cap=cap)
        assert n == len(ords)
        assert (np.ascontiguousarray(mg[absent]).view(np.uint32) == 0xABABABAB).all()
        mu.assert_merge_equal(mg[~absent], wmg[~absent], "kept reads")
        mu.assert_stream_equal(words, oo, wout, "kept reads")
        # the same range in two halves that touch
        mg2, words2, oo2, n = g.merge_kept_pairs(total, ov, [(first, first + 8), (first + 8, end)], p, out_words_cap=cap + 9)
        mu.assert_merge_equal(mg2[~absent], wmg[~absent], "kept reads, two ranges")
        mu.assert_stream_equal(words2, oo2, wout, "kept reads, two ranges")
        # no ranges: every read is single, nothing merges
        mg3, words3, oo3, n = g.merge_kept_pairs(total, ov, (), p, out_words_cap=4)
        assert not mg3["merged"].any() and oo3.tolist() == [0] and words3.tolist() == [0] * 4
        mu.assert_merge_equal(mg3[~absent], mu.expect_merge(codes, offs, ov, p, pair_ranges=[], ordinals=ords)[0][~absent], "kept reads, no pair ranges")
        # the singles as a second range: now they are a pair; their records must say one overlap
        ov2 = ov.copy()
        ov2[end] = ov2[end + 1] = c["ov"][2 * last]
        w4 = mu.expect_merge(codes, offs, ov2, p, pair_ranges=[(first, end), (end, total)], ordinals=ords)
        mg4, words4, oo4, n = g.merge_kept_pairs(total, ov2, [(first, end), (end, total)], p, out_words_cap=cap + 9)
        mu.assert_merge_equal(mg4[~absent], w4[0][~absent], "kept reads, the singles as a pair")
        mu.assert_stream_equal(words4, oo4, w4[1], "kept reads, the singles as a pair")
        assert len(w4[1]) == len(wout) + 1 and mg4[end]["merged"] == 100
        # inconsistent records refuse the call, naming the pair and the two inserts
        ov3 = ov2.copy()
        ov3["insert"][end + 1] = 77
        small = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_MERGE_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.merge_kept_pairs(total, ov3, [(first, end), (end, total)], p, out=small, out_words_cap=cap + 9)
        assert e.value.code == pkg.SDT_EINVAL and all(s in str(e.value) for s in (str(end), "100", "77")), str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        # out_words a word short, out_offsets an entry short: SDT_EFULL with both counts set, nothing written
        for kw in (dict(out_words_cap=cap - 1), dict(out_words_cap=cap, out_reads_cap=len(wout) - 1)):
            with pytest.raises(pkg.SdtError) as e:
                g.merge_kept_pairs(total, ov, [(first, end)], p, out=small, **kw)
            assert e.value.code == pkg.SDT_EFULL and (e.value.n_merged, e.value.needed) == (len(wout), cap - 4), str(e.value)
            assert (small.view(np.uint32) == 0xABABABAB).all()
        # one record short of the highest ordinal: SDT_EFULL and nothing written
        with pytest.raises(pkg.SdtError) as e:
            g.merge_kept_pairs(total - 1, ov, [(first, end)], p, out=small[: total - 1], out_words_cap=cap)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value) and (small.view(np.uint32) == 0xABABABAB).all()
        # the parameters and the pair ranges are refused as in the dense forms
        for prm, ranges, say in ((dict(p, flags=2), [], "flags"), (dict(p, min_len=5, max_len=4), [], "max_len"), (p, [(0, 3)], "range 0"),
                                 (p, [(0, 4), (2, 6)], "range 1")):
            with pytest.raises(pkg.SdtError) as e:
                g.merge_kept_pairs(total, ov, ranges, prm, out=small, out_words_cap=cap)
            assert e.value.code == pkg.SDT_EINVAL and say in str(e.value), str(e.value)
        # (phred_offset is not looked at: the kept reads carry no qualities)
        mg5 = g.merge_kept_pairs(total, ov, [(first, end)], dict(p, phred_offset=5), out_words_cap=cap)[0]
        mu.assert_merge_equal(mg5[~absent], wmg[~absent], "kept reads, phred 5")
        # the kept reads are as they were
        bc, bo = ro.concat(r2)
        w, o, b, stride = g.fetch_kept_batch(1)
        assert (b, stride) == (base + 1, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        with pytest.raises(pkg.SdtError) as e:
            g.merge_kept_pairs(total, ov, [(first, end)], p, out_words_cap=cap)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)


# ---- 6. quality bytes through the compaction ------------------------------------------------------------------------------------------
def test_compact_quals_trimmed(pkg, synth):
    """against numpy slicing, under the same records that compact_trimmed takes on the same reads: ranges with start > 0 and with len = 0,
    all four alignments of the output mod 4, a clamped range in the device form"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 100, 150, 0, 3, 6, 250, 1, 1, 1, 0, 0, 64]
    reads = [rng.integers(0, 4, size=L, dtype=np.uint8) for L in lens]
    codes, offs = ro.concat(reads)
    quals = rng.integers(33, 127, size=len(codes), dtype=np.uint8)
    n = len(lens)
    recs = np.zeros(n, dtype=pkg.READ_TRIM_DTYPE)
    for r, L in enumerate(lens):
        s = int(rng.integers(0, L + 1))
        recs[r]["start"], recs[r]["len"] = s, (0 if r % 5 == 4 else int(rng.integers(0, L - s + 1)))
    recs["kmers"] = 0xFFFFFFFF                                                # (the first three fields are not looked at)
    assert (recs["start"] > 0).sum() >= 8 and (recs["len"] == 0).sum() >= 5 and (recs["len"] > 0).sum() >= 10
    words = synth.pack_2bit(codes)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        seen = set()
        for drop in range(4):                                                 # the last read keeps 0 .. 3 bytes fewer: every length mod 4
            rc = recs.copy()
            rc[n - 1]["start"], rc[n - 1]["len"] = 5, 40 - drop
            want, nb = mu.compact_bytes(quals, offs, rc)
            seen.add(nb % 4)
            got, gb = g.compact_quals_trimmed(quals, offs, rc)
            assert gb == nb and got.tolist() == want.tolist(), f"host form, {nb} bytes"
            # where compact_trimmed puts the bases, compact_quals_trimmed puts their qualities
            cw, co = g.compact_trimmed(words, offs, rc)
            kept = [q for q in (quals[int(offs[r]) + int(x["start"]):int(offs[r]) + int(x["start"]) + int(x["len"])] for r, x in enumerate(rc)) if len(q)]
            assert int(co[-1]) == nb and [got[int(a):int(b)].tolist() for a, b in zip(co[:-1], co[1:])] == [q.tolist() for q in kept]
            d_q = torch.from_numpy(np.concatenate([quals, np.zeros(-len(quals) % 4, dtype=np.uint8)])).to(dev)
            d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_r = torch.from_numpy(rc.view(np.int32).reshape(n, 6)).to(dev)
            d_out = torch.full((len(want) + 8,), 0xAB, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            assert g.compact_quals_trimmed_device(d_q, d_o, n, d_r, d_out, len(want)) == nb
            assert d_out.cpu().numpy().tolist() == want.tolist() + [0xAB] * 8, f"device form, {nb} bytes"
            # one byte of room short: SDT_EFULL with the count set, nothing written
            d_out.fill_(0xAB)
            torch.cuda.synchronize()
            with pytest.raises(pkg.SdtError) as e:
                g.compact_quals_trimmed_device(d_q, d_o, n, d_r, d_out, len(want) - 1)
            assert e.value.code == pkg.SDT_EFULL and e.value.needed == nb and (d_out.cpu().numpy() == 0xAB).all()
            with pytest.raises(pkg.SdtError) as e:
                g.compact_quals_trimmed(quals, offs, rc, out_cap=len(want) - 1)
            assert e.value.code == pkg.SDT_EFULL and e.value.needed == nb
        assert seen == {0, 1, 2, 3}
        # a range past the read: the host form refuses it, the device form clamps it as compact_trimmed_device does
        rc = recs.copy()
        rc[12]["start"], rc[12]["len"] = 90, 20                               # a read of 100 bases
        rc[13]["start"], rc[13]["len"] = 200, 7                               # a read of 150 bases
        with pytest.raises(pkg.SdtError) as e:
            g.compact_quals_trimmed(quals, offs, rc)
        assert e.value.code == pkg.SDT_EINVAL and "read 12" in str(e.value)
        clamped = rc.copy()
        clamped[12]["len"], clamped[13]["start"], clamped[13]["len"] = 10, 150, 0
        want, nb = mu.compact_bytes(quals, offs, clamped)
        d_r = torch.from_numpy(rc.view(np.int32).reshape(n, 6)).to(dev)
        d_out = torch.full((len(want),), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert g.compact_quals_trimmed_device(d_q, d_o, n, d_r, d_out, len(want)) == nb and d_out.cpu().numpy().tolist() == want.tolist()
        # an output that is not 4-byte aligned, and the other refusals of the host form
        with pytest.raises(pkg.SdtError) as e:
            g.compact_quals_trimmed_device(d_q, d_o, n, d_r, d_out.data_ptr() + 2, len(want))
        assert e.value.code == pkg.SDT_EINVAL and "4-byte aligned" in str(e.value)
        with pytest.raises(pkg.SdtError) as e:
            g.compact_quals_trimmed(quals[:-1], offs, recs)
        assert e.value.code == pkg.SDT_EINVAL and "quals too short" in str(e.value)
        # nothing kept; no reads
        none = np.zeros(n, dtype=pkg.READ_TRIM_DTYPE)
        got, gb = g.compact_quals_trimmed(quals, offs, none)
        assert gb == 0 and len(got) == 0
        got, gb = g.compact_quals_trimmed(quals[:0], offs[:1], none[:0])
        assert gb == 0 and len(got) == 0


# ---- 7. the chain on the device: nothing crosses to the host ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case():
    """2 000 pairs of 2 x 80 bases from fragments of 60 .. 170 bases, with the qualities of a sequencer and substitution errors where
    the qualities are low; and what every stage of the chain makes of them by the restatements, chained the same way"""
    rng = np.random.default_rng(20250613)
    L, NP = 80, 2000
    reads, quals = [], []
    for t in range(NP):
        F = int(rng.integers(60, 171))
        frag = rng.integers(0, 4, size=F, dtype=np.uint8)
        for m, strand in enumerate((frag, ro.revcomp(frag))):
            r = np.concatenate([strand, rng.integers(0, 4, size=max(L - F, 0), dtype=np.uint8)])[:L].astype(np.uint8)
            q = rq.realistic(rng, L, 2 * t + m)
            q[0] = max(q[0], 25)                                             # (no read loses all its bases: the stream stays paired)
            err = (q < 12) & (rng.random(L) < 0.2)
            r[err] = (r[err] + 1 + rng.integers(0, 3, size=int(err.sum()))) & 3
            if t % 9 == 0 and m == 1:                                        # an error that the quality trim leaves in: a mismatch column
                r[10], q[10] = (r[10] + 1) & 3, 21 + (t % 3) * 10
            reads.append(r)
            quals.append((q + 33).astype(np.uint8))
    codes, offs = ro.concat(reads)
    qbytes = np.concatenate(quals)
    qp, op, mp = rq.params(max_low_pct=100), ro.params(min_overlap=20, max_err_pct=10), mu.params()
    qrec = rq.expect_quality(qbytes, offs, qp)[0]
    assert (qrec["len"] > 0).all() and (qrec["verdict"] == rq.CLIPPED).sum() >= 500
    codes1, offs1 = ro.concat(rq.cut_reads(codes, offs, qrec))
    quals1, nb1 = mu.compact_bytes(qbytes, offs, qrec)
    assert nb1 == len(codes1)
    ov = ro.expect_overlap(codes1, offs1, op)[0]
    mg, merged = mu.expect_merge(codes1, offs1, ov, mp, quals1[:nb1])
    rest = mu.rest_reads(codes1, offs1, mg)
    # the floors of the input; a run of this counted 874 merged pairs, 2 252 reads left, 168 / 48 merged reads with such columns
    assert len(merged) >= 600 and len(rest) >= 1500 and (mg["mismatches"] > 0).sum() >= 100 and (mg["from_b"] > 0).sum() >= 20
    return dict(codes=codes, offs=offs, quals=qbytes, qp=qp, op=op, mp=mp, qrec=qrec, codes1=codes1, offs1=offs1, quals1=quals1, ov=ov, mg=mg,
                merged=merged, rest=rest)


def test_chain_on_the_device(pkg, synth):
    """quality_reads_device -> compact_trimmed_device + compact_quals_trimmed_device -> overlap_pairs_device -> merge_pairs_device ->
    compact_trimmed_device of the merge records; both streams against the restatements chained the same way, and counted into a fresh
    context against the oracle's node table of the expected reads"""
    import torch
    dev = torch.device("cuda:0")
    c = chain_case()
    n = len(c["offs"]) - 1
    words = synth.pack_2bit(c["codes"])
    nwords = len(words)
    both = c["merged"] + c["rest"]
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(*ro.concat(both))
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    i32 = lambda shape, v=-1: torch.full(shape, v, dtype=torch.int32, device=dev)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(c["offs"].view(np.int64)).to(dev)
    d_q = torch.from_numpy(np.concatenate([c["quals"], np.zeros(-len(c["quals"]) % 4, dtype=np.uint8)])).to(dev)
    d_qrec, d_ov, d_mg = i32((n, 6)), i32((n, 6)), i32((n, 6))
    d_w1, d_wm, d_wr = i32((nwords,)), i32((nwords,)), i32((nwords,))
    d_o1, d_om, d_or = (torch.zeros((n + 1,), dtype=torch.int64, device=dev) for _ in range(3))
    d_q1 = torch.full((len(d_q),), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 20) as b:
        assert a.quality_reads_device(d_q, d_o, n, d_qrec, None, c["qp"]) == n
        nr, nw = a.compact_trimmed_device(d_w, d_o, n, d_qrec, d_w1, nwords, d_o1)
        nb = a.compact_quals_trimmed_device(d_q, d_o, n, d_qrec, d_q1, len(d_q1))
        assert nr == n and nb == len(c["codes1"]) and d_o1.cpu().numpy().view(np.uint64).tolist() == c["offs1"].tolist()
        assert d_q1.cpu().numpy()[: len(c["quals1"])].tolist() == c["quals1"].tolist()
        a.overlap_pairs_device(d_w1, d_o1, n, d_ov, None, c["op"])
        nm, nwm = a.merge_pairs_device(d_w1, d_o1, n, d_ov, d_mg, d_wm, nwords, d_om, d_q1, c["mp"])
        nrr, nwr = a.compact_trimmed_device(d_w1, d_o1, n, d_mg, d_wr, nwords, d_or)
        assert nm == len(c["merged"]) and nrr == len(c["rest"])
        b.count_reads_device(d_wm, nwm + 4, d_om, nm, max(len(m) for m in c["merged"]))
        b.count_reads_device(d_wr, nwr + 4, d_or, nrr, max(len(m) for m in c["rest"]))
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
    ro.assert_overlap_equal(d_ov.cpu().numpy().view(np.uint8).copy().view(pkg.READ_OVERLAP_DTYPE).reshape(-1), c["ov"], "the overlap on the trimmed reads")
    mu.assert_merge_equal(records(pkg, d_mg), c["mg"], "the merge on the trimmed reads")
    mu.assert_stream_equal(d_wm.cpu().numpy().view(np.uint32)[: nwm + 4], d_om.cpu().numpy().view(np.uint64)[: nm + 1], c["merged"], "the merged stream")
    mu.assert_stream_equal(d_wr.cpu().numpy().view(np.uint32)[: nwr + 4], d_or.cpu().numpy().view(np.uint64)[: nrr + 1], c["rest"], "the rest")
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want
