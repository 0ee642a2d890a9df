"""GPU (-m gpu): sdt_gpu_clip_reads and its siblings against the Python restatement of the rule (read_clip_util.py).  Expectations
never come from the library under test: hits are found by walking every position and comparing base by base, the counts of the
compacted stream are the oracle's, and every output is compared for exact equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_clip_util as rc
from test_kmer_search import keys_to_int, node_dict_oracle, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31


def assert_clip(pkg, got, want, what):
    clip, keep, kept = got
    wclip, wkeep, wkept = want
    assert clip.dtype == pkg.READ_CLIP_DTYPE
    rc.assert_clip_equal(clip, wclip, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
def test_clip_equals_the_rule(pkg, synth):
    """the case under its own parameters; under min_overlap 1 with an adapter of ONE base behind the set (no shorter adapter exists,
    and none passes the check under a larger min_overlap); and under both tail masks with two letters each and no mismatch allowed"""
    c = rc.case()
    assert rc.case_holds() >= 35                          # the case contains what its names promise
    words = synth.pack_2bit(c["codes"])
    runs = [(c["adapters"], c["params"]),
            (c["adapters"] + [(np.array([rc.G], dtype=np.uint8), 0), (np.array([rc.C], dtype=np.uint8), 1)], dict(c["params"], min_overlap=1)),
            (c["adapters"][:3] + c["adapters"][7:9], dict(c["params"], max_err_pct=0, tail_err_pct=0, tail3_bases=1 << rc.A | 1 << rc.G,
                                                          tail5_bases=1 << rc.T | 1 << rc.C, min_len=0, min_tail=3)),
            ([], dict(c["params"], tail3_bases=0, tail5_bases=0))]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for i, (adapters, p) in enumerate(runs):
            want = rc.case_expect() if i == 0 else rc.expect_clip(c["codes"], c["offs"], adapters, p)
            assert_clip(pkg, g.clip_reads(words, c["offs"], adapters, p), want, f"run {i}")
            if i == 1:
                assert (want[0]["adapters"] & 0xFFFF == len(adapters) - 1).any() and (want[0]["adapters"] >> 16 == len(adapters)).any()
            if i == 3:
                assert (want[0]["verdict"][np.diff(c["offs"].astype(np.int64)) >= 20] == rc.WHOLE).all()
        clip, keep, kept = g.clip_reads(words, c["offs"][:1], c["adapters"], c["params"])
        assert len(clip) == 0 and len(keep) == 0 and kept == 0


# ---- 2. what is refused ---------------------------------------------------------------------------------------------------------------
def test_clip_refusals(pkg, synth):
    c = rc.case()
    words = synth.pack_2bit(c["codes"])
    offs = c["offs"]
    n = len(offs) - 1
    good = c["params"]
    seq = lambda m: np.arange(m, dtype=np.uint8) & 3
    untouched = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLIP_DTYPE)

    def refused(adapters, p, *say):
        prm, aset, alive = pkg.PregraphGPU._clip_args(adapters, p)
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_clip_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, ctypes.addressof(prm), ctypes.addressof(aset),
                                        untouched.ctypes.data, None, ctypes.byref(kept))
        msg = g.lib.sdt_gpu_last_error().decode()
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and kept.value == 0

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(c["adapters"], dict(good, flags=1), "flags", "0x1")
        refused(c["adapters"], dict(good, min_overlap=0), "min_overlap", "0")
        refused(c["adapters"], dict(good, max_err_pct=101), "max_err_pct", "101")
        refused(c["adapters"], dict(good, tail_err_pct=200), "tail_err_pct", "200")
        refused(c["adapters"], dict(good, tail3_bases=16), "tail3_bases", "0x10")
        refused(c["adapters"], dict(good, tail5_bases=31), "tail5_bases", "0x1f")
        refused(c["adapters"], dict(good, min_tail=0), "min_tail", "0")
        refused([(seq(5), 0)] * 257, good, "n", "257")
        refused([(seq(33), 0), (seq(129), 1)], good, "adapter 1", "129")
        refused([(seq(33), 0), (seq(0), 0)], good, "adapter 1", "0 bases")
        refused([(seq(4), 0)], good, "adapter 0", "4 bases", "min_overlap = 5")
        refused([(seq(33), 0), (seq(40), 2)], good, "ends[1]", "2")
        aset, alive = pkg.pack_adapters([(seq(33), 0), (seq(40), 1), (seq(20), 0)])
        alive[1][2] = 30                                  # adapter 1 ends before it starts
        refused((aset, alive), good, "offsets", "adapter 1")
        # NULL params
        aset, alive = pkg.pack_adapters(c["adapters"])
        code = g.lib.sdt_gpu_clip_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, None, ctypes.addressof(aset),
                                        untouched.ctypes.data, None, None)
        assert code == pkg.SDT_EINVAL and "params" in g.lib.sdt_gpu_last_error().decode()
        # NULL adapters means none; min_tail == 0 is fine without a tail mask; the boundaries pass
        prm = pkg.ClipParams(**dict(good, min_tail=0, tail3_bases=0, tail5_bases=0))
        out = np.zeros(n, dtype=pkg.READ_CLIP_DTYPE)
        kept = ctypes.c_uint64()
        assert g.lib.sdt_gpu_clip_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, ctypes.addressof(prm), None, out.ctypes.data,
                                        None, ctypes.byref(kept)) == pkg.SDT_OK
        rc.assert_clip_equal(out, rc.expect_clip(c["codes"], c["offs"], [], dict(good, min_tail=0, tail3_bases=0, tail5_bases=0))[0], "no adapters")
        g.clip_reads(words, offs, [(seq(5), 1)] * 256, dict(good, max_err_pct=100, tail_err_pct=100, tail3_bases=15, tail5_bases=15))
        g.clip_reads(words, offs, [(seq(128), 0)], good)
        # no reads: SDT_OK whatever the rest says
        clip, keep, kept = g.clip_reads(words, offs[:1], c["adapters"], dict(good, flags=7))
        assert len(clip) == 0 and kept == 0


# ---- 3. where the reads and the adapters start ----------------------------------------------------------------------------------------
def test_clip_is_alignment_independent(pkg, synth):
    """the same reads behind one filler read of 0 .. 15 bases, and with offsets[0] = 7: every read starts at another base of its word;
    the same adapters behind one filler adapter of 12 .. 27 bases: every adapter starts at another base of its word, and every index
    is one higher.  A read is judged on its own, so its record is the one it had"""
    c = rc.case()
    base = rc.case_expect()
    p = c["params"]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            filler = np.full(f, rc.G, dtype=np.uint8)
            filler[::2] = rc.C                                                # CGCG...
            codes, offs = rc.concat([filler] + c["reads"])
            first = rc.expect_clip(filler, np.array([0, f], dtype=np.uint64), c["adapters"], p)
            want = tuple(np.concatenate([a, b]) for a, b in zip(first[:2], base[:2])) + (first[2] + base[2],)
            assert_clip(pkg, g.clip_reads(synth.pack_2bit(codes), offs, c["adapters"], p), want, f"{f} filler bases")
        shifted = np.concatenate([np.full(7, rc.T, dtype=np.uint8), c["codes"]])
        assert_clip(pkg, g.clip_reads(synth.pack_2bit(shifted), c["offs"] + np.uint64(7), c["adapters"], p), base, "offsets[0] = 7")
        for f in range(12, 28):
            filler = np.full(f, rc.T, dtype=np.uint8)
            filler[1::2] = rc.G                                               # TGTG...: as a 3' adapter it bounds no read of the case
            assert all(rc.hit3(r, filler, p["min_overlap"], p["max_err_pct"]) is None for r in c["reads"])
            want = (rc.shift_adapter_ids(base[0], 1),) + base[1:]
            assert_clip(pkg, g.clip_reads(synth.pack_2bit(c["codes"]), c["offs"], [(filler, 0)] + c["adapters"], p), want, f"a filler adapter of {f} bases")


# ---- 4. a host batch in pieces --------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_clip_util as rc
c = rc.case()
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    clip, keep, kept = g.clip_reads(synth.pack_2bit(c["codes"]), c["offs"], c["adapters"], c["params"])
np.savez({path!r}, clip=clip, keep=keep, kept=np.uint64(kept))
"""


def test_clip_in_pieces(pkg, synth, tmp_path):
    """SDT_SEARCH_CHUNK = 7: the host form stages 18 pieces of 7 reads (the last of fewer), each rebased to its first word"""
    c = rc.case()
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SEARCH_CHUNK="7")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    got = (hooked["clip"], hooked["keep"], int(hooked["kept"]))
    assert_clip(pkg, got, rc.case_expect(), "pieces of 7 reads")
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert_clip(pkg, got, g.clip_reads(synth.pack_2bit(c["codes"]), c["offs"], c["adapters"], c["params"]), "pieces against the unhooked run")


# ---- 5. clip, compact, count: nothing crosses to the host -----------------------------------------------------------------------------
def test_clip_device_form_and_compaction(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    L = 100
    _, codes, offs = workload(synth, K, L, n_reads=300)
    rng = np.random.default_rng(11)
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    reads = [r for r in reads if len(r) >= K + 1][:240]
    assert len(reads) == 240
    ad3, ad5 = rc.case()["adapters"][2][0], rc.case()["adapters"][8][0]
    for i in range(0, 240, 3):                            # a third of the reads carry a read-through adapter, a tail, a 5' remnant or all of them
        cut = int(rng.integers(20, len(reads[i])))
        kind = i // 3 % 4
        r = reads[i][:cut]
        if kind in (1, 3):
            r = np.concatenate([r, np.full(int(rng.integers(8, 30)), rc.A, dtype=np.uint8)])
        if kind in (0, 1, 3):
            r = np.concatenate([r, ad3[:int(rng.integers(6, 34))]])
        if kind in (2, 3):
            r = np.concatenate([ad5[-int(rng.integers(6, 34)):], np.full(int(rng.integers(0, 15)), rc.T, dtype=np.uint8), r])
        reads[i] = r.astype(np.uint8)
    codes, offs = rc.concat(reads)
    n = len(offs) - 1
    adapters = [(ad3, 0), (ad5, 1)]
    p = rc.params(min_len=K + 1, min_tail=6, tail3_bases=1 << rc.A, tail5_bases=1 << rc.T)
    wclip, wkeep, wkept = rc.expect_clip(codes, offs, adapters, p)
    assert {rc.WHOLE, rc.CLIPPED, rc.DROPPED} == set(wclip["verdict"].tolist()) and (wclip["tail3"] > 0).sum() >= 20 and (wclip["tail5"] > 0).sum() >= 10
    assert (wclip["adapters"] >> 16 > 0).sum() >= 20 and (wclip["adapters"] & 0xFFFF > 0).sum() >= 40
    kcodes, koffs = rc.concat(rc.clipped_reads(codes, offs, wclip))
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_clip = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    # the clip runs on a context that never counts (a contig index) and before any count: it needs no table
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        assert a.clip_reads_device(d_w, d_o, n, d_clip, d_keep, adapters, p) == wkept
        assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
        assert a.clip_reads_device(d_w, d_o, n, d_clip, None, adapters, p) == wkept                 # d_keep may be NULL
        assert a.clip_reads_device(d_w, d_o, 0, None) == 0
        nr, nw = a.compact_trimmed_device(d_w, d_o, n, d_clip, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, int(np.diff(koffs.astype(np.int64)).max()))
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
        # the host form on the same kind of context
        assert_clip(pkg, a.clip_reads(words, offs, adapters, p), (wclip, wkeep, wkept), "a contig index, host form")
    got_clip = d_clip.cpu().numpy().view(np.uint8).copy().view(pkg.READ_CLIP_DTYPE).reshape(-1)
    rc.assert_clip_equal(got_clip, wclip, "device form")
    assert d_oo.cpu().numpy()[: nr + 1].tolist() == koffs.tolist()
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want


# ---- 6. kept reads ----------------------------------------------------------------------------------------------------------------
def test_clip_kept_reads(pkg, synth):
    """the layout of the host program: the read-1 file as one kept batch (ordinals base, base + 2, ...), the read-2 file as another
    (base + 1, base + 3, ...); no read has ordinals 0 .. 2, and the read-2 file is one read short"""
    c = rc.case()
    rng = np.random.default_rng(78)
    pool = [r for r, n in zip(c["reads"], c["names"]) if 40 <= len(r) <= 200]
    P, base = 14, 3
    r1 = [pool[int(i)] for i in rng.permutation(len(pool))[:P + 1]]
    r2 = [pool[int(i)] for i in rng.permutation(len(pool))[:P]]
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)]
    codes, offs = rc.concat(r1 + r2)
    total = base + 2 * (P + 1)
    absent = np.ones(total, dtype=bool)
    absent[ords] = False
    assert absent.sum() == 4
    wclip, wkeep, wkept = rc.expect_clip(codes, offs, c["adapters"], c["params"], ordinals=ords)
    assert len(wclip) == total - 1 and {rc.WHOLE, rc.CLIPPED} <= set(wclip["verdict"][~absent[:-1]].tolist())
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for batch, b in ((r1, base), (r2, base + 1)):
            g.set_read_ordinal(b, 2)
            bc, bo = rc.concat(batch)
            g.push_reads(synth.pack_2bit(bc), bo)
        g.finish_count()
        out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLIP_DTYPE)
        clip, n, kept = g.clip_kept_reads(total, c["adapters"], c["params"], out=out)
        assert n == len(ords) and kept == wkept
        assert (np.ascontiguousarray(clip[absent]).view(np.uint32) == 0xABABABAB).all()
        rc.assert_clip_equal(clip[:-1][~absent[:-1]], wclip[~absent[:-1]], "kept reads")
        # exactly the records up to the highest ordinal fit
        clip, n, kept = g.clip_kept_reads(total - 1, c["adapters"], c["params"])
        rc.assert_clip_equal(clip, wclip, "kept reads, out_capacity = highest ordinal + 1")
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 2, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLIP_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.clip_kept_reads(total - 2, c["adapters"], c["params"], out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.clip_kept_reads(total, c["adapters"], dict(c["params"], flags=2))
        assert e.value.code == pkg.SDT_EINVAL
        # the kept reads are as they were
        bc, bo = rc.concat(r2)
        w, o, b, stride = g.fetch_kept_batch(1)
        assert (b, stride) == (base + 1, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        with pytest.raises(pkg.SdtError) as e:
            g.clip_kept_reads(total, c["adapters"], c["params"])
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
