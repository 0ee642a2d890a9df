"""GPU (-m gpu): sdt_gpu_quality_reads and its device form against the numpy restatement of the rule (read_quality_util.py).
Expectations never come from the library under test: the segment is found by prefix sums and a running minimum on the CPU, the counts
of the compacted stream are the oracle's, and every output is compared for exact equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_quality_util as qu
from read_dedup_util import concat
from test_kmer_search import keys_to_int, node_dict_oracle, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31


def assert_q(pkg, got, want, what):
    out, keep, kept = got
    wout, wkeep, wkept = want
    assert out.dtype == pkg.READ_QUALITY_DTYPE
    qu.assert_q_equal(out, wout, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
VARIATIONS = (dict(), dict(cut_q=0), dict(cut_q=93), dict(phred_offset=0), dict(phred_offset=64), dict(max_low_pct=100), dict(low_q=0),
              dict(max_ee_ppm=1000), dict(max_ee_ppm=10000), dict(max_ee_ppm=100000), dict(max_ee_ppm=0, min_len=0))


def test_quality_equals_the_rule(pkg):
    """the case under its own parameters; without trimming and with a cut no base passes; under the other two offsets; with the low
    filter off either way; with the error filter at three thresholds and off"""
    c = qu.case()
    assert qu.case_holds() >= 30                          # the case contains what its names promise
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for kw in VARIATIONS:
            assert_q(pkg, g.quality_reads(c["quals"], c["offs"], dict(c["params"], **kw)), qu.case_expect(**kw), f"{kw}")
        out, keep, kept = g.quality_reads(c["quals"], c["offs"][:1], c["params"])
        assert len(out) == 0 and len(keep) == 0 and kept == 0


# ---- 2. what is refused ---------------------------------------------------------------------------------------------------------------
def test_quality_refusals(pkg):
    c = qu.case()
    quals, offs = c["quals"], c["offs"]
    n = len(offs) - 1
    good = c["params"]
    untouched = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_QUALITY_DTYPE)
    keep = np.full(n, 0xAB, dtype=np.uint8)

    def call(prm, nbytes=quals.size, o=offs):
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_quality_reads(g._ctx, quals.ctypes.data, nbytes, o.ctypes.data, n, ctypes.addressof(prm) if prm is not None else None,
                                           untouched.ctypes.data, keep.ctypes.data, ctypes.byref(kept))
        return code, g.lib.sdt_gpu_last_error().decode(), kept.value

    def refused(p, *say, **kw):
        code, msg, kept = call(pkg.QualityParams(**p) if p is not None else None, **kw)
        assert code == pkg.SDT_EINVAL and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and (keep == 0xAB).all() and kept == 0

    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        refused(None, "sdt_quality_params is NULL")
        for v in (1, 32, 34, 63, 65, 0xFFFFFFFF):
            refused(dict(good, phred_offset=v), "phred_offset", f"= {v}")
        refused(dict(good, cut_q=94), "cut_q", "= 94")
        refused(dict(good, low_q=94), "low_q", "= 94")
        refused(dict(good, max_low_pct=101), "max_low_pct", "= 101")
        refused(dict(good, flags=1), "flags", "0x1")
        refused(dict(good, flags=0x80000000), "flags", "0x80000000")
        refused(dict(good, reserved=7), "reserved", "= 7")
        # the stream: offsets that descend, fewer bytes than the offsets say
        bad = offs.copy()
        bad[5] = bad[6] + np.uint64(1)
        refused(good, "offsets not monotonic", "read 5", o=bad)
        refused(good, "quals too short", f"{int(offs[-1])} bytes", nbytes=int(offs[-1]) - 1)
        # the boundaries pass, and so does a NULL keep
        for q in (dict(good, cut_q=93, low_q=93, max_low_pct=100), dict(good, cut_q=0, low_q=0, max_low_pct=0), dict(good, phred_offset=64, max_ee_ppm=0xFFFFFFFF),
                  dict(good, phred_offset=0, min_len=0xFFFFFFFF)):
            prm = pkg.QualityParams(**q)
            out = np.zeros(n, dtype=pkg.READ_QUALITY_DTYPE)
            kept = ctypes.c_uint64()
            assert g.lib.sdt_gpu_quality_reads(g._ctx, quals.ctypes.data, quals.size, offs.ctypes.data, n, ctypes.addressof(prm), out.ctypes.data, None,
                                               ctypes.byref(kept)) == pkg.SDT_OK
            want = qu.expect_quality(quals, offs, q)
            qu.assert_q_equal(out, want[0], f"{q}")
            assert kept.value == want[2]
        # no reads: SDT_OK whatever the rest says
        out, _, kept = g.quality_reads(quals, offs[:1], dict(good, flags=6, phred_offset=7, reserved=1))
        assert len(out) == 0 and kept == 0
        kept = ctypes.c_uint64(99)
        assert g.lib.sdt_gpu_quality_reads_device(g._ctx, None, None, 0, None, None, None, ctypes.byref(kept)) == pkg.SDT_OK and kept.value == 0


# ---- 3. where the reads start ---------------------------------------------------------------------------------------------------------
def test_quality_is_alignment_independent(pkg):
    """the same reads behind one filler read of 0 .. 7 bytes, the host form with offsets[0] = 5, and the device form on a stream that
    starts 1, 2 and 3 bytes into a word of its buffer: every read starts at another byte of its word, and the bytes around a read are
    never those it had.  A read is judged on its own, so its record is the one it had"""
    import torch
    dev = torch.device("cuda:0")
    c = qu.case()
    p = c["params"]
    base = qu.case_expect()
    n = len(c["reads"])
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(8):
            filler = np.full(f, 33 + 40, dtype=np.uint8)
            quals, offs = qu.concat_bytes([filler] + c["reads"])
            first = qu.expect_quality(filler, np.array([0, f], dtype=np.uint64), p)
            want = tuple(np.concatenate([a, b]) for a, b in zip(first[:2], base[:2])) + (first[2] + base[2],)
            assert_q(pkg, g.quality_reads(quals, offs, p), want, f"{f} filler bytes")
        shifted = np.concatenate([np.full(5, 255, dtype=np.uint8), c["quals"]])
        assert_q(pkg, g.quality_reads(shifted, c["offs"] + np.uint64(5), p), base, "offsets[0] = 5")
        for lead in (1, 2, 3):
            buf = np.concatenate([np.full(lead, 255, dtype=np.uint8), c["quals"], np.full(8, 255, dtype=np.uint8)])
            d_q = torch.from_numpy(buf).to(dev)
            d_o = torch.from_numpy((c["offs"] + np.uint64(lead)).view(np.int64)).to(dev)
            d_out = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            assert d_q.data_ptr() % 4 == 0
            kept = g.quality_reads_device(d_q, d_o, n, d_out, d_keep, p)
            out = d_out.cpu().numpy().view(np.uint8).copy().view(pkg.READ_QUALITY_DTYPE).reshape(-1)
            assert_q(pkg, (out, d_keep.cpu().numpy(), kept), base, f"the device form, {lead} bytes into a word")
        # a stream that does not start at a word is refused by its address, not read
        with pytest.raises(pkg.SdtError) as e:
            g.quality_reads_device(d_q.data_ptr() + 1, d_o, n, d_out, None, p)
        assert e.value.code == pkg.SDT_EINVAL and "4-byte aligned" in str(e.value)


# ---- 4. a host batch in pieces --------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
import read_quality_util as qu
c = qu.case()
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    out, keep, kept = g.quality_reads(c["quals"], c["offs"], c["params"])
np.savez({path!r}, out=out, keep=keep, kept=np.uint64(kept))
"""


def test_quality_in_pieces(pkg, tmp_path):
    """SDT_SEARCH_CHUNK = 7: the host form stages 22 pieces of 7 reads (the last of fewer), each from a 4-byte-aligned byte of the
    stream; the reads of 1 000 and 5 000 bytes are among them, and most pieces start inside a word"""
    c = qu.case()
    starts = c["offs"][:-1:7].astype(np.int64)
    assert (starts % 4 != 0).sum() >= 10 and max(len(r) for r in c["reads"]) == 5000
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SEARCH_CHUNK="7")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    got = (hooked["out"], hooked["keep"], int(hooked["kept"]))
    assert_q(pkg, got, qu.case_expect(), "pieces of 7 reads")
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert_q(pkg, got, g.quality_reads(c["quals"], c["offs"], c["params"]), "pieces against the unhooked run")


# ---- 5. quality, compact, count: nothing crosses to the host --------------------------------------------------------------------------
def test_quality_device_form_and_compaction(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    _, codes, offs = workload(synth, K, 150, n_reads=300)
    rng = np.random.default_rng(12)
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    reads = [r.copy() for r in reads if len(r) >= K + 1][:240]
    assert len(reads) == 240
    codes, offs = concat(reads)
    n = len(offs) - 1
    quals, qoffs = qu.concat_bytes([(qu.realistic(rng, len(r), i) + 33).astype(np.uint8) for i, r in enumerate(reads)])
    assert qoffs.tolist() == offs.tolist()
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_q = torch.from_numpy(quals).to(dev)
    p = qu.params(min_len=K + 1, max_ee_ppm=20000)
    wout, wkeep, wkept = qu.expect_quality(quals, offs, p)
    v = wout["verdict"]
    assert (v == qu.WHOLE).sum() >= 20 and (v == qu.CLIPPED).sum() >= 60 and (v == qu.DROPPED).sum() >= 10 and (wout["start"] > 0).sum() >= 20
    kcodes, koffs = concat(qu.cut_reads(codes, offs, wout))
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (x[0], x[1] & 0xFFFFFF, x[2]) for k, x in node_dict_oracle(o2).items()}
    d_out = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    # the stage runs on a context that never counts (a contig index) and before any count: it needs no table
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        assert a.quality_reads_device(d_q, d_o, n, d_out, d_keep, p) == wkept
        assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
        assert a.quality_reads_device(d_q, d_o, n, d_out, None, p) == wkept                        # d_keep may be NULL
        assert a.quality_reads_device(d_q, d_o, 0, None) == 0
        nr, nw = a.compact_trimmed_device(d_w, d_o, n, d_out, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, int(np.diff(koffs.astype(np.int64)).max()))
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
        # the host form on the same kind of context
        assert_q(pkg, a.quality_reads(quals, offs, p), (wout, wkeep, wkept), "a contig index, host form")
    got_out = d_out.cpu().numpy().view(np.uint8).copy().view(pkg.READ_QUALITY_DTYPE).reshape(-1)
    qu.assert_q_equal(got_out, wout, "device form")
    assert d_oo.cpu().numpy()[: nr + 1].tolist() == koffs.tolist()
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want


# ---- 6. long reads ----------------------------------------------------------------------------------------------------------------
def test_quality_of_long_reads(pkg):
    """40 reads of 3 000 .. 20 000 bases whose best segment lies in a random place: qualities of 2 .. 19 everywhere but for one
    stretch of 25 .. 40, with single low bases inside it; the minimum, the best end and the start of a step (256 bases) fall anywhere"""
    rng = np.random.default_rng(6)
    reads = []
    for _ in range(40):
        L = int(rng.integers(3000, 20001))
        q = rng.integers(2, 20, L)
        n = int(rng.integers(200, L - 200))
        at = int(rng.integers(0, L - n + 1))
        q[at:at + n] = rng.integers(25, 41, n)
        q[at + rng.integers(0, n, n // 50)] = 2
        reads.append((q + 33).astype(np.uint8))
    quals, offs = qu.concat_bytes(reads)
    p = qu.params(min_len=100, max_ee_ppm=50000)
    want = qu.expect_quality(quals, offs, p)
    assert (want[0]["verdict"] == qu.CLIPPED).sum() >= 30 and (want[0]["start"] > 256).sum() >= 30 and (want[0]["span"] > 1000).sum() >= 20
    assert (want[0]["low"] > 0).sum() >= 30
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert_q(pkg, g.quality_reads(quals, offs, p), want, "long reads")
        # the same without trimming: every step of every read is measured
        assert_q(pkg, g.quality_reads(quals, offs, dict(p, cut_q=0, max_low_pct=100, max_ee_ppm=0)), qu.expect_quality(quals, offs, dict(p, cut_q=0, max_low_pct=100, max_ee_ppm=0)),
                 "long reads, whole")


def test_quality_gain_past_2_30(pkg):
    """One read whose running gain P - M passes 2^30: from there on the kernel holds the carried minimum, relative to P, at -2^30 (Mr)
    and takes the gain from the 64-bit values.  cut_q = 40: a base of quality 93 adds 53, a base of quality 0 takes away 40, so the
    gain needs 2^30 / 53 = 20.3 M bases.  The read: 1 000 bases of quality 0 (the minimum lies at base 1 000, not at 0), quality 93
    with 3 000 single bases of quality 2 until the gain is 500 bases past 2^30, a dip of 1 000 bases of quality 0 (40 000 down: the
    gain falls below 2^30 again and passes it a second time behind the dip), 100 000 bases of quality 93, 500 bases of quality 0.
    Its best segment starts at base 1 000 and ends 500 bases before the end.  The reads before and after it are ordinary ones: nothing
    carries over."""
    import torch
    dev = torch.device("cuda:0")
    p = qu.params(cut_q=40, phred_offset=33, low_q=15, max_low_pct=100, max_ee_ppm=0, min_len=1)
    up, down, low_down = qu.MAX_Q - p["cut_q"], p["cut_q"], p["cut_q"] - 2
    assert (up, down) == (53, 40)
    head, n_low, dip, tail, end = 1000, 3000, 1000, 100000, 500
    rise = -(-((1 << 30) + n_low * (up + low_down)) // up) + 500              # bases from the minimum until the gain is 500 bases past 2^30
    L = head + rise + dip + tail + end
    q = np.full(L, qu.MAX_Q, dtype=np.int64)
    q[:head] = 0
    rng = np.random.default_rng(230)
    stride = rise // n_low
    lows = head + np.arange(n_low) * stride + rng.integers(0, stride, n_low)
    q[lows] = 2
    q[head + rise:head + rise + dip] = 0
    q[L - end:] = 0
    before = (qu.realistic(rng, 150, 0) + 33).astype(np.uint8)
    after = (qu.realistic(rng, 150, 1) + 33).astype(np.uint8)
    quals, offs = qu.concat_bytes([before, (q + 33).astype(np.uint8), after])
    # on the input itself: the gain before the dip, behind it, and at the best end
    P = np.concatenate([[0], np.cumsum(q - p["cut_q"])])
    gain = P - np.minimum.accumulate(P)
    at_dip = head + rise
    assert 20_000_000 < L < 21_000_000 and len(np.unique(lows)) == n_low and lows.max() < at_dip
    assert gain[:at_dip + 1].max() == gain[at_dip] > 1 << 30 and int(np.argmax(gain > 1 << 30)) <= L - 100000
    assert gain[at_dip + dip] < 1 << 30 < gain[at_dip + dip + tail] == gain.max() and int(np.argmin(P)) == head
    span = L - head - end
    want = qu.expect_quality(quals, offs, p)
    middle = (span, n_low + dip, (n_low * int(qu.EE_PPM[2]) + dip * int(qu.EE_PPM[0])) // span, head, span, qu.CLIPPED)
    assert tuple(int(x) for x in want[0][1].tolist()) == middle
    lone = [qu.expect_quality(r, np.array([0, len(r)], dtype=np.uint64), p)[0][0] for r in (before, after)]
    assert want[0][0].tolist() == lone[0].tolist() and want[0][2].tolist() == lone[1].tolist()
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        host = g.quality_reads(quals, offs, p)
        assert_q(pkg, host, want, "the host form")
        d_q = torch.from_numpy(np.concatenate([quals, np.zeros(-len(quals) % 4, dtype=np.uint8)])).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_out = torch.full((3, 6), -3, dtype=torch.int32, device=dev)
        d_keep = torch.full((3,), 7, dtype=torch.uint8, device=dev)
        kept = g.quality_reads_device(d_q, d_o, 3, d_out, d_keep, p)
        out = d_out.cpu().numpy().view(np.uint8).copy().view(pkg.READ_QUALITY_DTYPE).reshape(-1)
        assert_q(pkg, (out, d_keep.cpu().numpy(), kept), want, "the device form")
        assert_q(pkg, (out, d_keep.cpu().numpy(), kept), host, "the device form against the host form")
