"""GPU (-m gpu): sdt_gpu_dedup_reads and its siblings against the Python restatement of the rule (read_dedup_util.py).  Expectations
never come from the library under test: a class is an entry of a dictionary keyed on the reads' lengths and bases, the counts of the
compacted stream are the oracle's, and every output is compared for exact equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_dedup_util as rd
from read_select_util import ranged_units
from test_kmer_search import keys_to_int, node_dict_oracle, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31
RUNS = [(False, 0), (False, rd.MATE_SWAP), (True, 0), (True, rd.MATE_SWAP)]


def the_case(paired):
    return rd.paired_case() if paired else rd.case()


def assert_dedup(pkg, got, want, what):
    dup, keep, kept = got
    wdup, wkeep, wkept = want
    assert dup.dtype == pkg.READ_DUP_DTYPE
    rd.assert_dup_equal(dup, wdup, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,flags", RUNS)
def test_dedup_equals_the_rule(pkg, synth, paired, flags):
    c = the_case(paired)
    words = synth.pack_2bit(c["codes"])
    want = rd.expect_dedup(c["codes"], c["offs"], paired=paired, flags=flags)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert_dedup(pkg, g.dedup_reads(words, c["offs"], paired=paired, flags=flags), want, f"paired={paired} flags={flags}")
        dup, keep, kept = g.dedup_reads(words, c["offs"][:1], paired=paired, flags=flags)
        assert len(dup) == 0 and len(keep) == 0 and kept == 0
        with pytest.raises(pkg.SdtError) as e:
            g.dedup_reads(words, c["offs"], paired=paired, flags=flags | 2)
        assert e.value.code == pkg.SDT_EINVAL and "flags" in str(e.value)
        if paired:
            with pytest.raises(pkg.SdtError) as e:
                g.dedup_reads(words, c["offs"][:-1], paired=True, flags=flags)
            assert e.value.code == pkg.SDT_EINVAL and "odd" in str(e.value)
    # the case holds what it says (more of it: test_read_dedup_host.py)
    wdup = want[0]
    assert ({1, 2, 4, 9} if paired and flags else {1, 2, 3, 7}) <= set(wdup["copies"].tolist()) and len(set(wdup["first"].tolist())) <= 64
    if paired:
        plain = rd.expect_dedup(c["codes"], c["offs"], paired=True)[0]
        swap = rd.expect_dedup(c["codes"], c["offs"], paired=True, flags=rd.MATE_SWAP)[0]
        assert ((plain["verdict"] == rd.KEPT) & (swap["verdict"] == rd.DROPPED)).any(), "no pair is dropped only under the flag"
        # (a, b) three times, (b, a), (a, c), (a, a): four classes without the flag, three with it
        special = [i for i, (x, y) in enumerate(c["pairs"]) if x is c["a"] or y is c["a"]]
        assert len(special) == 6
        assert len({int(plain["first"][2 * i]) for i in special}) == 4 and len({int(swap["first"][2 * i]) for i in special}) == 3
    else:
        seq_reads = {i for i, o in enumerate(c["origin"]) if o[0] == "seq"}
        twins = [i for i, o in enumerate(c["origin"]) if o[0] == "twin"]
        assert len(twins) >= 13 and all(int(wdup["first"][i]) not in seq_reads for i in twins), "a near-miss twin is dropped"
        assert (np.diff(c["offs"].astype(np.int64)) == 0).sum() == 2 and 5000 in np.diff(c["offs"].astype(np.int64))


# ---- 2. where the stream starts -----------------------------------------------------------------------------------------------------
def test_dedup_is_geometry_and_alignment_independent(pkg, synth):
    """the same reads behind one filler read of 0 .. 15 bases: every read starts at another base of its word and every unit id is one
    higher; the classes are the same"""
    c = rd.case()
    n = len(c["offs"]) - 1
    base = rd.expect_dedup(c["codes"], c["offs"])[0]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for f in range(16):
            filler = np.full(f, 3, dtype=np.uint8)
            filler[::2] = 1                                                   # CGCG...: no read of the case
            codes, offs = rd.concat([filler] + c["reads"])
            want = rd.expect_dedup(codes, offs)
            got = g.dedup_reads(synth.pack_2bit(codes), offs)
            assert_dedup(pkg, got, want, f"{f} filler bases")
            if f and want[0]["copies"][0] == 1:                               # (the filler of 0 bases joins the empty reads)
                assert (got[0]["first"][1:] == base["first"] + 1).all() and (got[0]["copies"][1:] == base["copies"]).all()
                assert (got[0]["verdict"][1:] == base["verdict"]).all()
        # the stream itself need not start at base 0 of its first word
        shifted = np.concatenate([np.full(7, 2, dtype=np.uint8), c["codes"]])
        got = g.dedup_reads(synth.pack_2bit(shifted), c["offs"] + np.uint64(7))
        rd.assert_dup_equal(got[0], base, "offsets[0] = 7")
    assert n == len(base)


# ---- 3. collisions of fingerprints --------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_dedup_util as rd
out = {{}}
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    for paired, flags in {runs!r}:
        c = rd.paired_case() if paired else rd.case()
        dup, keep, kept = g.dedup_reads(synth.pack_2bit(c["codes"]), c["offs"], paired=paired, flags=flags)
        out[f"dup_{{int(paired)}}_{{flags}}"], out[f"keep_{{int(paired)}}_{{flags}}"], out[f"kept_{{int(paired)}}_{{flags}}"] = dup, keep, np.uint64(kept)
np.savez({path!r}, **out)
"""


@pytest.mark.parametrize("bits", [64, 8, 3, 1])
def test_dedup_survives_fingerprint_collisions(pkg, synth, tmp_path, bits):
    """SDT_DEDUP_FP_BITS keeps the low bits of every unit fingerprint: with 3 bits the 27 to 62 classes of a run share 8 values, so
    at least four to eight rounds are needed; with 1 bit as many rounds as the fuller of two slots has classes.  The case has at most 64
    classes per run, so the cap of 64 rounds cannot bind: every round resolves a class at least.  A fresh process per setting."""
    path = str(tmp_path / "records.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_DEDUP_FP_BITS=str(bits))
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), runs=RUNS, path=path)], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hooked = np.load(path)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        for paired, flags in RUNS:
            c = the_case(paired)
            want = rd.expect_dedup(c["codes"], c["offs"], paired=paired, flags=flags)
            classes = len(set(want[0]["first"].tolist()))
            assert 20 <= classes <= 64
            tag = f"{int(paired)}_{flags}"
            got = (hooked[f"dup_{tag}"], hooked[f"keep_{tag}"], int(hooked[f"kept_{tag}"]))
            assert_dedup(pkg, got, want, f"{bits} bits, paired={paired} flags={flags}")
            plain = g.dedup_reads(synth.pack_2bit(c["codes"]), c["offs"], paired=paired, flags=flags)
            assert_dedup(pkg, got, plain, f"{bits} bits against the unhooked run, paired={paired} flags={flags}")


# ---- 4. dedup, compact, count: nothing crosses to the host ----------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_dedup_device_form_and_compaction(pkg, synth, paired):
    import torch
    dev = torch.device("cuda:0")
    L = 100
    _, codes, offs = workload(synth, K, L, n_reads=300)
    rng = np.random.default_rng(5)
    reads = [codes[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    reads = [r for r in reads if len(r) >= K + 1][:240]
    assert len(reads) == 240
    units = [tuple(reads[2 * t:2 * t + 2]) for t in range(120)] if paired else [(r,) for r in reads]
    units = units + [units[int(i)] for i in rng.integers(0, len(units), size=len(units) // 2)]          # planted copies
    if paired:
        units += [(b, a) for a, b in units[:10]]                                                        # not copies without the flag
    units = [units[int(i)] for i in rng.permutation(len(units))]
    codes, offs = rd.concat([r for u in units for r in u])
    n = len(offs) - 1
    wdup, wkeep, wkept = rd.expect_dedup(codes, offs, paired=paired)
    assert n // 2 < wkept < n - n // 5
    kcodes, koffs = rd.concat([codes[int(offs[r]):int(offs[r + 1])] for r in range(n) if wkeep[r]])
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_dup = torch.full((n, 2), -3, dtype=torch.int64, device=dev)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        assert a.dedup_reads_device(d_w, d_o, n, d_dup, d_keep, paired=paired) == wkept
        assert a.dedup_reads_device(d_w, d_o, n, d_dup, None, paired=paired) == wkept             # d_keep may be NULL
        assert a.dedup_reads_device(d_w, d_o, 0, None) == 0
        nr, nw = a.compact_reads_device(d_w, d_o, n, d_keep, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, L)
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
    got_dup = d_dup.cpu().numpy().view(np.uint8).copy().view(pkg.READ_DUP_DTYPE).reshape(-1)
    rd.assert_dup_equal(got_dup, wdup, "device form")
    assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want


# ---- 5. kept reads ----------------------------------------------------------------------------------------------------------------
def test_dedup_kept_reads(pkg, synth):
    """the layout of the host program: the read-1 file as one kept batch (ordinals base, base + 2, ...), the read-2 file as another
    (base + 1, base + 3, ...), a batch of single reads behind them; no read has ordinals 0 .. 2.  The read-2 file is one read short"""
    rng = np.random.default_rng(77)
    seq = lambda L: rng.integers(0, 4, size=L, dtype=np.uint8)
    P, base = 12, 3
    r1 = [seq(int(rng.integers(40, 120))) for _ in range(P + 1)]
    r2 = [seq(int(rng.integers(40, 120))) for _ in range(P)]
    for t in (5, 9):                                      # copies of pair 0, spread over the range
        r1[t], r2[t] = r1[0], r2[0]
    r1[3], r2[3] = r2[0], r1[0]                           # pair 0 read from the other strand
    r1[7], r2[7] = r1[6], r2[6]
    singles = [seq(int(rng.integers(40, 120))) for _ in range(9)]
    singles[1] = r1[2]                                    # equals mate 1 of a pair: a single read never equals a pair
    singles[4] = r1[P]                                    # equals the pair of which only the first mate is kept
    singles[6] = singles[0]
    singles[8] = r2[P - 1][:-1]                           # a proper prefix of a mate
    first, end = base, base + 2 * (P + 1)
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)] + [end + i for i in range(len(singles))]
    codes, offs = rd.concat(r1 + r2 + singles)
    total = end + len(singles)
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for batch, b, stride in ((r1, base, 2), (r2, base + 1, 2), (singles, end, 1)):
            g.set_read_ordinal(b, stride)
            bc, bo = rd.concat(batch)
            g.push_reads(synth.pack_2bit(bc), bo)
        g.finish_count()
        for flags in (0, rd.MATE_SWAP):
            wdup, wkeep, wkept = rd.expect_dedup(codes, offs, flags=flags, ordinals=ords, units=ranged_units(ords, [(first, end)]))
            out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_DUP_DTYPE)
            dup, n, kept = g.dedup_kept_reads(total, [(first, end)], flags=flags, out=out)
            assert n == len(ords) and kept == wkept
            absent = np.ones(total, dtype=bool)
            absent[ords] = False
            assert absent.sum() == 4 and (np.ascontiguousarray(dup[absent]).view(np.uint32) == 0xABABABAB).all()
            rd.assert_dup_equal(dup[~absent], wdup[~absent], f"kept reads, flags={flags}")
            # what the case is about
            assert wdup["verdict"][end + 1] == rd.KEPT and wdup["copies"][end + 1] == 1
            assert wdup[end + 4].tolist() == (base + 2 * P, 2, rd.DROPPED) and wdup[base + 2 * P].tolist() == (base + 2 * P, 2, rd.KEPT)
            assert wdup["copies"][base] == (4 if flags else 3) and wdup["verdict"][base + 6] == (rd.DROPPED if flags else rd.KEPT)
            assert wdup["verdict"][end + 8] == rd.KEPT
        # no ranges: every read on its own
        wdup = rd.expect_dedup(codes, offs, ordinals=ords)[0]
        dup, n, kept = g.dedup_kept_reads(total)
        rd.assert_dup_equal(dup[~absent], wdup[~absent], "kept reads, no pair ranges")
        # the same range in two halves that touch
        wdup = rd.expect_dedup(codes, offs, ordinals=ords, units=ranged_units(ords, [(first, end)]))[0]
        dup, n, kept = g.dedup_kept_reads(total, [(first, first + 8), (first + 8, end)])
        rd.assert_dup_equal(dup[~absent], wdup[~absent], "kept reads, two ranges")
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_DUP_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.dedup_kept_reads(total - 1, [(first, end)], out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        # ranges that overlap, run backwards or hold half a pair: refused before anything is written
        full = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_DUP_DTYPE)
        for bad in ([(first, end), (end - 2, end + 2)], [(first, first + 3)], [(end, first)], [(first + 8, end), (first, first + 8)]):
            with pytest.raises(pkg.SdtError) as e:
                g.dedup_kept_reads(total, bad, out=full)
            assert e.value.code == pkg.SDT_EINVAL and "range" in str(e.value)
            assert (full.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.dedup_kept_reads(total, [(first, end)], flags=4)
        assert e.value.code == pkg.SDT_EINVAL
        # the kept reads are as they were
        bc, bo = rd.concat(r2)
        w, o, b, stride = g.fetch_kept_batch(1)
        assert (b, stride) == (base + 1, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        with pytest.raises(pkg.SdtError) as e:
            g.dedup_kept_reads(total, [(first, end)])
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)


# ---- 6. no table ------------------------------------------------------------------------------------------------------------------
def test_dedup_needs_no_table(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    c = rd.case()
    words = synth.pack_2bit(c["codes"])
    n = len(c["offs"]) - 1
    want = rd.expect_dedup(c["codes"], c["offs"])
    _, codes, offs = workload(synth, K, 100, n_reads=500)
    batch = synth.pack_2bit(codes)

    def snapshot(g):
        keys, l, rf, cnt = g.export_nodes()[:4]
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt)]

    def device_form(g):
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(c["offs"].view(np.int64)).to(dev)
        d_dup = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kept = g.dedup_reads_device(d_w, d_o, n, d_dup, d_keep)
        return d_dup.cpu().numpy().view(np.uint8).copy().view(pkg.READ_DUP_DTYPE).reshape(-1), d_keep.cpu().numpy(), kept

    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g, pkg.PregraphGPU(K, est_distinct=1 << 16) as fresh:
        assert_dedup(pkg, g.dedup_reads(words, c["offs"]), want, "a fresh context, host form")
        assert_dedup(pkg, device_form(g), want, "a fresh context, device form")
        # the context then counts like one that never ran it -- and dedup runs between a push and its drain too
        g.push_reads(batch, offs)
        assert_dedup(pkg, g.dedup_reads(words, c["offs"]), want, "pushed, not drained")
        fresh.push_reads(batch, offs)
        assert g.finish_count() == fresh.finish_count()
        for x, y in zip(snapshot(g), snapshot(fresh)):
            assert x.shape == y.shape and (x == y).all()
        hist, linear = g.mark_and_hist()
        fhist, flinear = fresh.mark_and_hist()
        assert linear == flinear and (hist == fhist).all()
        assert_dedup(pkg, g.dedup_reads(words, c["offs"]), want, "a counted context")
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        assert_dedup(pkg, g.dedup_reads(words, c["offs"]), want, "a contig index, host form")
        assert_dedup(pkg, device_form(g), want, "a contig index, device form")
