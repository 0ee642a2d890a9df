"""GPU (-m gpu): an assembly scored against the counted table (sdt_gpu_asm_*) against the Python restatement of the rule
(asm_support_util.py): records, totals and the copy-number spectrum, all exact.  Counts come from the oracle, never from the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import asm_support_util as au

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counted(pkg, synth, case, flags=0):
    """a context with the case's reads counted; the table is the oracle's"""
    g = pkg.PregraphGPU(case["K"], est_distinct=1 << 16, flags=flags)
    g.push_reads(synth.pack_2bit(case["reads"][0]), case["reads"][1])
    assert g.finish_count() == (case["kmers_in_reads"], case["nodes"])
    return g


def add_all(g, synth, seqs, records=True):
    codes, offs = au.concat(seqs)
    return g.asm_add(synth.pack_2bit(codes), offs, records=records)


def check(pkg, synth, g, case, min_count, rows, what):
    want, cn = au.support(case["seqs"], case["K"], case["counts"], min_count)
    g.asm_begin(dict(min_count=min_count, rows=rows))
    au.assert_records_equal(add_all(g, synth, case["seqs"]), want, what)
    m, tot = g.asm_spectrum()
    assert m.shape == (rows, pkg.ASM_CN_COLS) and (m == au.spectrum(case["counts"], cn, rows)).all(), what
    assert (tot == au.totals(want)).all(), (what, tot, au.totals(want))
    return want, m, tot


# ---- 1. records, totals and matrix equal the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(23, 0), (24, 0), (31, 1), (31, 2), (47, 0), (63, 0), (95, 0), (127, 0), (33, 0), (65, 0), (97, 0)])
def test_records_totals_and_matrix_equal_the_model(pkg, synth, K, flags):
    """1, 2 and 4 key words, both pass-1 kernel families at K = 31 (SDT_FLAG_DIRECT, SDT_FLAG_PARTITION).  K = 24: the library takes odd
    K only (sdt_gpu_init refuses an even one before any table exists), so the one thing an even K adds to the rule -- a palindrome is
    its own reverse complement and counts once per occurrence -- cannot be reached through the ABI; what is asserted here is that
    refusal, and the palindrome itself is held against the restatement on the CPU (test_asm_support_host.py)."""
    if K % 2 == 0:
        with pytest.raises(pkg.SdtError) as e:
            pkg.PregraphGPU(K, est_distinct=1 << 16)
        assert e.value.code == pkg.SDT_EINVAL and "odd" in str(e.value)
        return
    case = au.reduced_case(synth, K)
    with counted(pkg, synth, case, flags) as g:
        assert g.nw == (1 if K <= 31 else 2 if K <= 63 else 4)
        want, m, tot = check(pkg, synth, g, case, 2, 64, f"K={K} flags={flags}")
        assert max(case["counts"].values()) > 65535 and m[63].sum() >= 1 and m[:, 7].sum() >= 1 and m[:, 2].sum() >= 1
        assert (want["gaps"] > 0).sum() >= 4 and tot[3] < tot[2] < tot[1]
        g.asm_end()


# ---- 2. the named case, the high halves of the counts through aux and through the hash -------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import asm_support_util as au
from test_asm_support import counted, add_all
case = au.named_case(synth)
with counted(pkg, synth, case) as g:
    g.asm_begin(dict(min_count=au.NAMED_MIN_COUNT, rows=au.NAMED_ROWS))
    rec = add_all(g, synth, case["seqs"])
    m, tot = g.asm_spectrum()
np.savez({path!r}, rec=rec, m=m, tot=tot)
"""


@pytest.mark.parametrize("aux_form,wave_blocks", [("aux", "2"), ("hash", "")])
def test_named_case(pkg, synth, tmp_path, aux_form, wave_blocks):
    """every property that test_asm_support_host.py asserts on the model: all 16 phases, columns 0 .. 7, a byte driven to 255 by 64
    lanes at once, the cap row, a count past 65 535, gaps across, up to and from a step's boundary, a gap of 200 carried over four
    steps, a sequence of 20 000 bases.  With two workgroups (test hook) a wavefront takes sequence after sequence."""
    case = au.named_case(synth)
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_PROFILE_AUX=aux_form)
    if wave_blocks:
        env["SDT_WAVE_BLOCKS"] = wave_blocks
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    au.assert_records_equal(got["rec"], case["want"], f"the named case, {aux_form}")
    assert (got["m"] == case["matrix"]).all() and (got["tot"] == au.totals(case["want"])).all()


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------------
def test_invariance(pkg, synth, monkeypatch):
    """one add; the same sequences over three adds; reversed order; the device form; pieces of 7 sequences: the same matrix and totals,
    the same record per sequence"""
    import torch
    case = au.named_case(synth)
    seqs, want = case["seqs"], case["want"]
    n = len(seqs)
    with counted(pkg, synth, case) as g:
        prm = dict(min_count=au.NAMED_MIN_COUNT, rows=au.NAMED_ROWS)

        def finish(rec, what):
            au.assert_records_equal(rec, want, what)
            m, tot = g.asm_spectrum()
            assert (m == case["matrix"]).all() and (tot == au.totals(want)).all(), what

        g.asm_begin(prm)
        finish(add_all(g, synth, seqs), "one add")
        g.asm_begin(prm)
        a, b = n // 3, 2 * n // 3
        parts = [add_all(g, synth, seqs[:a])]
        m1, tot1 = g.asm_spectrum()                                            # (between adds: the tally so far)
        assert tot1[0] == a and 0 < m1[:, 1:].sum() < case["matrix"][:, 1:].sum()
        parts += [add_all(g, synth, seqs[a:b]), add_all(g, synth, seqs[b:])]
        finish(np.concatenate(parts), "three adds")
        g.asm_begin(prm)
        finish(add_all(g, synth, seqs[::-1])[::-1], "reversed order")
        g.asm_begin(prm)
        codes, offs = au.concat(seqs)
        d_w = torch.from_numpy(synth.pack_2bit(codes).view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        d_out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        g.asm_add_device(d_w, d_o, n, d_out)
        torch.cuda.synchronize()
        finish(d_out.cpu().numpy().view(au.DTYPE).reshape(n), "the device form")
        monkeypatch.setenv("SDT_SEARCH_CHUNK", "7")
        g.asm_begin(prm)
        finish(add_all(g, synth, seqs), "pieces of 7 sequences")


# ---- 4. parameters ---------------------------------------------------------------------------------------------------------------------
def test_min_count_rows_and_no_records(pkg, synth):
    case = au.reduced_case(synth, 31)
    top = max(case["counts"].values())
    with counted(pkg, synth, case) as g:
        w0 = check(pkg, synth, g, case, 0, 2, "min_count 0, rows 2")[0]
        w1 = check(pkg, synth, g, case, 1, 1024, "min_count 1, rows 1024")[0]
        assert (w0 == w1).all() and (w0["solid"] == w0["found"]).all()         # an absent k-mer is weak whatever min_count says
        w2 = check(pkg, synth, g, case, 2, 1024, "min_count 2, rows 1024")[0]
        assert (w2["solid"] < w2["found"]).any()
        wt = check(pkg, synth, g, case, top + 1, 64, "min_count above the largest count")[0]
        assert (wt["solid"] == 0).all() and (wt["gaps"] == (wt["kmers"] > 0)).all() and (wt["longest_gap"] == wt["kmers"]).all()
        # out = NULL: the tally alone
        want, cn = au.support(case["seqs"], 31, case["counts"], 2)
        g.asm_begin(dict(min_count=2, rows=64))
        assert add_all(g, synth, case["seqs"], records=False) is None
        m, tot = g.asm_spectrum()
        assert (m == au.spectrum(case["counts"], cn, 64)).all() and (tot == au.totals(want)).all()
        # no sequence: nothing touched
        g.asm_add(np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
        assert (g.asm_spectrum()[1] == tot).all()


# ---- 5. the table is untouched -----------------------------------------------------------------------------------------------------------
def test_the_table_is_untouched(pkg, synth):
    case = au.reduced_case(synth, 31)

    def snapshot(g):
        keys, l, rf, cnt = g.export_nodes()[:4]
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt)]

    with counted(pkg, synth, case) as g:
        before = snapshot(g)
        ans0 = g.search_kmers(before[0])
        check(pkg, synth, g, case, 2, 64, "between two snapshots")
        after = snapshot(g)
        for a, b in zip(before, after):
            assert a.shape == b.shape and (a == b).all()
        for a, b in zip(ans0, g.search_kmers(before[0])):
            assert (a == b).all()
        # ... and the tally survives what only reads the table
        m, tot = g.asm_spectrum()
        assert tot[0] == len(case["seqs"]) and m[:, 1:].sum() > 0


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------
def raises(pkg, code, call, *words):
    with pytest.raises(pkg.SdtError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_state_and_arguments(pkg, synth):
    case = au.reduced_case(synth, 31)
    K, seqs = 31, case["seqs"][:6]
    rcodes, roffs = case["reads"]
    words = synth.pack_2bit(rcodes)
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        # before finish_count: batches pushed and not drained
        g.push_reads(words, roffs)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_begin(), "sdt_gpu_asm_begin", "sdt_gpu_finish_count")
        g.finish_count()
        # without a begin
        raises(pkg, pkg.SDT_ESTATE, lambda: add_all(g, synth, seqs), "sdt_gpu_asm_begin first")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_spectrum(), "sdt_gpu_asm_begin first")
        g.asm_end()                                                            # (nothing to free: fine)
        # the parameters
        for rows in (0, 1, 1025):
            raises(pkg, pkg.SDT_EINVAL, lambda: g.asm_begin(dict(rows=rows)), "rows", str(rows))
        raises(pkg, pkg.SDT_EINVAL, lambda: g.asm_begin(dict(flags=1)), "flags")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.asm_begin(dict(reserved=7)), "reserved")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_spectrum(), "sdt_gpu_asm_begin first")             # (a refused begin begins nothing)
        g.asm_begin(dict(min_count=2, rows=64))
        want, cn = au.support(seqs, K, case["counts"], 2)
        au.assert_records_equal(add_all(g, synth, seqs), want, "first add")
        # offsets that descend, words that are too few: refused, nothing tallied
        codes, offs = au.concat(seqs)
        bad = offs.copy()
        bad[2] = bad[1] - 1
        raises(pkg, pkg.SDT_EINVAL, lambda: g.asm_add(synth.pack_2bit(codes), bad), "monotonic")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.asm_add(synth.pack_2bit(codes)[:-5], offs), "too short")
        assert (g.asm_spectrum()[1] == au.totals(want)).all()
        # begin again zeroes the tally
        g.asm_begin(dict(min_count=2, rows=64))
        m, tot = g.asm_spectrum()
        assert (tot == 0).all() and m[:, 1:].sum() == 0 and m.sum() == case["nodes"]
        add_all(g, synth, seqs)
        assert (g.asm_spectrum()[0] == au.spectrum(case["counts"], cn, 64)).all()
        # the table changes: a push and finish_count after begin
        g.push_reads(words, roffs[:41])
        g.finish_count()
        raises(pkg, pkg.SDT_ESTATE, lambda: add_all(g, synth, seqs), "the table changed since sdt_gpu_asm_begin")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_spectrum(), "the table changed since sdt_gpu_asm_begin")
        g.asm_begin(dict(min_count=2, rows=64))                                # a new begin is on the new table
        assert add_all(g, synth, seqs)["kmers"].tolist() == want["kmers"].tolist()
        # end, then add
        g.asm_end()
        raises(pkg, pkg.SDT_ESTATE, lambda: add_all(g, synth, seqs), "sdt_gpu_asm_begin first")
        # path words in place of the counters
        g.load_paths(None, None, None, None, 0)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_begin(), "sdt_gpu_asm_begin", "path words")
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        raises(pkg, pkg.SDT_ESTATE, lambda: g.asm_begin(), "sdt_gpu_asm_begin", "SDT_FLAG_CONTIG_INDEX")
    # a context destroyed with a tally open frees it
    with counted(pkg, synth, case) as g:
        g.asm_begin()
        add_all(g, synth, seqs)
