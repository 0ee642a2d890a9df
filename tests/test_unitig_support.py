"""GPU (-m gpu): the read support tally on the unitig list (sdt_gpu_unitigs_support_*) against the Python restatement of the rule
(unitig_support_util.py): per unitig, per link, junctions, mate links and totals, all exact.  The nodes of the model come from the oracle
or are written by hand, and its segments are its own, never the library's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_support_util as su
import unitig_thread_util as tu
from test_unitigs import counted_case, imported, raises

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = dict(junction_capacity=4096, mate_capacity=4096)


def prm(min_count, min_link=1, max_count=0):
    return dict(min_count=min_count, max_count=max_count, min_link=min_link)


def begun(g, params, room=ROOM):
    g.unitigs_begin(params)
    g.unitigs_index()
    g.unitigs_support_begin(room)


def add_host(g, synth, reads, paired=False):
    codes, offs = cu.concat(list(reads))
    g.unitigs_support_add(synth.pack_2bit(codes), offs, paired)


def add_device(g, synth, reads, paired=False):
    import torch
    codes, offs = cu.concat(list(reads))
    d_w = torch.from_numpy(synth.pack_2bit(codes).view(np.int32)).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    g.unitigs_support_add_device(d_w, d_o, len(offs) - 1, paired)
    torch.cuda.synchronize()


# ---- 1. the built cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [23, 33, 65, 97])
def test_bubble_case_equals_the_model(pkg, synth, K):
    """the device form without pairs, the host form with them; min_count 2 and 1"""
    case = bu.built_case(K)
    with counted_case(pkg, synth, case) as g:
        for mc in (2, 1):
            begun(g, prm(mc))
            add_device(g, synth, case["counted"])
            want = su.bubble_support(K, mc, 1)
            su.assert_support_equal(g, want, f"K={K} min_count={mc}, device form")
            assert want.t["traversals"] > 250 and want.t["passages"] > 10 and len(want.junctions) >= 4
            g.unitigs_support_begin(ROOM)                       # (a second begin replaces the first: the tally starts again)
            add_host(g, synth, su.even(case["counted"]), True)
            want = su.bubble_pairs_support(K, mc, 1)
            su.assert_support_equal(g, want, f"K={K} min_count={mc}, host form, pairs")
            assert len(want.mates) > 10 and want.t["pairs_within"] > 500


@pytest.mark.parametrize("K", [23, 33, 65, 97])
def test_cluster_case_equals_the_model(pkg, synth, K):
    """short, empty and unplaced reads and mates; polyA makes every lane a traversal of one link and a passage (u, u, u); under link_cut
    the junction is an unlinked step: no traversal"""
    case = cu.built_case(K)
    with counted_case(pkg, synth, case) as g:
        for name, p in cu.PARAM_SETS.items():
            begun(g, p)
            add_host(g, synth, case["query"], True)
            su.assert_support_equal(g, su.cluster_support(K, name, True), f"K={K} {name}, host form")
            g.unitigs_support_begin(ROOM)
            add_device(g, synth, case["query"], True)
            su.assert_support_equal(g, su.cluster_support(K, name, True), f"K={K} {name}, device form")
        base = su.cluster_support(K, "base", True)
        assert base.t["passages"] > 50 and max(base.junctions.values()) > 50 and base.t["placed"] < base.t["reads"] and base.t["pairs_placed"] < base.t["pairs"]


# ---- 2. the boundaries of a step, a cycle, pairs --------------------------------------------------------------------------------------------------
def test_step_boundaries(pkg, synth):
    """links at lanes 63 and 0 of consecutive steps: the passage's earlier start lies in the step before; and two steps before, behind a
    unitig of 70 nodes; each read alone, on both strands, and all together"""
    case = su.boundary_case()
    th = case["th"]
    with imported(pkg, case["nodes"], case["K"]) as g:
        begun(g, prm(1))
        for name, read in case["reads"].items():
            g.unitigs_support_begin(ROOM)
            add_host(g, synth, [read])
            want = su.Support(th).add([read])
            assert want.t["passages"] == {"two": 1, "thr": 3, "lon": 2}[name[:3]]
            su.assert_support_equal(g, want, name)
        g.unitigs_support_begin(ROOM)
        add_device(g, synth, case["reads"].values())
        want = su.Support(th).add(list(case["reads"].values()))
        assert sorted(want.junctions.values()) == [2, 2, 2, 2, 4]      # (a read and its reverse complement: the same junctions; two reads share one)
        su.assert_support_equal(g, want, "all the reads")


def test_round_a_cycle(pkg, synth):
    """the closing link of a circular unitig is a link like any other, and its own mirror's mirror; the passage (u, u, u)"""
    case = su.cycle_case()
    with imported(pkg, case["nodes"], case["K"]) as g:
        begun(g, prm(1))
        add_host(g, synth, case["reads"])
        su.assert_support_equal(g, su.Support(case["th"]).add(case["reads"]), "a cycle of 40")
        assert g.unitigs_support_junctions().tolist() == [(0, 0, 0, 0, 4)]


def test_pairs(pkg, synth):
    """both orientations of both mates, one mate unplaced or too short, both mates in one unitig, a pair that turns round in one unitig:
    each pair alone, and all of them in one batch"""
    case = su.boundary_case()
    th = case["th"]
    with imported(pkg, case["nodes"], case["K"]) as g:
        begun(g, prm(1))
        for name, pair in case["pairs"].items():
            g.unitigs_support_begin(ROOM)
            add_device(g, synth, pair, True)
            su.assert_support_equal(g, su.Support(th).add(list(pair), True), name)
        every = [r for pair in case["pairs"].values() for r in pair]
        g.unitigs_support_begin(ROOM)
        add_host(g, synth, every, True)
        want = su.Support(th).add(every, True)
        assert want.t["pairs_within"] == 2 and want.t["pairs_placed"] == 7 and sorted(want.mates.values()) == [1, 1, 1, 2]
        su.assert_support_equal(g, want, "all the pairs")


# ---- 3. the split over calls, the order, pieces, one workgroup ----------------------------------------------------------------------------------------
def everything(g):
    n = int(g.unitigs_index()[1])
    return dict(unitigs=g.unitigs_support_unitigs(0, n).view(np.uint64), links=g.unitigs_support_links(0, n).view(np.uint64),
                junctions=g.unitigs_support_junctions().view(np.uint64), mates=g.unitigs_support_mates().view(np.uint64), totals=g.unitigs_support_totals())


def test_split_and_order(pkg, synth):
    """one batch against the same pairs added in three calls, and in the reverse order of the pairs"""
    K = 33
    case = bu.built_case(K)
    reads = su.even(case["counted"])
    want = su.bubble_pairs_support(K, 2, 1)
    pairs = list(zip(reads[0::2], reads[1::2]))
    backwards = [r for pair in reversed(pairs) for r in pair]
    with counted_case(pkg, synth, case) as g:
        begun(g, prm(2))
        add_host(g, synth, reads, True)
        once = everything(g)
        g.unitigs_support_begin(ROOM)
        for part in (reads[:600], reads[600:602], reads[602:]):
            add_host(g, synth, part, True)
        su.assert_support_equal(g, want, "three calls")
        g.unitigs_support_begin(ROOM)
        add_device(g, synth, backwards, True)
        there = everything(g)
        su.assert_support_equal(g, want, "the pairs in reverse order")
        for name, a in once.items():
            assert (a == there[name]).all(), name


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
from test_unitig_support import whole_run
np.savez({path!r}, **whole_run(pkg, synth))
"""


def whole_run(pkg, synth):
    """the pairs of the bubble case at K = 31 through the host form and the device form -> arrays by name"""
    K = 31
    case = bu.built_case(K)
    reads = su.even(case["counted"])
    with counted_case(pkg, synth, case) as g:
        begun(g, prm(2))
        add_host(g, synth, reads, True)
        out = {"host_" + k: v for k, v in everything(g).items()}
        g.unitigs_support_begin(ROOM)
        add_device(g, synth, reads, True)
        out.update({"device_" + k: v for k, v in everything(g).items()})
        return out


def test_geometry_and_pieces(pkg, synth, tmp_path):
    """one workgroup and pieces of 5 reads -- an odd number, so the cut would fall inside a pair if pieces did not hold whole pairs -- (test
    hooks, so in a child process) give what the default run gives; the device form gives what the host form gives; both are the model's"""
    here = whole_run(pkg, synth)
    want = su.bubble_pairs_support(31, 2, 1)
    for form in ("host_", "device_"):
        assert here[form + "unitigs"].tolist() == want.unitigs().view(np.uint64).tolist() and here[form + "links"].tolist() == want.links().view(np.uint64).tolist()
        assert here[form + "junctions"].tolist() == want.junction_list().view(np.uint64).tolist() and here[form + "mates"].tolist() == want.mate_list().view(np.uint64).tolist()
        assert here[form + "totals"].tolist() == want.totals().tolist()
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_WAVE_BLOCKS="1", SDT_SCAN_BLOCKS="1", SDT_SEARCH_CHUNK="5")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    there = np.load(path)
    for name, a in here.items():
        assert a.dtype == there[name].dtype and a.shape == there[name].shape and (a == there[name]).all(), name


# ---- 4. a set that fills up ----------------------------------------------------------------------------------------------------------------------
def test_full_sets(pkg, synth):
    """capacities one below the model's distinct junctions and mate links: the add says SDT_EFULL, entries are dropped, the fetch of that
    set says SDT_EFULL, and the tallies per unitig and per link are the model's; with exactly the room nothing is dropped"""
    K = 23
    case = bu.built_case(K)
    reads = su.even(case["counted"])
    want = su.bubble_pairs_support(K, 2, 1)
    nj, nm = len(want.junctions), len(want.mates)
    assert nj > 2 and nm > 2
    with counted_case(pkg, synth, case) as g:
        begun(g, prm(2), dict(junction_capacity=nj, mate_capacity=nm))
        add_host(g, synth, reads, True)
        su.assert_support_equal(g, want, "exactly the room that is needed")
        for room, full in ((dict(junction_capacity=nj - 1, mate_capacity=nm), "j"), (dict(junction_capacity=nj, mate_capacity=nm - 1), "m"),
                           (dict(junction_capacity=nj - 1, mate_capacity=nm - 1), "jm")):
            g.unitigs_support_begin(room)
            raises(pkg, pkg.SDT_EFULL, lambda: add_host(g, synth, reads, True), "is full")
            totals = g.unitigs_support_totals()
            assert int(totals[11]) > 0 and totals[:11].tolist() == want.totals()[:11].tolist()
            if "j" in full:
                raises(pkg, pkg.SDT_EFULL, g.unitigs_support_junctions, "filled up")
            if "m" in full:
                raises(pkg, pkg.SDT_EFULL, g.unitigs_support_mates, "filled up")
            su.assert_support_equal(g, want, f"full: {full}", junctions="j" not in full, mates="m" not in full, totals=False)
            raises(pkg, pkg.SDT_EFULL, lambda: add_device(g, synth, reads[:2], True), "is full")      # (and so says every add after it)
        # a list that is not kept; the room that a fetch is offered
        g.unitigs_support_begin(dict(junction_capacity=0, mate_capacity=nm))
        add_host(g, synth, reads, True)
        raises(pkg, pkg.SDT_EINVAL, g.unitigs_support_junctions, "not kept")
        su.assert_support_equal(g, want, "no junction set", junctions=False)
        with pytest.raises(pkg.SdtError) as e:
            g.unitigs_support_mates(capacity=nm - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.n == nm and "room for" in str(e.value)
        n = len(want.segs)
        with pytest.raises(pkg.SdtError) as e:
            g.unitigs_support_links(0, n, capacity=len(want.m.links) - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.n_links == len(want.m.links)


def test_a_set_overshot_many_times(pkg, synth):
    """every unitig of the bubble case paired with every other, in all orientations: thousands of distinct mate links for a set of
    capacity 1 and 64 slots.  Once the set is full nothing more is looked up, so the add ends at once; it says SDT_EFULL, the drops
    are at least the links that no slot could hold, the junction set beside it keeps its list, and the other tallies are the model's"""
    K = 23
    case = bu.built_case(K)
    th = tu.bubble_threading(K, 2, 1)
    seqs = [np.array(th.m.codes(i)[:K + 40], dtype=np.uint8) for i in range(len(th.m.unitigs))]      # (the head of every unitig: one segment)
    seqs += [cu.revcomp(x) for x in seqs]
    reads = [r for a in seqs for b in seqs for r in (a, b)]
    want = su.Support(th).add(reads, True)
    assert len(want.mates) > 20 * 64 and want.t["pairs_placed"] == want.t["pairs"] == len(seqs) ** 2
    with counted_case(pkg, synth, case) as g:
        begun(g, prm(2), dict(junction_capacity=4096, mate_capacity=1))
        raises(pkg, pkg.SDT_EFULL, lambda: add_host(g, synth, reads, True), "mate-link set is full")
        totals = g.unitigs_support_totals()
        assert int(totals[11]) >= len(want.mates) - 64 and totals[:11].tolist() == want.totals()[:11].tolist()
        raises(pkg, pkg.SDT_EFULL, g.unitigs_support_mates, "filled up")
        su.assert_support_equal(g, want, "a mate-link set overshot many times", mates=False, totals=False)


# ---- 5. state and arguments -------------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(pkg, synth):
    K = 31
    case = bu.built_case(K)
    reads = su.even(case["counted"])
    codes, offs = cu.concat(reads)
    words = synth.pack_2bit(codes)
    want = su.bubble_pairs_support(K, 2, 1)
    n = len(want.segs)
    no_list, changed, no_index, no_begin = "sdt_gpu_unitigs_begin first", "the table changed since sdt_gpu_unitigs_begin", "no sdt_gpu_unitigs_index", "no sdt_gpu_unitigs_support_begin"
    calls = lambda g: (lambda: g.unitigs_support_add(words, offs, True), lambda: g.unitigs_support_unitigs(0, 1), lambda: g.unitigs_support_links(0, 1),
                       g.unitigs_support_junctions, g.unitigs_support_mates, g.unitigs_support_totals)
    with counted_case(pkg, synth, case) as g:
        g.unitigs_support_end()                                 # (without a begin: SDT_OK)
        for call in calls(g) + (lambda: g.unitigs_support_begin(ROOM),):
            raises(pkg, pkg.SDT_ESTATE, call, no_list)
        g.unitigs_begin(prm(2))
        for call in calls(g) + (lambda: g.unitigs_support_begin(ROOM),):
            raises(pkg, pkg.SDT_ESTATE, call, no_index)
        g.unitigs_index()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_begin)
        # a clustering, a bubble list and an assembly tally begun before stay usable
        cinfo = g.cluster_begin()
        ckeys = g.cluster_components()[0].tolist()
        binfo = g.bubbles_begin(bu.DEFAULTS)
        g.asm_begin()
        g.asm_add(words, offs, records=False)
        asm = [a.tolist() for a in g.asm_spectrum()]
        g.unitigs_support_begin(ROOM)
        # refused before any launch, with nothing added
        launches = g.kernel_time(reset=False)[1]
        lib, ctx = g.lib, g._ctx
        assert lib.sdt_gpu_unitigs_support_add(ctx, pkg._ptr(words), words.size, pkg._ptr(offs), len(reads) - 1, 1) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_add_device(ctx, 8, 8, 3, 1) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_add(ctx, None, words.size, pkg._ptr(offs), len(reads), 1) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_add(ctx, pkg._ptr(words), words.size, None, len(reads), 1) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_add_device(ctx, None, 8, 2, 1) == pkg.SDT_EINVAL
        bad = offs.copy()
        bad[3] = bad[5]
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_support_add(words, bad, True), "not monotonic")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_support_add(words[:10], offs, True), "too short")
        nn = ctypes.c_uint64(0)
        assert lib.sdt_gpu_unitigs_support_unitigs(ctx, 0, 1, None) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_links(ctx, 0, 1, None, 0, None) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_junctions(ctx, None, 0, None) == pkg.SDT_EINVAL and lib.sdt_gpu_unitigs_support_mates(ctx, None, 3, ctypes.byref(nn)) == pkg.SDT_EINVAL
        assert lib.sdt_gpu_unitigs_support_totals(ctx, None) == pkg.SDT_EINVAL
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_support_unitigs(n, 1), "unitigs")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_support_links(0, n + 1), "unitigs")
        assert g.kernel_time(reset=False)[1] == launches
        assert g.unitigs_support_totals().tolist() == [0] * 12 and len(g.unitigs_support_junctions()) == 0 and not g.unitigs_support_unitigs(0, n).view(np.uint64).any()
        # nothing to do: SDT_OK, nothing touched
        assert lib.sdt_gpu_unitigs_support_add(ctx, None, 0, None, 0, 1) == pkg.SDT_OK and lib.sdt_gpu_unitigs_support_add_device(ctx, None, None, 0, 0) == pkg.SDT_OK
        assert lib.sdt_gpu_unitigs_support_unitigs(ctx, 0, 0, None) == pkg.SDT_OK and lib.sdt_gpu_unitigs_support_links(ctx, 0, 0, None, 0, None) == pkg.SDT_OK
        # flags, reserved, NULL: the tally that is there stays
        for room in (dict(flags=1), dict(reserved=1), dict(junction_capacity=1 << 40)):
            raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_support_begin(room), "sdt_support_params")
        assert lib.sdt_gpu_unitigs_support_begin(ctx, None) == pkg.SDT_EINVAL
        g.unitigs_support_add(words, offs, True)
        su.assert_support_equal(g, want, "after the refusals")
        # a second index leaves the tally valid; the adds go on adding
        g.unitigs_index()
        su.assert_support_equal(g, want, "across a second unitigs_index")
        g.unitigs_support_add(words, offs, True)
        twice = su.Support(want.th).add(reads, True).add(reads, True)
        su.assert_support_equal(g, twice, "added twice")
        # the clustering, the bubble list and the assembly tally are what they were
        assert g.cluster_components()[0].tolist() == ckeys and int(g.cluster_begin()[2]) == int(cinfo[2])
        bu.assert_bubbles_equal(g, case["model"], binfo, "the bubble list across the support calls")
        assert [a.tolist() for a in g.asm_spectrum()] == asm
        su.assert_support_equal(g, twice, "across a cluster_begin")
        # end; a second unitigs_begin; unitigs_end
        g.unitigs_support_end()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_begin)
        g.unitigs_support_begin(ROOM)
        g.unitigs_begin(prm(2))
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_index)
        g.unitigs_index()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_begin)
        g.unitigs_support_begin(ROOM)
        g.unitigs_end()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_list)
        # the table changes under a tally
        begun(g, prm(2))
        g.unitigs_support_add(words, offs, True)
        g.delow(1)
        for call in calls(g) + (lambda: g.unitigs_support_begin(ROOM),):
            raises(pkg, pkg.SDT_ESTATE, call, changed)
        begun(g, prm(2))                                        # (a context destroyed with a tally frees it)
