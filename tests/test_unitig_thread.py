"""GPU (-m gpu): reads threaded through the unitig list (sdt_gpu_unitigs_index / _lookup / _reads / _reads_device) against the Python
restatement of the rule (unitig_thread_util.py): labels, read records, segment offsets and segments, all exact.  The nodes of the model
come from the oracle or are written by hand, never from the library."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_thread_util as tu
import unitig_util as uu
from test_unitigs import counted_case, imported, raises

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prm(min_count, min_link=1, max_count=0):
    return dict(min_count=min_count, max_count=max_count, min_link=min_link)


def thread_reads(g, synth, reads, **kw):
    codes, offs = cu.concat(reads)
    return g.unitigs_reads(synth.pack_2bit(codes), offs, **kw)


def indexed(g, params, model):
    """begin and index; info against the model"""
    binfo = g.unitigs_begin(params)
    assert [int(x) for x in binfo] == model.info
    info = g.unitigs_index()
    assert info.tolist() == [model.info[0], model.info[2], 8 * g.table_slots(), 0]
    return info


# ---- 1. the bubble cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [23, 31, 33, 65, 97])
@pytest.mark.parametrize("mc,ml", [(1, 1), (2, 1)])
def test_bubble_case_equals_the_model(pkg, synth, K, mc, ml):
    case = bu.built_case(K)
    th = tu.bubble_threading(K, mc, ml)
    want = tu.bubble_records(K, mc, ml)
    rng = np.random.default_rng(K)
    with counted_case(pkg, synth, case) as g:
        indexed(g, prm(mc, ml), th.m)
        # every node of the table, live or not, on both strands, and k-mers that the table does not hold
        words = sorted(case["nodes"])
        words += [cu.rc_int(w, K) for w in words]
        absent = [int.from_bytes(rng.bytes(32), "little") & ((1 << (2 * K)) - 1) for _ in range(100)]
        assert not any(cu.canon(w, K) in case["nodes"] for w in absent)
        got = g.unitigs_lookup(cu.keys_array(words + absent, g.nw))
        wl = th.lookup(words + absent)
        assert got.dtype == tu.POS_DTYPE
        for f in tu.POS_FIELDS:
            assert (got[f] == wl[f]).all(), f
        assert int((wl["unitig"] != tu.NONE).sum()) == 2 * th.m.info[0] and (wl["unitig"][-100:] == tu.NONE).all()
        # the counted reads
        rec, offs, segs = thread_reads(g, synth, case["counted"])
        tu.assert_threading_equal((rec, offs, segs), want, f"K={K} min_count={mc} min_link={ml}")
        # the device alone: links, sums, and the reads rebuilt from the sequences along their paths
        n = int(th.m.info[2])
        links, _ = g.unitigs_links(0, n)
        link_set = {(int(l["from"]), int(l["info"]) & 1, int(l["to"]), int(l["info"]) >> 1 & 1, int(l["info"]) >> 2 & 3) for l in links}
        bases, boffs = g.unitigs_seqs(0, n)
        seq = lambda u, o: bases[int(boffs[u]):int(boffs[u + 1])] if o == 0 else cu.revcomp(bases[int(boffs[u]):int(boffs[u + 1])])
        nodes_of = (boffs[1:] - boffs[:-1]).astype(np.int64) - (K - 1)
        linked = rebuilt = 0
        for r, read in enumerate(case["counted"]):
            mine = segs[int(offs[r]):int(offs[r + 1])]
            assert int(mine["kmers"].sum()) == int(rec["live"][r])
            for a, b in zip(mine, mine[1:]):
                if int(b["info"]) >> 1 == 1:
                    base = int(read[int(b["read_pos"]) + K - 1])
                    assert (int(a["unitig"]), int(a["info"]) & 1, int(b["unitig"]), int(b["info"]) & 1, base) in link_set
                    linked += 1
            if rec["live"][r] == rec["kmers"][r] and rec["breaks"][r] == 0 and rec["segs"][r]:
                out = []
                for j, s in enumerate(mine):
                    u, o, i, k = int(s["unitig"]), int(s["info"]) & 1, int(s["unitig_pos"]), int(s["kmers"])
                    at = i if o == 0 else int(nodes_of[u]) - 1 - i       # where the segment starts in the oriented sequence
                    part = seq(u, o)[at:at + k + K - 1]
                    out.append(part if j == 0 else part[K - 1:])
                assert np.concatenate(out).tobytes() == np.asarray(read, dtype=np.uint8).tobytes(), r
                rebuilt += 1
        assert linked == int((want[2]["info"] >> 1 == 1).sum()) > 300 and rebuilt > 1000


# ---- 2. the cluster cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [31, 97])
def test_cluster_case_equals_the_model(pkg, synth, K):
    """short, empty and unplaced reads; polyA makes every lane a segment start; the junction under link_cut is the unlinked step"""
    case = cu.built_case(K)
    with counted_case(pkg, synth, case) as g:
        for name, p in cu.PARAM_SETS.items():
            th = tu.cluster_threading(K, name)
            indexed(g, p, th.m)
            tu.assert_threading_equal(thread_reads(g, synth, case["query"]), tu.cluster_records(K, name), f"K={K} {name}")


# ---- 3. the boundaries of a step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [31, 97])
def test_step_boundaries(pkg, synth, K):
    case = bu.built_case(K)
    th = tu.bubble_threading(K, 2, 1)
    m = th.m
    longest = max(range(len(m.unitigs)), key=lambda i: len(m.unitigs[i]["words"]))
    assert len(m.unitigs[longest]["words"]) == {31: 3030, 97: 3096}[K]
    useq = np.array(m.codes(longest), dtype=np.uint8)
    reads = []
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        for cut in (useq[500:500 + n + K - 1], cu.revcomp(useq[700:700 + n + K - 1])):
            one, segs = th.thread(cut)
            assert one == (n, n, 1, 0, longest, longest)
            reads.append(cut)
    for p in (63, 64, 65):
        # one substituted base in front of position p: the k-mers before p that hold it are not live, the first live one after them is at p
        for strand in (0, 1):
            cut = useq[1000:1000 + 200 + K - 1] if strand == 0 else cu.revcomp(useq[1000:1000 + 200 + K - 1])
            cut = cu.substituted(cut, p - 1)
            one, segs = th.thread(cut)
            assert [s[2] for s in segs][-1] == p and segs[-1][1] >> 1 == 0 and one[0] == 200 and len(segs) == (2 if p > K else 1)
            reads.append(cut)
    with counted_case(pkg, synth, case) as g:
        indexed(g, prm(2), m)
        tu.assert_threading_equal(thread_reads(g, synth, reads), th.records(reads), f"K={K}: cuts of the longest unitig")
    # the cluster case: a poly-A read whose every position starts a linked segment, and the unlinked step at p = 64
    ccase = cu.built_case(K)
    base, cut_th = tu.cluster_threading(K, "base"), tu.cluster_threading(K, "link_cut")
    poly = np.zeros(150 + K - 1, dtype=np.uint8)
    one, segs = base.thread(poly)
    assert one[:4] == (150, 150, 150, 0) and all(s[1] >> 1 == 1 for s in segs[1:])
    _, jsegs = cut_th.thread(ccase["query"][ccase["at"]["junction"]])
    (u1, i1, _, _, _, _), (u2, i2, _, _, _, _) = jsegs
    left = np.array(cut_th.m.codes(u1), dtype=np.uint8) if i1 & 1 == 0 else cu.revcomp(cut_th.m.codes(u1))
    right = np.array(cut_th.m.codes(u2), dtype=np.uint8) if i2 & 1 == 0 else cu.revcomp(cut_th.m.codes(u2))
    assert len(left) >= 64 + K - 1 and len(right) >= 70 + K - 1 and left[-(K - 1):].tobytes() == right[:K - 1].tobytes()
    long_jn = np.concatenate([left[-(64 + K - 1):], right[K - 1:K - 1 + 70]])
    one, segs = cut_th.thread(long_jn)
    assert one[:4] == (134, 134, 2, 1) and [s[2] for s in segs] == [0, 64] and segs[1][1] >> 1 == 2
    with counted_case(pkg, synth, ccase) as g:
        indexed(g, cu.PARAM_SETS["base"], base.m)
        tu.assert_threading_equal(thread_reads(g, synth, [poly, long_jn]), base.records([poly, long_jn]), f"K={K}: poly-A over three steps")
        indexed(g, cu.PARAM_SETS["link_cut"], cut_th.m)
        tu.assert_threading_equal(thread_reads(g, synth, [poly, long_jn]), cut_th.records([poly, long_jn]), f"K={K}: the unlinked step at p = 64")


# ---- 4. round a cycle -------------------------------------------------------------------------------------------------------------------------
def test_round_a_cycle(pkg, synth):
    K, n = 23, 40
    nodes = uu.cycle_graph(K, n, 3)
    m = uu.Unitigs(bu.as_model_nodes(nodes), K, min_count=1)
    th = tu.Threading(m)
    ring = np.array(m.codes(0)[:n], dtype=np.uint8)          # the cycle from x0
    read = np.concatenate([ring, ring, ring])[:85 + K - 1]
    reads = [read, cu.revcomp(read), read[7:], cu.revcomp(read[7:])]
    one, segs = th.thread(read)
    assert one == (85, 85, 3, 0, 0, 0) and [(s[3], s[4], s[1] >> 1) for s in segs] == [(0, 40, 0), (0, 40, 1), (0, 5, 1)]
    assert [(s[3], s[4], s[1]) for s in th.thread(reads[1])[1]] == [(4, 5, 1), (39, 40, 3), (39, 40, 3)]
    with imported(pkg, nodes, K) as g:
        indexed(g, prm(1), m)
        tu.assert_threading_equal(thread_reads(g, synth, reads), th.records(reads), "a read round a cycle of 40")


# ---- 5. geometry and pieces ---------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
from test_unitig_thread import whole_run
np.savez({path!r}, **whole_run(pkg, synth))
"""


def whole_run(pkg, synth):
    """the bubble case at K = 31 through the host form, the device form and the look-up -> arrays by name"""
    import torch
    K = 31
    case = bu.built_case(K)
    codes, offs = case["reads"]
    words = synth.pack_2bit(codes)
    n = len(offs) - 1
    with counted_case(pkg, synth, case) as g:
        g.unitigs_begin(prm(2))
        info = g.unitigs_index()
        rec, so, segs = g.unitigs_reads(words, offs)
        keys = cu.keys_array(sorted(case["nodes"]), g.nw)
        look = g.unitigs_lookup(keys)
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        d_rec = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
        d_so = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        total = g.unitigs_reads_device(d_w, d_o, n, d_rec, d_so)                  # the size first ...
        d_segs = torch.zeros((total, 6), dtype=torch.int32, device="cuda")
        assert g.unitigs_reads_device(d_w, d_o, n, d_rec, d_so, d_segs, total) == total      # ... then the segments
        torch.cuda.synchronize()
        return dict(info=info, rec=rec.view(np.uint32), so=so, segs=segs.view(np.uint32), look=look.view(np.uint32),
                    d_rec=d_rec.cpu().numpy().view(np.uint32).reshape(-1), d_so=d_so.cpu().numpy().view(np.uint64),
                    d_segs=d_segs.cpu().numpy().view(np.uint32).reshape(-1))


def test_geometry_and_pieces(pkg, synth, tmp_path):
    """one workgroup for every kernel and pieces of 300 reads (test hooks, so in a child process) give what the default run gives, bit for
    bit; the device form gives what the host form gives; both are the model's"""
    here = whole_run(pkg, synth)
    want = tu.bubble_records(31, 2, 1)
    tu.assert_threading_equal((here["rec"].view(tu.REC_DTYPE), here["so"], here["segs"].view(tu.SEG_DTYPE)), want, "default geometry")
    assert len(want[0]) > 2000 and (here["d_rec"] == here["rec"]).all() and (here["d_so"] == here["so"]).all() and (here["d_segs"] == here["segs"]).all()
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_WAVE_BLOCKS="1", SDT_SCAN_BLOCKS="1", SDT_SEARCH_CHUNK="300")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    there = np.load(path)
    for name, a in here.items():
        assert a.dtype == there[name].dtype and a.shape == there[name].shape and (a == there[name]).all(), name


# ---- 6. capacity and state -------------------------------------------------------------------------------------------------------------------
def test_capacity_and_state(pkg, synth):
    K = 31
    case = bu.built_case(K)
    codes, offs = case["reads"]
    words = synth.pack_2bit(codes)
    n = len(offs) - 1
    want = tu.bubble_records(K, 2, 1)
    total = len(want[2])
    keys = cu.keys_array(sorted(case["nodes"])[:5], 1)
    no_index, changed, no_list = "no sdt_gpu_unitigs_index", "the table changed since sdt_gpu_unitigs_begin", "sdt_gpu_unitigs_begin first"
    calls = lambda g: (lambda: g.unitigs_reads(words, offs), lambda: g.unitigs_lookup(keys))
    with counted_case(pkg, synth, case) as g:
        for call in calls(g) + (g.unitigs_index,):
            raises(pkg, pkg.SDT_ESTATE, call, no_list)
        g.unitigs_begin(prm(2))
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_index)
        # a clustering and a bubble list begun before the index are usable after it
        cinfo = g.cluster_begin()
        ckeys = g.cluster_components()[0].tolist()
        binfo = g.bubbles_begin(bu.DEFAULTS)
        g.unitigs_index()
        assert g.unitigs_index().tolist() == [tu.bubble_threading(K, 2, 1).m.info[0], 36, 8 * g.table_slots(), 0]      # a second index rebuilds
        # the size only; one record too few; nothing asked for
        rec, so, none = g.unitigs_reads(words, offs, segments=False)
        assert none is None and so.tolist() == want[1].tolist() and (rec == want[0]).all()
        with pytest.raises(pkg.SdtError) as e:
            g.unitigs_reads(words, offs, capacity=total - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.n_segs == total and (e.value.rec == want[0]).all() and e.value.seg_offsets.tolist() == want[1].tolist()
        tu.assert_threading_equal(g.unitigs_reads(words, offs, capacity=total), want, "exactly the room that is needed")
        nsegs = ctypes.c_uint64(77)
        assert g.lib.sdt_gpu_unitigs_reads(g._ctx, None, 0, None, 0, None, None, None, 0, ctypes.byref(nsegs)) == pkg.SDT_OK and nsegs.value == 77
        assert g.lib.sdt_gpu_unitigs_reads_device(g._ctx, None, None, 0, None, None, None, 0, None) == pkg.SDT_OK
        assert g.lib.sdt_gpu_unitigs_lookup(g._ctx, None, 0, None) == pkg.SDT_OK and len(g.unitigs_lookup(np.zeros((0, 1), dtype=np.uint64))) == 0
        # refused before any launch: NULL arguments, offsets that descend, too few words
        launches = g.kernel_time(reset=False)[1]
        r6, so1 = np.zeros(n, dtype=pkg.READ_PATH_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        assert g.lib.sdt_gpu_unitigs_reads(g._ctx, pkg._ptr(words), words.size, pkg._ptr(offs), n, None, pkg._ptr(so1), None, 0, ctypes.byref(nsegs)) == pkg.SDT_EINVAL
        assert g.lib.sdt_gpu_unitigs_reads(g._ctx, pkg._ptr(words), words.size, pkg._ptr(offs), n, pkg._ptr(r6), pkg._ptr(so1), None, 5, ctypes.byref(nsegs)) == pkg.SDT_EINVAL
        bad = offs.copy()
        bad[3] = bad[5]
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_reads(words, bad), "not monotonic")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_reads(words[:10], offs), "too short")
        assert g.kernel_time(reset=False)[1] == launches
        # the clustering and the bubble list are what they were
        assert g.cluster_components()[0].tolist() == ckeys and int(g.cluster_begin()[2]) == int(cinfo[2])
        bu.assert_bubbles_equal(g, case["model"], binfo, "the bubble list across an index and the reads")
        tu.assert_threading_equal(g.unitigs_reads(words, offs), want, "the index across a cluster_begin")
        # a second begin without an index; end
        g.unitigs_begin(prm(2))
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, no_index)
        g.unitigs_index()
        g.unitigs_end()
        for call in calls(g) + (g.unitigs_index,):
            raises(pkg, pkg.SDT_ESTATE, call, no_list)
        # the table changes under an index
        g.unitigs_begin(prm(2))
        g.unitigs_index()
        g.delow(1)
        for call in calls(g) + (g.unitigs_index,):
            raises(pkg, pkg.SDT_ESTATE, call, changed)
        g.unitigs_begin(prm(2))
        g.unitigs_index()                                                        # (a context destroyed with an index frees it)
