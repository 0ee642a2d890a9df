"""GPU (-m gpu): reads clustered by connected component of the counted k-mer graph (sdt_gpu_cluster_*) against the Python restatement
of the rule (read_cluster_util.py): info, the component list, look-ups and the read records, all exact.  The nodes of the model come
from the oracle, never from the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import read_cluster_util as cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counted(pkg, synth, codes, offs, K, want=None, flags=0, est_distinct=1 << 16):
    g = pkg.PregraphGPU(K, est_distinct=est_distinct, flags=flags)
    g.push_reads(synth.pack_2bit(codes), offs)
    got = g.finish_count()
    assert want is None or got == want, (got, want)
    return g


def counted_case(pkg, synth, case, **kw):
    return counted(pkg, synth, *case["reads"], case["K"], (case["kmers_in_reads"], case["node_count"]), **kw)


def cluster_batch(g, synth, reads, **kw):
    codes, offs = cu.concat(reads)
    return g.cluster_reads(synth.pack_2bit(codes), offs, **kw)


def check_lookup(g, model, nodes, K, rng):
    """every node key on both strands, and absent keys"""
    ks = list(nodes)
    want = [model.label.get(k, cu.NONE) for k in ks]
    assert g.cluster_lookup(cu.keys_array(ks, g.nw)).tolist() == want
    assert g.cluster_lookup(cu.keys_array([cu.rc_int(k, K) for k in ks], g.nw)).tolist() == want
    absent = [int.from_bytes(rng.bytes(32), "big") & ((1 << (2 * K)) - 1) for _ in range(100)]
    absent = [k for k in absent if cu.canon(k, K) not in nodes]
    assert len(absent) >= 90 and (g.cluster_lookup(cu.keys_array(absent, g.nw)) == cu.NONE).all()


def check_all(pkg, synth, g, case, name, what):
    model, query = case["models"][name], case["query"]
    info = g.cluster_begin(cu.PARAM_SETS[name])
    cu.assert_clustering_equal(pkg, g, model, info, what)
    check_lookup(g, model, case["nodes"], case["K"], np.random.default_rng(5))
    for paired in (False, True):
        rec, keep, kept = cluster_batch(g, synth, query, paired=paired)
        wrec, wkeep, wkept = model.records(query, paired=paired)
        cu.assert_records_equal(rec, wrec, f"{what} paired={paired}")
        assert (keep == wkeep).all() and kept == wkept == int((wrec["unit"] != cu.NONE).sum())
    return info


# ---- 1. the model, per key width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(23, 0), (31, 1), (31, 2), (47, 0), (63, 0), (95, 0), (127, 0), (33, 0), (65, 0), (97, 0)])
def test_clustering_equals_the_model(pkg, synth, K, flags):
    """1, 2 and 4 key words, both pass-1 kernel families at K = 31; the four parameter sets the case is built around"""
    case = cu.built_case(K)
    with counted_case(pkg, synth, case, flags=flags) as g:
        assert g.nw == (1 if K <= 31 else 2 if K <= 63 else 4)
        clusters = {name: int(check_all(pkg, synth, g, case, name, f"K={K} flags={flags} {name}")[2]) for name in cu.PARAM_SETS}
        assert len(set(clusters.values())) == 4, clusters
        g.cluster_end()


# ---- 2. ids do not depend on the layout ----------------------------------------------------------------------------------------------------
def test_layout_independence(pkg, synth):
    case = cu.built_case(31)
    model, query = case["models"]["base"], case["query"]
    got, slots = [], []
    for est, flags in ((1 << 16, 0), (1 << 20, 0), (1 << 16, pkg.SDT_FLAG_DIRECT)):
        with counted_case(pkg, synth, case, flags=flags, est_distinct=est) as g:
            slots.append(g.table_slots())
            info = g.cluster_begin(cu.PARAM_SETS["base"])
            cu.assert_clustering_equal(pkg, g, model, info, f"est_distinct={est} flags={flags}")
            keys, comp = g.cluster_components()
            got.append((info.tolist(), keys.tolist(), comp.tolist(), cluster_batch(g, synth, query, paired=True)[0].tolist()))
    assert slots[0] != slots[1]
    assert got[0] == got[1] == got[2]


# ---- 3. depth and contention -----------------------------------------------------------------------------------------------------------------
DEEP_K, DEEP_L = 31, 100


def deep_reads():
    """one linear sequence of 20 000 bases, a circular one of 5 000, one random sequence of 50 000 bases at 40-fold coverage, and 200
    small transcripts"""
    rng = np.random.default_rng(2024)
    L = DEEP_L
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    reads = cu.tiled(rnd(20000), L, step=25)
    circle = rnd(5000)
    reads += cu.tiled(np.concatenate([circle, circle[:L]]), L, step=25)           # (the tiles run over the seam)
    big = rnd(50000)
    for s in rng.integers(0, len(big) - L + 1, size=40 * len(big) // L).tolist():
        reads.append(big[s:s + L] if s & 1 else cu.revcomp(big[s:s + L]))
    for _ in range(200):
        reads += cu.tiled(rnd(300), L, step=20)
    return reads


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_cluster_util as cu
from test_read_cluster import counted, deep_reads, DEEP_K
reads = deep_reads()
codes, offs = cu.concat(reads)
with counted(pkg, synth, codes, offs, DEEP_K, est_distinct=1 << 18) as g:
    info = g.cluster_begin(dict(min_count=2, max_count=0, min_link=1))
    keys, comp = g.cluster_components()
    rec, keep, kept = g.cluster_reads(synth.pack_2bit(codes), offs)
np.savez({path!r}, info=info, keys=keys, comp=comp, rec=rec, kept=kept)
"""


def test_depth_and_contention(pkg, synth, tmp_path):
    """two workgroups for every scan and every walk (test hooks), in a child process under a time limit: a chain of 20 000 nodes, a
    cycle, one cluster that holds most of the link ends, and 200 small ones.  The sequences listed make 1 + 1 + 1 + 200 = 203 clusters
    (the model says so before the child starts); a child that runs into its time limit fails the test."""
    reads = deep_reads()
    codes, offs = cu.concat(reads)
    nodes = cu.oracle_nodes(cu.counted_oracle(codes, offs, DEEP_K))
    model = cu.Clustering(nodes, DEEP_K, 2, 0, 1)
    assert model.info[2] == 203 and model.info[3] > 49000
    sizes = sorted(c[1] for c in model.comps)
    assert sizes[-3:-1] == [5000, 20000 - DEEP_K + 1] and sizes[:200] == [300 - DEEP_K + 1] * 200
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SCAN_BLOCKS="2", SDT_WAVE_BLOCKS="2")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    assert got["info"].tolist() == model.info
    assert [cu.key_int(k) for k in got["keys"].tolist()] == [c[0] for c in model.comps]
    assert got["comp"]["nodes"].tolist() == [c[1] for c in model.comps] and got["comp"]["count_sum"].tolist() == [c[2] for c in model.comps]
    wrec, _, wkept = model.records(reads)
    cu.assert_records_equal(got["rec"], wrec, "depth and contention")
    assert int(got["kept"]) == wkept


# ---- 4. after delow ----------------------------------------------------------------------------------------------------------------------------
def raises(pkg, code, call, *words):
    with pytest.raises(pkg.SdtError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_after_delow(pkg, synth):
    case = cu.built_case(31)
    query = case["query"]
    o = cu.counted_oracle(*case["reads"], 31)
    removed = o.delow(1)
    nodes = cu.oracle_nodes(o)
    prm = dict(min_count=1, max_count=0, min_link=1)      # (a node seen once would be live: what keeps it out is what delow did)
    model = cu.Clustering(nodes, 31, **prm)
    # (delow takes the nodes seen once away, and with them the bridge; it also clears the link counters of 1, and with them the junction)
    assert removed > 0 and model.info[2] == case["models"]["link_cut"].info[2] > case["models"]["bridge"].info[2]
    with counted_case(pkg, synth, case) as g:
        info = g.cluster_begin(prm)
        cu.assert_clustering_equal(pkg, g, case["models"]["bridge"], info, "before delow")
        assert g.delow(1) == removed
        raises(pkg, pkg.SDT_ESTATE, lambda: cluster_batch(g, synth, query), "the table changed since sdt_gpu_cluster_begin")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_components(), "the table changed since sdt_gpu_cluster_begin")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_lookup(cu.keys_array([5], 1)), "the table changed since sdt_gpu_cluster_begin")
        info = g.cluster_begin(prm)
        cu.assert_clustering_equal(pkg, g, model, info, "after delow")
        check_lookup(g, model, nodes, 31, np.random.default_rng(6))
        cu.assert_records_equal(cluster_batch(g, synth, query, paired=True)[0], model.records(query, paired=True)[0], "after delow")


# ---- 5. keep bytes, and on into a compaction -----------------------------------------------------------------------------------------------------
def test_keep_bytes_and_compaction(pkg, synth):
    import torch
    case = cu.built_case(31)
    model, query = case["models"]["base"], case["query"]
    n = len(query)
    codes, offs = cu.concat(query)
    wrec = model.records(query, paired=True)[0]
    one = int(wrec["unit"][case["at"]["mates_apart"]])
    far = model.info[2] + 5
    with counted_case(pkg, synth, case) as g:
        g.cluster_begin(cu.PARAM_SETS["base"])
        d_w = torch.from_numpy(synth.pack_2bit(codes).view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        for lo, hi in ((one, one), (2, 9), (far, far + 3), (0, cu.NONE)):
            _, wkeep, wkept = model.records(query, paired=True, pick=(lo, hi))
            assert (wkept > 0) == (lo < far) and (wkeep[0::2] == wkeep[1::2]).all()
            d_rec = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            assert g.cluster_reads_device(d_w, d_o, n, d_rec, d_keep, paired=True, pick_lo=lo, pick_hi=hi) == wkept
            cu.assert_records_equal(d_rec.cpu().numpy().view(np.uint32).view(cu.DTYPE).reshape(n), wrec, f"device form, pick {lo}..{hi}")
            assert (d_keep.cpu().numpy() == wkeep).all()
            d_ow = torch.zeros(d_w.numel() + 4, dtype=torch.int32, device="cuda")
            d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            nr, nwords = g.compact_reads_device(d_w, d_o, n, d_keep, d_ow, d_ow.numel(), d_oo)
            kept_reads = [q for q, k in zip(query, wkeep) if k]
            kc, ko = cu.concat(kept_reads)
            assert nr == wkept and (d_oo.cpu().numpy()[:nr + 1].view(np.uint64) == ko).all()
            assert (d_ow.cpu().numpy()[:nwords].view(np.uint32) == synth.pack_2bit(kc)[:nwords]).all()
        # without a count the call only enqueues; the host form agrees
        d_rec = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
        assert g.cluster_reads_device(d_w, d_o, n, d_rec, None, paired=True, wait=False) is None
        torch.cuda.synchronize()
        cu.assert_records_equal(d_rec.cpu().numpy().view(np.uint32).view(cu.DTYPE).reshape(n), wrec, "device form, enqueued")


# ---- 6. the kept form ------------------------------------------------------------------------------------------------------------------------------
def test_kept_form_equals_the_dense_form_by_ordinal(pkg, synth, monkeypatch):
    """a single-end batch, then a paired stream pushed as two batches with strides: interleaved pairs; the dense form in pieces of 7"""
    K = 31
    case = cu.built_case(K)
    singles = [case["query"][i] for i in range(26, 59)]                          # an odd number: the pair range starts at an odd ordinal
    m1, m2 = case["query"][0:26:2], case["query"][1:26:2]
    reads = singles + [r for pair in zip(m1, m2) for r in pair]
    first, end, total = len(singles), len(singles) + 2 * len(m1), len(singles) + 2 * len(m1)
    assert first & 1
    codes, offs = cu.concat(reads)
    model = cu.Clustering(cu.oracle_nodes(cu.counted_oracle(codes, offs, K)), K, 1, 0, 1)
    units = [[i] for i in range(first)] + [[i, i + 1] for i in range(first, end, 2)]
    wrec, wkeep, wkept = model.records(reads, units=units, pick=(0, 3))
    assert {cu.WHOLE, cu.NOT_WHOLE, cu.THROUGH_MATE, cu.SHORT} <= set(wrec["verdict"].tolist()) and 0 < wkept < total
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for part, base, stride in ((singles, 0, 1), (m1, first, 2), (m2, first + 1, 2)):
            c, o = cu.concat(part)
            g.set_read_ordinal(base, stride)
            g.push_reads(synth.pack_2bit(c), o)
        g.finish_count()
        g.cluster_begin(dict(min_count=1))
        out = np.full(total + 3, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLUSTER_DTYPE)
        rec, n, kept = g.cluster_kept_reads(total + 3, [(first, end)], pick_lo=0, pick_hi=3, out=out)
        assert n == total and kept == wkept and (rec[total:].view(np.uint32) == 0xABABABAB).all()
        cu.assert_records_equal(rec[:total], wrec, "kept form")
        # the dense form of the paired part, in pieces
        monkeypatch.setenv("SDT_SEARCH_CHUNK", "7")
        dense, dkeep, dkept = cluster_batch(g, synth, reads[first:], paired=True, pick_lo=0, pick_hi=3)
        cu.assert_records_equal(dense, wrec[first:], "dense form in pieces")
        assert (dkeep == wkeep[first:]).all() and dkept == int(wkeep[first:].sum())
        # no ranges: every read on its own
        srec = model.records(reads)[0]
        cu.assert_records_equal(g.cluster_kept_reads(total)[0], srec, "kept form, no ranges")
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLUSTER_DTYPE)
        raises(pkg, pkg.SDT_EFULL, lambda: g.cluster_kept_reads(total - 1, [(first, end)], out=small), "ordinal")
        assert (small.view(np.uint32) == 0xABABABAB).all()
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_kept_reads(total, [(first, first + 3)]), "range")


def test_kept_pair_with_one_mate_in_hbm(pkg, synth):
    """only the read-1 file of a paired stream is kept: every pair is judged on that mate alone"""
    K = 31
    case = cu.built_case(K)
    m1 = case["query"][0:60:2]
    n = len(m1)
    codes, offs = cu.concat(m1)
    model = cu.Clustering(cu.oracle_nodes(cu.counted_oracle(codes, offs, K)), K, 1, 0, 1)
    want = model.records(m1)[0]
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.set_read_ordinal(0, 2)
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.cluster_begin(dict(min_count=1))
        out = np.full(2 * n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_CLUSTER_DTYPE)
        rec, got_n, kept = g.cluster_kept_reads(2 * n, [(0, 2 * n)], out=out)
        assert got_n == n and kept == int((want["unit"] != cu.NONE).sum())
        cu.assert_records_equal(np.ascontiguousarray(rec[0::2]), want, "the mates that are there")
        assert (np.ascontiguousarray(rec[1::2]).view(np.uint32) == 0xABABABAB).all()


# ---- 7. state and arguments ------------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(pkg, synth, monkeypatch):
    case = cu.built_case(31)
    K, query = 31, case["query"]
    codes, offs = case["reads"]
    words = synth.pack_2bit(codes)
    qc, qo = cu.concat(query)
    qw = synth.pack_2bit(qc)
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(words, offs)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_begin(), "sdt_gpu_cluster_begin", "sdt_gpu_finish_count")
        g.finish_count()
        for call in (lambda: g.cluster_reads(qw, qo), lambda: g.cluster_components(), lambda: g.cluster_lookup(cu.keys_array([5], 1)),
                     lambda: g.cluster_kept_reads(4)):
            raises(pkg, pkg.SDT_ESTATE, call, "sdt_gpu_cluster_begin first")
        g.cluster_end()                                                        # (nothing to free: fine)
        # the parameters
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_begin(dict(flags=1)), "flags")
        for ml in (0, 64):
            raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_begin(dict(min_link=ml)), "min_link", str(ml))
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_begin(dict(min_count=5, max_count=4)), "max_count")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_begin(dict(min_count=0, max_count=0, min_link=1, flags=2)), "flags")
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_components(), "sdt_gpu_cluster_begin first")       # (a refused begin begins nothing)
        assert int(g.cluster_begin(dict(min_count=0, max_count=1))[0]) > 0     # (min_count 0 is 1: max_count 1 is allowed)
        info = g.cluster_begin(cu.PARAM_SETS["base"])                          # a second begin replaces the first
        cu.assert_clustering_equal(pkg, g, case["models"]["base"], info, "second begin")
        # a table too large for 32-bit labels (test hook: the limit, 2^32 - 2 slots, is brought down to where this table lies above it)
        monkeypatch.setenv("SDT_CLUSTER_MAX_SLOTS", str(g.table_slots() - 1))
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_begin(), "slots", "32-bit")
        assert len(g.cluster_components()[1]) == int(info[2])                 # (a refused begin leaves the clustering that was there)
        monkeypatch.setenv("SDT_CLUSTER_MAX_SLOTS", str(g.table_slots()))
        info = g.cluster_begin(cu.PARAM_SETS["base"])
        monkeypatch.delenv("SDT_CLUSTER_MAX_SLOTS")
        # the component list into too little room
        with pytest.raises(pkg.SdtError) as e:
            g.cluster_components(capacity=3)
        assert e.value.code == pkg.SDT_EFULL and e.value.needed == int(info[2])
        # an odd number of paired reads; offsets that descend; words that are too few; no read at all
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_reads(qw, qo[:-1], paired=True), "odd")
        bad = qo.copy()
        bad[2] = bad[1] - 1
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_reads(qw, bad), "monotonic")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.cluster_reads(qw[:-5], qo), "too short")
        rec, keep, kept = g.cluster_reads(np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint64), paired=True)
        assert len(rec) == 0 and kept == 0
        assert len(g.cluster_lookup(np.zeros((0, 1), dtype=np.uint64))) == 0
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_kept_reads(4), "kept")  # (the reads were not kept)
        # the table changes: a push and finish_count after begin
        g.push_reads(words, offs[:41])
        g.finish_count()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_reads(qw, qo), "the table changed since sdt_gpu_cluster_begin")
        g.cluster_begin()
        assert len(g.cluster_reads(qw, qo)[0]) == len(query)
        # end, then the records
        g.cluster_end()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_reads(qw, qo), "sdt_gpu_cluster_begin first")
        g.cluster_begin()
        g.release_table()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_begin(), "sdt_gpu_cluster_begin", "released")
    with counted_case(pkg, synth, case) as g:
        g.load_paths(None, None, None, None, 0)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_begin(), "sdt_gpu_cluster_begin", "path words")
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_begin(), "sdt_gpu_cluster_begin", "SDT_FLAG_CONTIG_INDEX")
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:                        # a context with a communicator holds one shard
        g.comm_init_shm(f"sdt_cluster_{os.getpid()}", 0, 1)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.cluster_begin(), "sdt_gpu_cluster_begin", "shard")
    # a context destroyed with a clustering open frees it
    with counted_case(pkg, synth, case) as g:
        g.cluster_begin()


def test_the_table_is_untouched(pkg, synth):
    case = cu.built_case(31)

    def snapshot(g):
        keys, l, rf, cnt = g.export_nodes()[:4]
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt)]

    with counted_case(pkg, synth, case) as g:
        before = snapshot(g)
        check_all(pkg, synth, g, case, "base", "between two snapshots")
        for a, b in zip(before, snapshot(g)):
            assert a.shape == b.shape and (a == b).all()
