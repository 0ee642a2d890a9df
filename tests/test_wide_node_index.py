"""64-bit node indices of the device's graph phases: a graph past 2^32 - 16 nodes keeps layout, cutting and edges on the device
(sdt_gpu_set_graph_index_bits / sdt_gpu_graph_index_bits / sdt_gpu_build_host_index64).  On the golden cases the CLI is told that
the graph is past its node limit (SDT_NODE_LIMIT), and the nodes are numbered from a base past 2^32 (SDT_NODE_BASE), so that a node
index cut to 32 bits anywhere on the device would change the output."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu

WIDE_SYMBOLS = ("sdt_gpu_build_host_index64", "sdt_gpu_set_graph_index_bits", "sdt_gpu_graph_index_bits")
BASE = (1 << 32) + 12345


def test_library_exports_the_wide_index_entry_points(pkg):
    lib = pkg.load_library()
    for s in WIDE_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s


def _materialise(info, tmp):
    d = info["dir"]
    for f in os.listdir(d):
        if f.endswith(".fq.gz"):
            with gzip.open(os.path.join(d, f), "rb") as fi, open(os.path.join(tmp, f[:-3]), "wb") as fo:
                fo.write(fi.read())
    cfg = os.path.join(tmp, "lib.cfg")
    with open(os.path.join(d, "lib.cfg.template")) as fi, open(cfg, "w") as fo:
        fo.write(fi.read().replace("@DIR@", str(tmp)))
    return cfg


def _pregraph(pkg, info, tmp_path, base, extra=(), env_extra=None, timeout=600):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-pregraph")
    if not os.path.exists(exe):
        pkg.build()
    cfg = _materialise(info, tmp_path)
    cmd = [exe, "pregraph", "-s", cfg, "-K", str(info["K"]), "-p", str(info["p"]), "-o", str(tmp_path / "out"),
           "--max-k", str(gu.VARIANT_MAXK[info["variant"]])] + list(extra)
    if info["d"]:
        cmd += ["-d", str(info["d"])]
    if info.get("a"):
        cmd += ["-a", str(info["a"])]
    env = dict(os.environ, SDT_NODE_LIMIT="1000", **(env_extra or {}))
    if base is not None:
        env["SDT_NODE_BASE"] = str(base)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "past the 32-bit node indices" in r.stderr and "64-bit node indices" in r.stderr, r.stderr[-2000:]
    assert "run on the host" not in r.stderr, r.stderr[-2000:]
    return r


def _five_files_equal_goldens(info, tmp_path):
    assert open(tmp_path / "out.kmerFreq").read() == gu.golden_text(info, "kmerFreq")
    assert open(tmp_path / "out.vertex").read() == gu.golden_text(info, "vertex")
    assert gzip.open(tmp_path / "out.edge.gz", "rt").read() == gzip.open(os.path.join(info["dir"], "out.edge.txt.gz"), "rt").read()
    assert open(tmp_path / "out.preGraphBasic").read() == gu.golden_text(info, "preGraphBasic")
    assert open(tmp_path / "out.preArc").read() == gu.golden_text(info, "preArc")


@pytest.mark.gpu
@pytest.mark.parametrize("base", [None, BASE], ids=["base0", "base2^32+12345"])
@pytest.mark.parametrize("name", gu.case_names())
def test_cli_past_the_node_limit_stays_on_the_device(pkg, tmp_path, name, base):
    """past the node limit the CLI asks for the 64-bit form and keeps the graph phases on the device (the parent commit took the host
    route here): all five files of the reference, and its counters, byte for byte"""
    info = gu.load_case(name)
    assert info["nodes_allocated"] >= 1000
    r = _pregraph(pkg, info, tmp_path, base)
    _five_files_equal_goldens(info, tmp_path)
    assert [int(x) for x in re.findall(r"(\d+) tips off", r.stdout)] == info["tips_off"]
    assert [int(x) for x in re.findall(r"(\d+) linear nodes", r.stdout)] == info["linear_after"]
    m = re.search(r"(\d+) nodes allocated, (\d+) kmer in reads, (\d+) kmer processed", r.stdout)
    assert (int(m.group(1)), int(m.group(2))) == (info["nodes_allocated"], info["kmer_in_reads"])


@pytest.mark.gpu
@pytest.mark.parametrize("base", [None, BASE], ids=["base0", "base2^32+12345"])
@pytest.mark.parametrize("name", ["pe150_k31_p8", "se250_k63_p8_127mer", "dirty_ragged_k25_cut80",
                                  # 1 000-base reads through the sharded count stage.  (Not se1000_k63_p3_127mer: the sharded path refuses
                                  # 1 000-base reads at K = 63 with SDT_EINVAL, tests/test_read_lengths.py pins it.)
                                  "se1000_k31_p4"])
def test_cli_ranks_past_the_node_limit_use_rank0s_device_table(pkg, tmp_path, name, base):
    """`--gpus 3`: past the node limit the shards go into rank 0's device table and the graph phases run there in the 64-bit form"""
    info = gu.load_case(name)
    _pregraph(pkg, info, tmp_path, base, extra=["--gpus", "3", "--share-device"], env_extra={"SDT_CHUNK_BYTES": "30000"}, timeout=900)
    _five_files_equal_goldens(info, tmp_path)


def _same_host_index(a, b):
    """two linear-probing tables over the same keys: the occupied slots do not depend on the order of insertion, the entries inside a
    cluster (a run of occupied slots) may come in any order when threads race"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    occ = a != 0
    assert (occ == (b != 0)).all()
    r = int(np.flatnonzero(~occ)[0]) + 1
    a, b, occ = np.roll(a, -r), np.roll(b, -r), np.roll(occ, -r)
    cid = np.cumsum(~occ)
    assert (a[np.lexsort((a, cid))] == b[np.lexsort((b, cid))]).all()


def _same_partition(x, y):
    x, y = [int(v) for v in x], [int(v) for v in y]
    assert len(x) == len(y)
    fw, bw = {}, {}
    for p, q in zip(x, y):
        assert fw.setdefault(p, q) == q and bw.setdefault(q, p) == p


def _same_records(ra, rb, nj):
    """minor-out records: the junction records [0, nj) in the same order (by label, node), the records behind them in the order they
    were appended (one per node: compared by node); labels (word 13) as partitions"""
    ta, tb = ra[nj:][np.argsort(ra[nj:, 0], kind="stable")], rb[nj:][np.argsort(rb[nj:, 0], kind="stable")]
    xa, xb = np.concatenate([ra[:nj], ta]), np.concatenate([rb[:nj], tb])
    assert (xa[:, :13] == xb[:, :13]).all()
    _same_partition(xa[:, 13], xb[:, 13])


@pytest.mark.gpu
@pytest.mark.parametrize("K,L,variant,p", [(31, 150, 1, 4), (47, 150, 2, 5), (75, 200, 4, 3), (97, 250, 4, 5)])
def test_wide_form_equals_the_narrow_one(pkg, synth, monkeypatch, K, L, variant, p):
    """two contexts on the same reads, the default form and the 64-bit one with the nodes numbered from 2^32 + 12345: layout, labelled
    walks, labelled junctions, the minor-out commit, the edges and the host's look-up index agree"""
    monkeypatch.setenv("SDT_NODE_BASE", str(BASE))       # (read by the 64-bit form only)
    tx = synth.make_transcriptome(8, seed=K + 51)
    codes, offs = synth.sample_reads(*tx, n_reads=5000, read_len=L, seed=K + 52, err=0.01)
    packed = synth.pack_2bit(codes)
    ctxs = []
    try:
        for wide in (False, True):
            g = pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST)
            ctxs.append(g)
            g.push_reads(packed, offs)
            g.finish_count()
            g.mark_and_hist()
            if wide:
                assert g.lib.sdt_gpu_set_graph_index_bits(g._ctx, 64) == 0
                assert g.lib.sdt_gpu_set_graph_index_bits(g._ctx, 48) != 0
            assert g.lib.sdt_gpu_graph_index_bits(g._ctx) == (64 if wide else 32)
        a, b = ctxs
        for g in ctxs:
            g.layout_on_device(p, variant)
        assert a.lib.sdt_gpu_graph_index_bits(a._ctx) == 32 and b.lib.sdt_gpu_graph_index_bits(b._ctx) == 64
        ea, eb = a.export_ordered(), b.export_ordered()
        for x, y in zip(ea, eb):
            assert (x == y).all()
        n = len(ea[0])
        # labelled walks: node | info, end node; labels as partitions
        for thin, cut_len in ((1, 2 * K), (0, 2 * K), (0, 5)):
            ra, rb = a.tip_walks_labelled(bool(thin), cut_len), b.tip_walks_labelled(bool(thin), cut_len)
            assert len(ra) > 0 and (ra[:, :2] == rb[:, :2]).all()
            assert int((rb[:, 0] & np.uint64((1 << 56) - 1)).max()) < n and int(rb[:, 1].max()) < n      # (positions: no base left)
            _same_partition(ra[:, 2], rb[:, 2])
        # labelled junctions
        for thr in (0.05, 0.3):
            (ra, nja), (rb, njb) = a.minor_out_labelled(thr), b.minor_out_labelled(thr)
            assert nja == njb > 0 and len(ra) == len(rb)
            _same_records(ra, rb, nja)
        # the commit (a component limit that leaves some components to the caller)
        ca, cb = a.minor_out_commit(0.3, max_component=2), b.minor_out_commit(0.3, max_component=2)
        for k in ("n_junctions", "largest", "off", "linear"):
            assert ca[k] == cb[k], k
        assert ca["off"] > 0
        _same_records(ca["records"], cb["records"], ca["n_junctions"])
        _same_records(np.concatenate([ca["skipped"], ca["skipped_neighbours"]]), np.concatenate([cb["skipped"], cb["skipped_neighbours"]]), len(ca["skipped"]))
        wa, wb = np.argsort(ca["node"]), np.argsort(cb["node"])
        assert (ca["node"][wa] == cb["node"][wb]).all() and int(cb["node"].max()) < n
        assert (ca["l_links"][wa] == cb["l_links"][wb]).all() and (ca["r_flags"][wa] == cb["r_flags"][wb]).all()
        for x, y in zip(a.export_ordered(), b.export_ordered()):
            assert (x == y).all()
        # kmer2edges
        (rec_a, bases_a, ids_a), (rec_b, bases_b, ids_b) = a.build_edges(), b.build_edges()
        assert ids_a == ids_b > 0 and bases_a == bases_b and (rec_a == rec_b).all()
        # the host's look-up index: 64-bit entries from the wide context, 32-bit ones from the narrow one, widened
        cap = 1024
        while cap < 2 * n + 2:
            cap <<= 1
        i32 = np.zeros(cap, dtype=np.uint32)
        i64 = np.zeros(cap, dtype=np.uint64)
        assert a.lib.sdt_gpu_build_host_index(a._ctx, i32.ctypes.data, cap) == 0
        assert b.lib.sdt_gpu_build_host_index64(b._ctx, i64.ctypes.data, cap) == 0
        assert int(i64.max()) == n and int((i64 != 0).sum()) == n
        _same_host_index(i32.astype(np.uint64), i64)
    finally:
        for g in ctxs:
            g.close()
