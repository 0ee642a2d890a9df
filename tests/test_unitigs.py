"""GPU (-m gpu): the unitigs of the counted k-mer graph and their links (sdt_gpu_unitigs_*) against the Python restatement of the rule
(unitig_util.py): info, records, first and last words, sequences and links, all exact.  The nodes of the model come from the oracle or
are written by hand, never from the library."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_util as uu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K23 = 23


def counted(pkg, synth, codes, offs, K, want=None, flags=0, est_distinct=1 << 16):
    g = pkg.PregraphGPU(K, est_distinct=est_distinct, flags=flags)
    g.push_reads(synth.pack_2bit(codes), offs)
    got = g.finish_count()
    assert want is None or got == want, (got, want)
    return g


def counted_case(pkg, synth, case, **kw):
    return counted(pkg, synth, *case["reads"], case["K"], (case["kmers_in_reads"], case["node_count"]), **kw)


def imported(pkg, nodes, K):
    """a fresh context that holds the hand-made nodes"""
    g = pkg.PregraphGPU(K, est_distinct=1 << 12)
    g.import_nodes(*bu.node_arrays(nodes, g.nw))
    assert g.finish_count()[1] == len(nodes)
    return g


def raises(pkg, code, call, *words):
    with pytest.raises(pkg.SdtError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def whole_list(g, info):
    n = int(info[2])
    keys, rec = g.unitigs_fetch(0, n)
    bases, offs = g.unitigs_seqs(0, n)
    links, dangling = g.unitigs_links(0, n)
    return info.tolist(), keys.tolist(), rec.tolist(), bases.tobytes(), offs.tolist(), links.tolist(), dangling


# ---- 1. the model, per key width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(23, 0), (31, 1), (31, 2), (47, 0), (63, 0), (95, 0), (127, 0), (33, 0), (65, 0), (97, 0)])
def test_unitigs_equal_the_model(pkg, synth, K, flags):
    """1, 2 and 4 key words, both pass-1 kernel families at K = 31; min_count 2 and 1, and an upper bound with min_link 3"""
    case = bu.built_case(K)
    with counted_case(pkg, synth, case, flags=flags) as g:
        assert g.nw == (1 if K <= 31 else 2 if K <= 63 else 4)
        for prm, n in ((uu.DEFAULTS, 36), (dict(uu.DEFAULTS, min_count=1), 41), (dict(min_count=2, max_count=40, min_link=3), None)):
            model = uu.Unitigs(case["nodes"], K, **prm)
            assert n is None or model.info[2] == n
            uu.assert_unitigs_equal(g, model, g.unitigs_begin(prm), f"K={K} flags={flags} {prm}")
        g.unitigs_end()


# ---- 2. the list does not depend on the layout ---------------------------------------------------------------------------------------------
def test_layout_independence(pkg, synth):
    case = bu.built_case(31)
    model = uu.Unitigs(case["nodes"], 31, **uu.DEFAULTS)
    got, slots = [], []
    for est, flags in ((1 << 16, 0), (1 << 20, 0), (1 << 16, pkg.SDT_FLAG_DIRECT)):
        with counted_case(pkg, synth, case, flags=flags, est_distinct=est) as g:
            slots.append(g.table_slots())
            info = g.unitigs_begin(uu.DEFAULTS)
            uu.assert_unitigs_equal(g, model, info, f"est_distinct={est} flags={flags}")
            got.append(whole_list(g, info))
    with counted(pkg, synth, *bu.reverse_complemented(case), 31) as g:
        got.append(whole_list(g, g.unitigs_begin(uu.DEFAULTS)))
    assert slots[0] != slots[1]
    assert got[0] == got[1] == got[2] == got[3]


# ---- 3. graphs written by hand -----------------------------------------------------------------------------------------------------------------
def check_hand(pkg, nodes, K, what, **params):
    prm = dict(uu.DEFAULTS, **params)
    model = uu.Unitigs(bu.as_model_nodes(nodes), K, **prm)
    with imported(pkg, nodes, K) as g:
        uu.assert_unitigs_equal(g, model, g.unitigs_begin(prm), what)
    uu.assert_overlaps(model)
    return model


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def test_small_hand_graphs(pkg):
    K = K23
    m = check_hand(pkg, bu.hand_graph([rnd(1, K)], K), K, "one isolated node")
    assert m.info == [1, 2, 1, 0, 1, K, 1, 0] and m.links == [] and m.records()["info"][0] == 0
    m = check_hand(pkg, bu.hand_graph([rnd(2, K + 2)], K), K, "a chain of 3")
    assert m.info == [3, 2, 1, 0, 3, K + 2, 3, 0] and m.links == []
    # a Y fork: three unitigs, links on both strands
    stem, arm, other = rnd(3, 60), rnd(4, 40), rnd(6, 40)
    other[0] = (arm[0] + 1) & 3
    m = check_hand(pkg, bu.hand_graph([np.concatenate([stem, arm]), np.concatenate([stem, other])], K), K, "a Y fork")
    seen = {(u, o, v, o2) for u, v, o, o2, _, _ in m.links}
    assert m.info[2] == 3 and len(seen) == 4 and all((v, 1 - o2, u, 1 - o) in seen for u, o, v, o2 in seen) and m.dangling == 0
    assert sorted((r >> 4 & 15) + (r >> 8 & 15) for r in m.records()["info"].tolist()) == [1, 1, 2]      # the stem's fork end, an end of each arm
    # one substitution site: four unitigs
    ref = rnd(7, 3 * K + 10)
    m = check_hand(pkg, bu.hand_graph([ref, cu.substituted(ref, K + 5)], K), K, "one substitution site")
    assert m.info[2] == 4 and len(m.links) == 8 and sorted(len(t["counts"]) for t in m.unitigs)[1:3] == [K, K]
    # poly-A: one node, a link to itself, and it joins nothing
    m = check_hand(pkg, bu.hand_graph([np.zeros(K + 3, dtype=np.uint8)], K), K, "poly-A")
    assert m.info == [1, 2, 1, 0, 1, K, 1, 0] and [(u, v, o, o2, b) for u, v, o, o2, b, _ in m.links] == [(0, 0, 0, 0, 0), (0, 0, 1, 1, 2)]
    assert m.records()["info"][0] == 0 | 1 << 4 | 1 << 8
    # an inverted repeat: the last word of the unitig is followed by its own reverse complement -- a hairpin link, and no join
    half = rnd(8, 40)
    m = check_hand(pkg, bu.hand_graph([np.concatenate([half, cu.revcomp(half)])], K), K, "an inverted repeat")
    n = (2 * 40 - K + 1) // 2
    assert m.info == [n, 2, 1, 0, n, n + K - 1, n, 0] and len(m.links) == 1 and m.links[0][:2] == (0, 0) and m.links[0][2] != m.links[0][3]
    assert len(m.gfa_links()) == 1


def test_cycles(pkg):
    K = K23
    m = check_hand(pkg, uu.cycle_graph(K, 200, 11), K, "a cycle of 200")
    assert m.info == [200, 0, 1, 1, 200, 200 + K - 1, 200, 0] and len(m.links) == 2 and m.records()["info"][0] == 1 | 1 << 4 | 1 << 8
    m = check_hand(pkg, uu.merged(uu.cycle_graph(K, 200, 11), bu.hand_graph([rnd(12, 70 + K - 1)], K)), K, "a cycle beside a path of 70")
    assert m.info[:4] == [270, 2, 2, 1] and sorted(len(t["counts"]) for t in m.unitigs) == [70, 200]
    m = check_hand(pkg, uu.merged(uu.cycle_graph(K, 200, 11), uu.cycle_graph(K, 61, 13)), K, "two cycles")
    assert m.info[:4] == [261, 0, 2, 2] and len(m.links) == 4
    # the worst case of the early exit: the keys ascend along the walk (A..A, A..AC, A..ACA, ...), so every node walks to the end of the
    # cycle before it meets a smaller key
    c = np.zeros(K + 1, dtype=np.uint8)
    c[-1] = 1
    nodes = bu.hand_graph([np.concatenate([c, c[:K]])], K)
    m = check_hand(pkg, nodes, K, "a cycle whose keys ascend")
    words = m.unitigs[0]["words"]
    assert m.info[:4] == [K + 1, 0, 1, 1] and words == sorted(words) and words[0] == 0 and all(w <= cu.rc_int(w, K) for w in words)


def test_what_splits_a_unitig(pkg):
    K = K23
    path = rnd(21, 70 + K - 1)
    base = bu.hand_graph([path], K)
    fw, cn = cu.kmer_ints(path, K)
    mid = 30
    assert check_hand(pkg, base, K, "a path of 70").info[:3] == [70, 2, 1]
    g1 = {k: list(v) for k, v in base.items()}
    g1[cn[mid]][2] = 1
    m = check_hand(pkg, g1, K, "a deleted node in mid-path")
    assert m.info[:3] == [69, 4, 2] and sorted(len(t["counts"]) for t in m.unitigs) == [30, 39] and m.links == []
    g2 = {k: list(v) for k, v in base.items()}
    g2[cn[mid]][1] = 100
    m = check_hand(pkg, g2, K, "a node above max_count in mid-path", max_count=50)
    assert m.info[:3] == [69, 4, 2] and m.links == []
    assert check_hand(pkg, g2, K, "the same without an upper bound").info[:3] == [70, 2, 1]
    # a link counter below min_link, at both of its ends: two unitigs and nothing between them
    x, y = fw[mid], fw[mid + 1]
    g3 = {k: list(v) for k, v in base.items()}
    bu.set_link(g3, x, y & 3, 1, K)
    bu.set_link(g3, cu.rc_int(y, K), (x >> 2 * (K - 1) & 3) ^ 2, 1, K)
    m = check_hand(pkg, g3, K, "a link below min_link in mid-path", min_link=2)
    assert m.info[:3] == [70, 4, 2] and m.links == [] and m.dangling == 0
    assert check_hand(pkg, g3, K, "the same at min_link 1").info[:3] == [70, 2, 1]
    # one end of that link zeroed: no join from either side, two unitigs.  By the rule the link is still given from the end that has
    # it -- its target begins a unitig -- and from that end only
    g4 = {k: list(v) for k, v in base.items()}
    bu.set_link(g4, cu.rc_int(y, K), (x >> 2 * (K - 1) & 3) ^ 2, 0, K)
    m = check_hand(pkg, g4, K, "one end of a mid-path link zeroed")
    assert m.info[:3] == [70, 4, 2] and len(m.links) == 1 and m.dangling == 0
    # a counter that points into the middle of a unitig from a node that the unitig does not know: that link end dangles
    stray = np.concatenate([[(path[mid - 1] + 1) & 3], path[mid:mid + K - 1]]).astype(np.uint8)
    g5 = uu.merged(base, bu.hand_graph([stray], K))
    s = cu.kmer_ints(stray, K)[0][0]
    bu.set_link(g5, s, fw[mid] & 3, 5, K)
    m = check_hand(pkg, g5, K, "a dangling link end")
    assert m.info[:3] == [71, 4, 2] and m.links == [] and m.dangling == 1 and sorted(m.dangling_of) == [0, 1]


# ---- 4. geometry ---------------------------------------------------------------------------------------------------------------------------------
def test_many_starts_and_a_single_one(pkg):
    """the 2 000-site graph of the bubble tests: thousands of start words, whole wavefronts walk, more than one chunk of the list; and
    one path of 20 000 nodes in an otherwise empty table: two start words, one lane walks"""
    K, n = K23, 2000
    rng = np.random.default_rng(77)
    gap = 2 * K + 5
    ref = rng.integers(0, 4, size=gap * (n + 1), dtype=np.uint8)
    alt = ref.copy()
    alt[gap::gap] = (alt[gap::gap] + 1) & 3
    alt = alt[:gap * n + K + 3]
    m = check_hand(pkg, bu.hand_graph([ref, alt], K), K, "2 000 sites")
    assert m.info[2] == 3 * n + 1 and m.info[1] == 2 * m.info[2] > 4 * 256 and m.dangling == 0
    lone = rng.integers(0, 4, size=20000 + K - 1, dtype=np.uint8)
    m = check_hand(pkg, bu.hand_graph([lone], K), K, "one path of 20 000 nodes")
    assert m.info == [20000, 2, 1, 0, 20000, 20000 + K - 1, 20000, 0]


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
import unitig_util as uu
from test_unitigs import imported, many_short_paths, whole_list
nodes = many_short_paths()
with imported(pkg, nodes, 23) as g:
    info = g.unitigs_begin(uu.DEFAULTS)
    slots = g.table_slots()
    got = whole_list(g, info)
np.savez({path!r}, slots=slots, info=info, keys=np.array(got[1], dtype=np.uint64), rec=np.array(got[2], dtype=np.uint64), bases=np.frombuffer(got[3], dtype=np.uint8),
         links=np.array(got[5], dtype=np.uint32), dangling=got[6])
"""
SHORT_PATHS = 9000


def many_short_paths():
    rng = np.random.default_rng(99)
    return bu.hand_graph([rng.integers(0, 4, size=K23 + 2, dtype=np.uint8) for _ in range(SHORT_PATHS)], K23)


def test_more_starts_than_the_first_guess(pkg, tmp_path):
    """isolated 3-node paths, and every scan in ONE workgroup (test hook, so in a child process): the start words pass the first guess
    of the list -- one per 16 slots, 4 096 and a chunk per wavefront -- and the scan runs a second time with the room it asked for"""
    nodes = many_short_paths()
    model = uu.Unitigs(bu.as_model_nodes(nodes), K23, **uu.DEFAULTS)
    assert model.info[:4] == [3 * SHORT_PATHS, 2 * SHORT_PATHS, SHORT_PATHS, 0] and model.links == []
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SCAN_BLOCKS="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    first_guess = ((int(got["slots"]) // 16 + 4096) // 192 + 1 + 4) * 256
    assert 2 * SHORT_PATHS > first_guess, (int(got["slots"]), first_guess)
    assert got["info"].tolist() == model.info
    assert got["keys"].tolist() == model.keys(1).tolist()
    assert [tuple(r) for r in got["rec"].tolist()] == [tuple(int(x) for x in r) for r in model.records().tolist()]
    assert got["bases"].tobytes() == model.seqs()[0].tobytes() and len(got["links"]) == 0 and int(got["dangling"]) == 0


# ---- 5. cross-checks on the device alone -----------------------------------------------------------------------------------------------------
def test_cross_checks_on_the_device(pkg, synth):
    """nothing here comes from the model: the sequences hold the live keys of the table once each; every bubble side of the same
    context is one unitig; the live nodes are the clustering's; the sequences of every link overlap in K - 1 bases"""
    K = 31
    case = bu.built_case(K)
    prm = dict(min_count=1, max_count=0, min_link=1)
    letters = np.frombuffer(cu.LETTERS.encode(), dtype=np.uint8)
    with counted_case(pkg, synth, case) as g:
        info = g.unitigs_begin(prm)
        n = int(info[2])
        keys, rec = g.unitigs_fetch(0, n)
        bases, offs = g.unitigs_seqs(0, n)
        links, dangling = g.unitigs_links(0, n)
        seqs = [bases[int(a):int(b)] for a, b in zip(offs, offs[1:])]
        assert [len(s) for s in seqs] == (rec["nodes"] + K - 1).tolist() and int(info[4]) == int(info[0]) == int(rec["nodes"].sum())
        kmers = sorted(c for s in seqs for c in cu.kmer_ints(s, K)[1])
        ekeys, _, _, ecnt = g.export_nodes()[:4]
        assert kmers == sorted(cu.key_int(k) for k, c in zip(ekeys.tolist(), ecnt.tolist()) if c >= 1)
        assert int(g.cluster_begin(prm)[0]) == int(info[0])
        # the bubbles of the same context, at the same rule
        binfo = g.bubbles_begin(dict(prm, max_len=4000))
        bkeys, brec = g.bubbles_fetch(0, int(binfo[4]))
        first = {cu.key_int(k[0]): i for i, k in enumerate(keys.tolist())}
        rlast = {cu.rc_int(cu.key_int(k[1]), K): i for i, k in enumerate(keys.tolist())}
        sides = 0
        for bk, br in zip(bkeys.tolist(), brec):
            s = cu.key_int(bk[0])
            for tag, base in (("a", int(br["info"]) & 3), ("b", int(br["info"]) >> 2 & 3)):
                if br["len_" + tag] == 0:
                    continue
                y = ((s << 2) | base) & ((1 << (2 * K)) - 1)
                u = rec[first[y] if y in first else rlast[y]]
                assert (u["nodes"], u["min"], u["sum"]) == (br["len_" + tag], br["min_" + tag], br["sum_" + tag])
                sides += 1
        assert sides == 17 and int(binfo[4]) == 9
        # the links: K - 1 bases of overlap in the stated orientations, then the base of the link
        text = lambda i, o: (letters[seqs[i]] if o == 0 else letters[(seqs[i][::-1] ^ 2)]).tobytes()
        assert len(links) == 62 and dangling == 0
        for l in links:
            o, o2, b = int(l["info"]) & 1, int(l["info"]) >> 1 & 1, int(l["info"]) >> 2 & 3
            a, c = text(int(l["from"]), o), text(int(l["to"]), o2)
            assert a[-(K - 1):] == c[:K - 1] and c[K - 1:K] == cu.LETTERS[b].encode()
        # the clustering and the bubble list are still what they were
        assert len(g.bubbles_fetch(0, 9)[1]) == 9 and len(g.cluster_components()[1]) > 0
        assert whole_list(g, info) == (info.tolist(), keys.tolist(), rec.tolist(), bases.tobytes(), offs.tolist(), links.tolist(), dangling)


# ---- 6. fetch, seqs and links in ranges ---------------------------------------------------------------------------------------------------------
def test_ranges(pkg, synth):
    case = bu.built_case(31)
    model = uu.Unitigs(case["nodes"], 31, **uu.DEFAULTS)
    n = len(model.unitigs)
    with counted_case(pkg, synth, case) as g:
        assert int(g.unitigs_begin(uu.DEFAULTS)[2]) == n == 36
        keys, rec = g.unitigs_fetch(0, n)
        bases, offs = g.unitigs_seqs(0, n)
        links, dangling = g.unitigs_links(0, n)
        for cuts in (list(range(n + 1)), [0, 3, 4, 20, n], [0, n], [0, 0, 5, 5, n]):
            parts = [(g.unitigs_fetch(a, b - a), g.unitigs_seqs(a, b - a), g.unitigs_links(a, b - a)) for a, b in zip(cuts, cuts[1:])]
            assert np.concatenate([p[0][0] for p in parts]).tolist() == keys.tolist()
            assert np.concatenate([p[0][1] for p in parts]).tolist() == rec.tolist()
            assert b"".join(p[1][0].tobytes() for p in parts) == bases.tobytes()
            assert np.concatenate([p[2][0] for p in parts]).tolist() == links.tolist() and sum(p[2][1] for p in parts) == dangling
            for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
                assert p[1][1].tolist() == model.seqs(a, b - a)[1].tolist()
                assert p[2][0].tolist() == model.link_records(a, b - a)[0].tolist()
        # either array may be NULL
        k2 = np.zeros((n, 2, 1), dtype=np.uint64)
        g._check(g.lib.sdt_gpu_unitigs_fetch(g._ctx, 0, n, pkg._ptr(k2), None))
        r2 = np.zeros(n, dtype=pkg.UNITIG_DTYPE)
        g._check(g.lib.sdt_gpu_unitigs_fetch(g._ctx, 0, n, None, pkg._ptr(r2)))
        assert k2.tolist() == keys.tolist() and r2.tolist() == rec.tolist()
        # the offsets only; too little room: the offsets and no base
        o2 = np.zeros(n + 1, dtype=np.uint64)
        g._check(g.lib.sdt_gpu_unitigs_seqs(g._ctx, 0, n, None, 0, pkg._ptr(o2)))
        assert o2.tolist() == offs.tolist() and int(offs[-1]) == model.info[5]
        with pytest.raises(pkg.SdtError) as e:
            g.unitigs_seqs(2, 5, capacity=int(offs[7] - offs[2]) - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.offsets.tolist() == (offs[2:8] - offs[2]).tolist()
        preset = np.full(64, 0xAB, dtype=np.uint8)
        o3 = np.zeros(n + 1, dtype=np.uint64)
        assert g.lib.sdt_gpu_unitigs_seqs(g._ctx, 0, n, pkg._ptr(preset), 64, pkg._ptr(o3)) == pkg.SDT_EFULL
        assert (preset == 0xAB).all() and o3.tolist() == offs.tolist()
        # the number of links only; too little room: the number and no record
        nl, nd = ctypes.c_uint64(7), ctypes.c_uint64(7)
        g._check(g.lib.sdt_gpu_unitigs_links(g._ctx, 0, n, None, 0, ctypes.byref(nl), ctypes.byref(nd)))
        assert (nl.value, nd.value) == (len(links), 0) and len(links) == 50
        with pytest.raises(pkg.SdtError) as e:
            g.unitigs_links(0, n, capacity=len(links) - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.n_links == len(links)
        room = np.full(8, 0xABABABAB, dtype=np.uint32).view(pkg.UNITIG_LINK_DTYPE)
        nl = ctypes.c_uint64(0)
        assert g.lib.sdt_gpu_unitigs_links(g._ctx, 0, n, pkg._ptr(room), 2, ctypes.byref(nl), None) == pkg.SDT_EFULL
        assert nl.value == len(links) and (room.view(np.uint32) == 0xABABABAB).all()
        # past the end; nothing asked for
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_fetch(n - 4, 5), "sdt_gpu_unitigs_fetch")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_seqs(n, 1), "sdt_gpu_unitigs_seqs")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_links(n + 1, 1), "sdt_gpu_unitigs_links")
        assert g.lib.sdt_gpu_unitigs_fetch(g._ctx, 99, 0, None, None) == pkg.SDT_OK
        assert g.lib.sdt_gpu_unitigs_seqs(g._ctx, 99, 0, None, 0, None) == pkg.SDT_OK
        assert g.lib.sdt_gpu_unitigs_links(g._ctx, 99, 0, None, 0, None, None) == pkg.SDT_OK


# ---- 7. state -------------------------------------------------------------------------------------------------------------------------------------
def test_state(pkg, synth):
    case = bu.built_case(31)
    K = 31
    model, model1 = uu.Unitigs(case["nodes"], K, **uu.DEFAULTS), uu.Unitigs(case["nodes"], K, **dict(uu.DEFAULTS, min_count=1))
    codes, offs = case["reads"]
    words = synth.pack_2bit(codes)
    changed = "the table changed since sdt_gpu_unitigs_begin"
    calls = lambda g: (lambda: g.unitigs_fetch(0, 1), lambda: g.unitigs_seqs(0, 1), lambda: g.unitigs_links(0, 1))
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(words, offs)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.unitigs_begin(), "sdt_gpu_unitigs_begin", "sdt_gpu_finish_count")
        g.finish_count()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, "sdt_gpu_unitigs_begin first")
        g.unitigs_end()                                                        # (nothing to free: fine)
        # a second begin replaces the first
        assert int(g.unitigs_begin(dict(uu.DEFAULTS, min_count=1))[2]) == 41
        uu.assert_unitigs_equal(g, model, g.unitigs_begin(uu.DEFAULTS), "second begin")
        # a clustering, a bubble list and an assembly tally stay valid across a unitigs_begin, and the other way round
        cinfo = g.cluster_begin()
        ckeys = g.cluster_components()[0].tolist()
        binfo = g.bubbles_begin(bu.DEFAULTS)
        g.asm_begin()
        g.asm_add(words, offs, records=False)
        spectrum = g.asm_spectrum()
        uu.assert_unitigs_equal(g, model1, g.unitigs_begin(dict(uu.DEFAULTS, min_count=1)), "beside a clustering, a bubble list and a tally")
        assert g.cluster_components()[0].tolist() == ckeys and int(g.cluster_begin()[2]) == int(cinfo[2])
        bu.assert_bubbles_equal(g, case["model"], binfo, "the bubble list across a unitigs_begin")
        assert all((a == b).all() for a, b in zip(spectrum, g.asm_spectrum()))
        g.bubbles_begin(bu.DEFAULTS)
        uu.assert_unitigs_equal(g, model1, np.array(model1.info, dtype=np.uint64), "the unitig list across a bubbles_begin and a cluster_begin")
        g.asm_end()
        g.cluster_end()
        g.bubbles_end()
        assert len(g.unitigs_fetch(0, 41)[1]) == 41
        # the table changes: delow; more reads; reset
        g.delow(1)
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, changed)
        g.unitigs_begin(uu.DEFAULTS)
        g.push_reads(words, offs[:41])
        g.finish_count()
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, changed)
        g.unitigs_begin(uu.DEFAULTS)
        g.reset()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.unitigs_seqs(0, 1), changed)
        g.push_reads(words, offs)
        g.finish_count()
        g.unitigs_begin(uu.DEFAULTS)
        assert len(g.unitigs_fetch(0, 1)[1]) == 1
        # end, then a fetch
        g.unitigs_end()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.unitigs_fetch(0, 1), "sdt_gpu_unitigs_begin first")
        g.unitigs_begin()
        g.release_table()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.unitigs_begin(), "sdt_gpu_unitigs_begin", "released")
    # a graph phase
    with counted_case(pkg, synth, case, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        assert int(g.unitigs_begin(uu.DEFAULTS)[2]) == 36
        g.mark_and_hist()
        g.layout_on_device(4, 1)
        for call in calls(g):
            raises(pkg, pkg.SDT_ESTATE, call, changed)
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:                        # a context with a communicator holds one shard
        g.comm_init_shm(f"sdt_unitigs_{os.getpid()}", 0, 1)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.unitigs_begin(), "sdt_gpu_unitigs_begin", "shard")
    # a context destroyed with a list open frees it
    with counted_case(pkg, synth, case) as g:
        g.unitigs_begin()


def test_the_table_is_untouched(pkg, synth):
    case = bu.built_case(31)

    def snapshot(g):
        keys, l, rf, cnt = g.export_nodes()[:4]
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt)]

    with counted_case(pkg, synth, case) as g:
        before = snapshot(g)
        uu.assert_unitigs_equal(g, uu.Unitigs(case["nodes"], 31, **uu.DEFAULTS), g.unitigs_begin(uu.DEFAULTS), "between two snapshots")
        for a, b in zip(before, snapshot(g)):
            assert a.shape == b.shape and (a == b).all()


# ---- 8. the parameters ---------------------------------------------------------------------------------------------------------------------------------
def test_parameters_are_refused_before_any_launch(pkg, synth):
    case = bu.built_case(31)
    with counted_case(pkg, synth, case) as g:
        launches = g.kernel_time(reset=False)[1]
        bad = [(dict(flags=1), "flags", "0x1"), (dict(min_link=0), "min_link", "0"), (dict(min_link=64), "min_link", "64"),
               (dict(min_count=5, max_count=4), "max_count", "4")]
        for prm, field, value in bad:
            raises(pkg, pkg.SDT_EINVAL, lambda: g.unitigs_begin(prm), f"sdt_unitig_params.{field}", value)
        assert g.lib.sdt_gpu_unitigs_begin(g._ctx, None, None) == pkg.SDT_EINVAL
        for call in (lambda: g.unitigs_fetch(0, 1), lambda: g.unitigs_links(0, 1)):
            raises(pkg, pkg.SDT_ESTATE, call, "sdt_gpu_unitigs_begin first")       # (a refused begin begins nothing)
        assert g.kernel_time(reset=False)[1] == launches
        assert int(g.unitigs_begin(dict(min_count=0, max_count=1))[0]) >= 0    # (min_count 0 is 1: max_count 1 is allowed)
        assert g.kernel_time(reset=False)[1] > launches
