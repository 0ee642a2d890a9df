"""GPU (-m gpu): the bubbles of the counted k-mer graph (sdt_gpu_bubbles_*) against the Python restatement of the rule (bubble_util.py):
info, records, source and sink words and paths, all exact.  The nodes of the model come from the oracle or are written by hand, never
from the library."""
import os

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu

pytestmark = pytest.mark.gpu


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


# ---- 1. the model, per key width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(23, 0), (31, 1), (31, 2), (47, 0), (63, 0), (95, 0), (127, 0), (33, 0), (65, 0), (97, 0)])
def test_bubbles_equal_the_model(pkg, synth, K, flags):
    """1, 2 and 4 key words, both pass-1 kernel families at K = 31; min_count 2 and 1, max_len at the longest side and one below"""
    case = bu.built_case(K)
    with counted_case(pkg, synth, case, flags=flags) as g:
        assert g.nw == (1 if K <= 31 else 2 if K <= 63 else 4)
        bu.assert_bubbles_equal(g, case["model"], g.bubbles_begin(bu.DEFAULTS), f"K={K} flags={flags}")
        bu.assert_bubbles_equal(g, case["model1"], g.bubbles_begin(dict(bu.DEFAULTS, min_count=1)), f"K={K} flags={flags} min_count=1")
        for max_len, n in ((case["longest"], 8), (case["longest"] - 1, 7)):
            prm = dict(bu.DEFAULTS, max_len=max_len)
            info = g.bubbles_begin(prm)
            assert int(info[4]) == n
            bu.assert_bubbles_equal(g, bu.Bubbles(case["nodes"], K, **prm), info, f"K={K} max_len={max_len}")
        g.bubbles_end()


# ---- 2. the list does not depend on the layout ---------------------------------------------------------------------------------------------
def test_layout_independence(pkg, synth):
    case = bu.built_case(31)
    got, slots = [], []
    for est, flags in ((1 << 16, 0), (1 << 20, 0), (1 << 16, pkg.SDT_FLAG_DIRECT)):
        with counted_case(pkg, synth, case, flags=flags, est_distinct=est) as g:
            slots.append(g.table_slots())
            info = g.bubbles_begin(bu.DEFAULTS)
            bu.assert_bubbles_equal(g, case["model"], info, f"est_distinct={est} flags={flags}")
            keys, rec = g.bubbles_fetch(0, int(info[4]))
            bases, offs = g.bubbles_paths(0, int(info[4]))
            got.append((info.tolist(), keys.tolist(), rec.tolist(), bases.tolist(), offs.tolist()))
    assert slots[0] != slots[1]
    assert got[0] == got[1] == got[2]


# ---- 3. graphs written by hand -----------------------------------------------------------------------------------------------------------------
def site_graph(K, seed, alleles=2, **kw):
    """`alleles` sequences that differ at one site -> (nodes, ref, the site, s: the k-mer in front of it, the bases there)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=3 * K + 10, dtype=np.uint8)
    at = K + 5
    seqs = [ref] + [np.concatenate([ref[:at], [(ref[at] + k) & 3], ref[at + 1:]]).astype(np.uint8) for k in range(1, alleles)]
    return bu.hand_graph(seqs, K, **kw), seqs, at, cu.kmer_ints(ref[at - K:at], K)[0][0]


def check_hand(pkg, nodes, K, what, **params):
    prm = dict(bu.DEFAULTS, **params)
    model = bu.Bubbles(bu.as_model_nodes(nodes), K, **prm)
    with imported(pkg, nodes, K) as g:
        bu.assert_bubbles_equal(g, model, g.bubbles_begin(prm), what)
    return model


def test_hand_built_graphs(pkg):
    K = 23
    nodes, seqs, at, s = site_graph(K, 1)
    alt_b = int(seqs[1][at])
    assert len(check_hand(pkg, nodes, K, "one site").bubbles) == 1
    # a fork whose branch counter is below min_link
    g1 = {k: list(v) for k, v in nodes.items()}
    bu.set_link(g1, s, alt_b, 1, K)
    assert len(check_hand(pkg, g1, K, "a branch counter below min_link", min_link=2).found) == 0
    assert len(check_hand(pkg, g1, K, "the same at min_link 1").bubbles) == 1
    # an inner node with the deleted flag set; a node above max_count in the middle of a side
    inner = cu.kmer_ints(seqs[1][at - 5:at - 5 + K], K)[1][0]
    g2 = {k: list(v) for k, v in nodes.items()}
    g2[inner][2] = 1
    assert len(check_hand(pkg, g2, K, "a deleted inner node").found) == 0
    g3 = {k: list(v) for k, v in nodes.items()}
    g3[inner][1] = 100
    assert len(check_hand(pkg, g3, K, "an inner node above max_count", max_count=50).found) == 0
    assert len(check_hand(pkg, g3, K, "the same without an upper bound").bubbles) == 1
    # counters that disagree between the two ends of a link: the first node of the alternative side does not know its predecessor, so
    # the bubble is seen from s and not from the other end
    g4 = {k: list(v) for k, v in nodes.items()}
    y = ((s << 2) | alt_b) & ((1 << (2 * K)) - 1)
    bu.set_link(g4, cu.rc_int(y, K), (s >> (2 * (K - 1)) & 3) ^ 2, 0, K)
    assert len(check_hand(pkg, g4, K, "counters that disagree").found) == 1
    # a saturated counter
    g5, _, _, _ = site_graph(K, 1, link=63)
    m5 = check_hand(pkg, g5, K, "saturated counters", min_link=63)
    assert len(m5.bubbles) == 1 and int(m5.records()["info"][0]) >> 8 == 63 | 63 << 8
    # a 4-way fork of which three meet
    g6, seqs6, at6, s6 = site_graph(K, 2, alleles=3)
    rng = np.random.default_rng(3)
    stray = np.concatenate([seqs6[0][:at6], [(seqs6[0][at6] + 3) & 3], rng.integers(0, 4, size=2 * K, dtype=np.uint8)]).astype(np.uint8)
    for k, v in bu.hand_graph([stray], K).items():
        if k in g6:
            g6[k][0] |= v[0]
        else:
            g6[k] = v
    m6 = check_hand(pkg, g6, K, "a 4-way fork")
    assert len(m6.bubbles) == 3 and len(m6.succ(s6, cu.rc_int(s6, K))) == 4 and m6.info[2] == 4 + 3
    # s equal to the sink: two loops through one k-mer
    S = rng.integers(0, 4, size=K, dtype=np.uint8)
    xa, xb = rng.integers(0, 4, size=30, dtype=np.uint8), rng.integers(0, 4, size=30, dtype=np.uint8)
    xb[0], xb[-1] = (xa[0] + 1) & 3, (xa[-1] + 1) & 3
    g7 = bu.hand_graph([np.concatenate([S, x, S]) for x in (xa, xb)], K)
    m7 = check_hand(pkg, g7, K, "s equal to the sink")
    assert len(m7.bubbles) == 1 and m7.bubbles[0][0] == m7.bubbles[0][3] and m7.records()["len_a"][0] == 30 + K - 1


def test_even_k_has_no_device_table(pkg):
    """the palindromic source of the rule (K = 24) exists on the model only (test_bubbles_host.py): a context takes odd K alone, as the
    reference does, so no table on the device holds a k-mer that is its own reverse complement"""
    nodes, s = bu.palindrome_graph()
    assert cu.rc_int(s, 24) == s and s in nodes
    with pytest.raises(pkg.SdtError) as e:
        pkg.PregraphGPU(24, est_distinct=1 << 12)
    assert e.value.code == pkg.SDT_EINVAL and "odd" in str(e.value)


# ---- 4. geometry ---------------------------------------------------------------------------------------------------------------------------------
def test_many_forks_and_a_lonely_one(pkg, synth):
    """about 2 000 substitutions 2 K + 5 apart: the forks fill whole wavefronts, every lane walks; and one fork in an
    otherwise linear table, where most lanes have nothing to do"""
    K, n = 23, 2000
    rng = np.random.default_rng(77)
    gap = 2 * K + 5
    ref = rng.integers(0, 4, size=gap * (n + 1), dtype=np.uint8)
    alt = ref.copy()
    alt[gap::gap] = (alt[gap::gap] + 1) & 3
    alt = alt[:gap * n + K + 3]                               # (the last site keeps K + 2 bases behind it)
    nodes = bu.hand_graph([ref, alt], K)
    model = check_hand(pkg, nodes, K, "2 000 sites")
    assert model.info[4] == n and model.info[1] == 2 * n and model.info[6] == K
    lone = rng.integers(0, 4, size=20000, dtype=np.uint8)
    nodes = bu.hand_graph([lone, cu.substituted(lone, 9000)], K)
    model = check_hand(pkg, nodes, K, "a lonely fork")
    assert model.info[4] == 1 and model.info[0] > 19900


# ---- 5. fetch and paths in ranges -------------------------------------------------------------------------------------------------------------------
def test_ranges(pkg, synth):
    case = bu.built_case(31)
    model = case["model1"]
    n = len(model.bubbles)
    with counted_case(pkg, synth, case) as g:
        assert int(g.bubbles_begin(dict(bu.DEFAULTS, min_count=1))[4]) == n == 9
        keys, rec = g.bubbles_fetch(0, n)
        bases, offs = g.bubbles_paths(0, n)
        for cuts in ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 3, 4, 9], [0, 9], [0, 0, 5, 5, 9]):
            parts = [(g.bubbles_fetch(a, b - a), g.bubbles_paths(a, b - a)) for a, b in zip(cuts, cuts[1:])]
            assert np.concatenate([p[0][0] for p in parts]).tolist() == keys.tolist()
            assert np.concatenate([p[0][1] for p in parts]).tolist() == rec.tolist()
            assert b"".join(p[1][0].tobytes() for p in parts) == bases.tobytes()
            for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
                assert p[1][1].tolist() == model.paths(a, b - a)[1].tolist()
        # either array may be NULL
        k2 = np.zeros((n, 2, 1), dtype=np.uint64)
        g._check(g.lib.sdt_gpu_bubbles_fetch(g._ctx, 0, n, pkg._ptr(k2), None))
        r2 = np.zeros(n, dtype=pkg.BUBBLE_DTYPE)
        g._check(g.lib.sdt_gpu_bubbles_fetch(g._ctx, 0, n, None, pkg._ptr(r2)))
        assert k2.tolist() == keys.tolist() and r2.tolist() == rec.tolist()
        # the offsets only; too little room: the offsets and no base
        o2 = np.zeros(2 * n + 1, dtype=np.uint64)
        g._check(g.lib.sdt_gpu_bubbles_paths(g._ctx, 0, n, None, 0, pkg._ptr(o2)))
        assert o2.tolist() == offs.tolist() and int(offs[-1]) == model.info[5]
        with pytest.raises(pkg.SdtError) as e:
            g.bubbles_paths(2, 5, capacity=int(offs[14] - offs[4]) - 1)
        assert e.value.code == pkg.SDT_EFULL and e.value.offsets.tolist() == (offs[4:15] - offs[4]).tolist()
        preset = np.full(64, 0xAB, dtype=np.uint8)
        o3 = np.zeros(2 * n + 1, dtype=np.uint64)
        assert g.lib.sdt_gpu_bubbles_paths(g._ctx, 0, n, pkg._ptr(preset), 64, pkg._ptr(o3)) == pkg.SDT_EFULL
        assert (preset == 0xAB).all() and o3.tolist() == offs.tolist()
        # past the end; nothing asked for
        raises(pkg, pkg.SDT_EINVAL, lambda: g.bubbles_fetch(5, 5), "sdt_gpu_bubbles_fetch")
        raises(pkg, pkg.SDT_EINVAL, lambda: g.bubbles_paths(n, 1), "sdt_gpu_bubbles_paths")
        assert g.lib.sdt_gpu_bubbles_fetch(g._ctx, 99, 0, None, None) == pkg.SDT_OK
        assert g.lib.sdt_gpu_bubbles_paths(g._ctx, 99, 0, None, 0, None) == pkg.SDT_OK


# ---- 6. state -------------------------------------------------------------------------------------------------------------------------------------
def test_state(pkg, synth):
    case = bu.built_case(31)
    K, model = 31, case["model"]
    codes, offs = case["reads"]
    words = synth.pack_2bit(codes)
    changed = "the table changed since sdt_gpu_bubbles_begin"
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(words, offs)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_begin(), "sdt_gpu_bubbles_begin", "sdt_gpu_finish_count")
        g.finish_count()
        for call in (lambda: g.bubbles_fetch(0, 1), lambda: g.bubbles_paths(0, 1)):
            raises(pkg, pkg.SDT_ESTATE, call, "sdt_gpu_bubbles_begin first")
        g.bubbles_end()                                                        # (nothing to free: fine)
        # a second begin replaces the first
        assert int(g.bubbles_begin(dict(bu.DEFAULTS, min_count=1))[4]) == 9
        bu.assert_bubbles_equal(g, model, g.bubbles_begin(bu.DEFAULTS), "second begin")
        # the clustering and the assembly tally stay valid across a bubbles_begin, and the other way round
        cinfo = g.cluster_begin()
        ckeys = g.cluster_components()[0].tolist()
        g.asm_begin()
        g.asm_add(words, offs, records=False)
        spectrum = g.asm_spectrum()
        bu.assert_bubbles_equal(g, model, g.bubbles_begin(bu.DEFAULTS), "beside a clustering and a tally")
        assert g.cluster_components()[0].tolist() == ckeys and int(g.cluster_begin()[2]) == int(cinfo[2])
        assert all((a == b).all() for a, b in zip(spectrum, g.asm_spectrum()))
        g.asm_end()
        g.cluster_end()
        assert len(g.bubbles_fetch(0, 8)[1]) == 8 and len(g.bubbles_paths(0, 8)[0]) == model.info[5]
        # the table changes: delow; more reads; reset
        g.delow(1)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_fetch(0, 1), changed)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_paths(0, 1), changed)
        g.bubbles_begin(bu.DEFAULTS)
        g.push_reads(words, offs[:41])
        g.finish_count()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_fetch(0, 1), changed)
        g.bubbles_begin(bu.DEFAULTS)
        g.reset()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_paths(0, 1), changed)
        g.push_reads(words, offs)
        g.finish_count()
        g.bubbles_begin(bu.DEFAULTS)
        assert len(g.bubbles_fetch(0, 1)[1]) == 1
        # end, then a fetch
        g.bubbles_end()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_fetch(0, 1), "sdt_gpu_bubbles_begin first")
        g.bubbles_begin()
        g.release_table()
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_begin(), "sdt_gpu_bubbles_begin", "released")
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:                        # a context with a communicator holds one shard
        g.comm_init_shm(f"sdt_bubbles_{os.getpid()}", 0, 1)
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_begin(), "sdt_gpu_bubbles_begin", "shard")
    # a context destroyed with a list open frees it
    with counted_case(pkg, synth, case) as g:
        g.bubbles_begin()


def test_the_table_is_untouched(pkg, synth):
    case = bu.built_case(31)

    def snapshot(g):
        keys, l, rf, cnt = g.export_nodes()[:4]
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt)]

    with counted_case(pkg, synth, case) as g:
        before = snapshot(g)
        bu.assert_bubbles_equal(g, case["model"], g.bubbles_begin(bu.DEFAULTS), "between two snapshots")
        for a, b in zip(before, snapshot(g)):
            assert a.shape == b.shape and (a == b).all()


# ---- 7. the parameters ---------------------------------------------------------------------------------------------------------------------------------
def test_parameters_are_refused_before_any_launch(pkg, synth):
    case = bu.built_case(31)
    with counted_case(pkg, synth, case) as g:
        launches = g.kernel_time(reset=False)[1]
        bad = [(dict(flags=1), "flags", "0x1"), (dict(reserved=7), "reserved", "7"), (dict(min_link=0), "min_link", "0"), (dict(min_link=64), "min_link", "64"),
               (dict(min_count=5, max_count=4), "max_count", "4"), (dict(min_count=0, max_count=0, max_len=0), "max_len", "0"),
               (dict(max_len=(1 << 20) + 1), "max_len", str((1 << 20) + 1))]
        for prm, field, value in bad:
            raises(pkg, pkg.SDT_EINVAL, lambda: g.bubbles_begin(prm), f"sdt_bubble_params.{field}", value)
        assert g.lib.sdt_gpu_bubbles_begin(g._ctx, None, None) == pkg.SDT_EINVAL
        raises(pkg, pkg.SDT_ESTATE, lambda: g.bubbles_fetch(0, 1), "sdt_gpu_bubbles_begin first")       # (a refused begin begins nothing)
        assert g.kernel_time(reset=False)[1] == launches
        assert int(g.bubbles_begin(dict(min_count=0, max_count=1, max_len=1 << 20))[0]) >= 0       # (min_count 0 is 1: max_count 1 is allowed)
        assert g.kernel_time(reset=False)[1] > launches
