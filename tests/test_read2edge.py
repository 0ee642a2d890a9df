"""GPU (-m gpu): the second read pass at the ABI -- sdt_gpu_load_paths / map_reads / export_arcs / export_paths / import_paths /
keep_reads -- against the oracle's sdto_read2edge (pinned byte for byte to the reference's *.preArc, tests/test_oracle_vs_reference.py)
on node states of the tests' own making (tests/read2edge_util.py; the harness is checked on the CPU in test_read2edge_oracle.py).

Every node gets a random class and label, ~30 % of the (K+1)-mers the reads ask for are missing from the patch table: the branches
of k_map_reads that a graph of our own edge builder hardly ever reaches -- an unresolved item in mid-path, a reset that leaves
is_prev set so that two k-mers that are not adjacent form a (K+1)-mer, id + twin - 1 == 0, runs of one id cut by a vertex, reads of
K + 1 bases -- are taken hundreds of times per case.  All comparisons are exact.

Cases of (a): the issue asks for K in {21, 31, 47, 63, 65, 95, 127} x L in {100, 250}.  (95, 100) and (127, 100) cannot be had: reads
come from sample_reads(read_len=L, ragged=True), so at L = 100 no read holds a 127-mer and some 6 % hold one to five 95-mers -- fewer
than the 1 000 arcs the case has to show under any seed.  Those two K run at L = 250 only.

test_pass2_states_and_errors, what a failed load_paths leaves behind: the counter of keys that were not found used to stay set on
the device, and every later call that looks at the counters -- a correct load_paths included -- failed with it.  That is a
poisoned context for a caller's mistake that the call has already reported, so load_paths now clears the counter it raised and the
test asserts the recovery: a correct load_paths succeeds and map_reads gives the oracle's arcs."""
import numpy as np
import pytest

import read2edge_util as ru

pytestmark = pytest.mark.gpu

CASES = [(K, L) for K in (21, 31, 47, 63, 65, 95, 127) for L in (100, 250) if (K, L) not in ((95, 100), (127, 100))]
# the first K of the 2- and of the 4-word keys (65 is above): the top base of a K-mer at bit 0 of a key word.  (97, 100) cannot be had
# for the reason (95, 100) cannot
CASES += [(33, 100), (33, 250), (97, 250)]
SEED = {}                # (K, L, E) -> seed, where the default (100 K + L) does not meet the preconditions

_scenarios = {}


@pytest.fixture(scope="module")
def scen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("read2edge")


def scenario(synth, scen_dir, K, L, E, **kw):
    """built once per module and never changed: the oracle's run is the slow part"""
    key = (K, L, E, tuple(sorted(kw.items())))
    if key not in _scenarios:
        _scenarios[key] = ru.Scenario(synth, scen_dir, K, L, E, seed=SEED.get((K, L, E), 100 * K + L), **kw)
    return _scenarios[key]


def counted(pkg, s):
    """pass 1 over the scenario's reads, one batch, on a fresh context that keeps them and tracks first occurrences"""
    g = pkg.PregraphGPU(s.K, est_distinct=2 * len(s.keys4), flags=pkg.SDT_FLAG_KEEP_READS | pkg.SDT_FLAG_TRACK_FIRST)
    g.push_reads(s.words, s.offs)
    g.finish_count()
    return g


def device_nodes(g, s):
    """-> (the table's keys as export_nodes gives them, index of each in the scenario's node arrays)"""
    keys = g.export_nodes()[0]
    return keys, s.device_order(keys)


def arcs_of(g):
    """map_reads + export_arcs -> (kept reads, [(from, to, mult)], [first])"""
    reads, n = g.map_reads()
    fr, to, mult, first = g.export_arcs()
    assert len(fr) == n
    return reads, list(zip(fr.tolist(), to.tolist(), mult.tolist())), first.tolist()


def assert_is_oracles(s, reads, arcs, first, nreads=None):
    assert reads == (s.nreads if nreads is None else nreads)
    assert len(arcs) == s.narcs
    assert arcs == s.arcs                          # as sequences: from ascending, within a from the arc seen first comes last
    assert all(a > b for x, y, a, b in zip(arcs, arcs[1:], first, first[1:]) if x[0] == y[0]), "first must descend within a from"
    assert first == s.first                        # (read ordinal << 16) | item index of the first appearance (include/sdt_gpu.h)


@pytest.mark.parametrize("E", [6, 5000])
@pytest.mark.parametrize("K,L", CASES)
def test_map_reads_equals_oracle_on_random_states(pkg, synth, scen_dir, K, L, E):
    s = scenario(synth, scen_dir, K, L, E)
    assert s.walk_arcs == s.arcs                   # the walk that supplies the preconditions and `first` is the oracle's
    s.check_preconditions(min_occurrences=1000, min_distinct=1000 if E > 36 else 0)
    g = counted(pkg, s)
    with g:
        keys, idx = device_nodes(g, s)
        g.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        assert_is_oracles(s, *arcs_of(g))


def test_arc_map_regrows(pkg, synth, scen_dir):
    """more distinct arcs than the 65 536 slots the arc map starts with at num_ed = 0: the first attempt must overflow, the map
    doubles and the pass is redone from a clean map; a second map_reads starts from the grown map.  (Few skip nodes and few
    vertices here: paths as long as the reads, so that 3 000 reads have that many arcs.)"""
    s = scenario(synth, scen_dir, 21, 250, 60000, n_reads=3000, T=100, shares=(0.001, 0.001, 0.948, 0.05), zero=0.001)
    assert s.narcs == len(s.arcs) and len(s.arcs) > 65536 and s.walk_arcs == s.arcs
    g = counted(pkg, s)
    with g:
        keys, idx = device_nodes(g, s)
        g.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, 0)
        assert_is_oracles(s, *arcs_of(g))
        assert_is_oracles(s, *arcs_of(g))


def test_many_kept_batches_and_interleaved_ordinals(pkg, synth, scen_dir):
    """two paired files pushed as 6 batches each, alternating, with the ordinals of the interleaved stream (file 1: 0, 2, 4, ...;
    file 2: 1, 3, 5, ...): more than 8 kept batches take the six-stream launch.  The interleaved stream is the scenario's own"""
    K, L, E = 31, 100, 5000
    s = scenario(synth, scen_dir, K, L, E)
    g = pkg.PregraphGPU(K, est_distinct=2 * len(s.keys4), flags=pkg.SDT_FLAG_KEEP_READS | pkg.SDT_FLAG_TRACK_FIRST)
    with g:
        files = [np.arange(f, s.nreads, 2) for f in (0, 1)]
        cuts = [np.linspace(0, len(f), 7).astype(np.int64) for f in files]
        nb = 0
        for b in range(6):
            for f in (0, 1):
                part = files[f][cuts[f][b]:cuts[f][b + 1]]
                assert len(part) and int(part[0]) == 2 * int(cuts[f][b]) + f
                g.set_read_ordinal(int(part[0]), 2)
                codes, offs = ru.take_reads(s.codes, s.offs, part)
                g.push_reads(synth.pack_2bit(codes), offs)
                nb += 1
        assert nb == 12
        g.finish_count()
        keys, idx = device_nodes(g, s)
        g.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        many = arcs_of(g)
        assert_is_oracles(s, *many)
    g1 = counted(pkg, s)
    with g1:
        keys, idx = device_nodes(g1, s)
        g1.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        assert arcs_of(g1) == many


def test_load_paths_forms_agree(pkg, synth, scen_dir):
    K, L, E = 47, 100, 5000
    s = scenario(synth, scen_dir, K, L, E)
    rng = np.random.default_rng(3)
    results = []
    # keyed, the keys in a random permutation
    g = counted(pkg, s)
    with g:
        keys, idx = device_nodes(g, s)
        perm = rng.permutation(len(keys))
        g.load_paths(keys[perm], s.path_words[idx[perm]], s.patch_keys, s.patch_info, E)
        results.append(arcs_of(g))
    # by index after set_node_index: path_words[i] belongs to keys[i]
    g = counted(pkg, s)
    with g:
        keys, idx = device_nodes(g, s)
        perm = rng.permutation(len(keys))
        g.set_node_index(keys[perm])
        g.load_paths(None, s.path_words[idx[perm]], s.patch_keys, s.patch_info, E)
        results.append(arcs_of(g))
    # by index after layout_sorted_keys + layout_apply: node v is the key of rank order[v]
    g = counted(pkg, s)
    with g:
        skeys, _ = g.layout_sorted_keys(4, g.nw)
        order = rng.permutation(len(skeys)).astype(np.uint64)
        g.layout_apply(order)
        sidx = s.device_order(skeys)
        g.load_paths(None, s.path_words[sidx[order.astype(np.int64)]], s.patch_keys, s.patch_info, E)
        results.append(arcs_of(g))
    assert_is_oracles(s, *results[0])
    assert results[1] == results[0] and results[2] == results[0]


def merge_arcs(parts):
    """arcs of several contexts added up as the ranks of --gpus N add theirs: mult summed, first = the minimum, *.preArc's order"""
    acc = {}
    for arcs, first in parts:
        for (f, t, m), o in zip(arcs, first):
            a = acc.setdefault((f, t), [0, o])
            a[0] += m
            a[1] = min(a[1], o)
    order = sorted(acc, key=lambda k: (k[0], -acc[k][1]))
    return [(k[0], k[1], acc[k][0]) for k in order], [acc[k][1] for k in order]


def test_export_import_paths_round_trip_and_arc_sums(pkg, synth, scen_dir):
    K, L, E = 65, 250, 5000
    s = scenario(synth, scen_dir, K, L, E)
    a = counted(pkg, s)
    with a:
        keys, idx = device_nodes(a, s)
        a.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        xkeys, xwords = a.export_paths()
        xi = s.device_order(xkeys)                 # every key once (the key sets are equal and of equal size) ...
        assert (xwords == s.path_words[xi]).all()  # ... with its word
        whole = arcs_of(a)
        assert_is_oracles(s, *whole)
    half = s.nreads // 2
    shares = [np.arange(0, half), np.arange(half, s.nreads)]

    def rank(share, release):
        b = pkg.PregraphGPU(K, est_distinct=1 << 12)      # smaller than the graph: import_paths makes the room
        with b:
            b.set_read_ordinal(int(share[0]), 1)
            codes, offs = ru.take_reads(s.codes, s.offs, share)
            b.keep_reads(synth.pack_2bit(codes), offs)
            if release:
                b.release_table()
            b.import_paths(xkeys, xwords, s.patch_keys, s.patch_info, E)
            reads, arcs, first = arcs_of(b)
            assert reads == len(share)
            return arcs, first

    b1, b2 = rank(shares[0], False), rank(shares[1], False)
    assert len(b1[0]) and len(b2[0]) and b1 != b2
    assert merge_arcs([b1, b2]) == (whole[1], whole[2]) == (s.arcs, s.first)
    assert rank(shares[0], True) == b1


def test_pass2_states_and_errors(pkg, synth, scen_dir):
    K, L, E = 21, 100, 6
    s = scenario(synth, scen_dir, K, L, E)
    rng = np.random.default_rng(11)

    def fails(call, code, text=""):
        with pytest.raises(pkg.SdtError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)

    g = counted(pkg, s)
    with g:
        keys, idx = device_nodes(g, s)
        fails(g.map_reads, pkg.SDT_ESTATE, "load_paths")
        # a key that is not in the table: nothing of pass 1 holds a k-mer of all G's next to all A's
        alien = np.zeros((1, g.nw), dtype=np.uint64)
        alien[0, -1] = 0b11 << 2 * (K - 1)
        assert not (keys == alien).all(axis=1).any()
        fails(lambda: g.load_paths(np.concatenate([keys, alien]), np.concatenate([s.path_words[idx], [np.uint64(0)]]), s.patch_keys,
                                   s.patch_info, E), pkg.SDT_ESTATE, "1 nodes are not in the table")
        # the context recovers (see the header): the counter load_paths raised is cleared, a correct call succeeds
        g.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        reads, arcs, first = arcs_of(g)
        assert_is_oracles(s, reads, arcs, first)
        fails(lambda: g.export_arcs(len(arcs) - 1), pkg.SDT_EINVAL, f"need {len(arcs)}")
        fr, to, mult, first2 = g.export_arcs(len(arcs))
        assert list(zip(fr.tolist(), to.tolist(), mult.tolist())) == arcs and first2.tolist() == first
        # kept reads that the table has never seen: two of them (and one too short to be looked at)
        foreign = rng.integers(0, 4, size=3 * K + 8, dtype=np.uint8)
        offs = np.array([0, K + 5, 2 * K + 8, 3 * K + 8], dtype=np.uint64)
        canon = {min(a, b) for a, b in (kmer_pair(foreign[i:i + K], K) for i in (0, K + 5))}
        assert not canon & set(s.node_of)
        g.keep_reads(synth.pack_2bit(foreign), offs)
        fails(g.map_reads, pkg.SDT_ESTATE, "2 reads hold a k-mer that is not in the node table")
    # no kept reads
    g = pkg.PregraphGPU(K, est_distinct=2 * len(s.keys4))
    with g:
        g.push_reads(s.words, s.offs)
        g.finish_count()
        keys, idx = device_nodes(g, s)
        g.load_paths(keys, s.path_words[idx], s.patch_keys, s.patch_info, E)
        fails(g.map_reads, pkg.SDT_ESTATE, "not kept")
        xkeys, xwords = g.export_paths()
    # import_paths with one key twice
    g = pkg.PregraphGPU(K, est_distinct=1 << 12)
    with g:
        g.keep_reads(s.words, s.offs)
        fails(lambda: g.import_paths(np.concatenate([xkeys, xkeys[7:8]]), np.concatenate([xwords, xwords[7:8]]), s.patch_keys,
                                     s.patch_info, E), pkg.SDT_ESTATE)
        g.import_paths(xkeys, xwords, s.patch_keys, s.patch_info, E)
        assert_is_oracles(s, *arcs_of(g))


def kmer_pair(codes, K):
    fw = rc = 0
    for c in codes.tolist():
        fw = (fw << 2) | c
        rc = (rc >> 2) | ((c ^ 2) << 2 * (K - 1))
    return fw, rc
