"""CPU: the harness of tests/test_read2edge.py.  The GPU tests run the oracle's sdto_read2edge on node states of their own making; that
is only a reference if (1) the setters can express everything the pass reads -- shown by copying a NATURAL state (pass 1, -d, the
cleaning passes, kmer2edges) node by node and patch entry by patch entry onto a fresh instance and getting the same *.preArc -- and
(2) the Python walk that picks the patch candidates, judges the preconditions and supplies the first-appearance ordinals pairs
k-mers as parse1read does -- shown by its arcs being the oracle's on random states."""
import numpy as np
import pytest

import oracle_binding as ob
import read2edge_util as ru


@pytest.mark.parametrize("K", [25, 45, 127, 33, 97])
def test_setters_reproduce_a_natural_state(synth, tmp_path, K):
    L, d = (250 if K > 90 else 100), 1
    # isoforms that share exons: junction vertices, short edges, (K+1)-mer patches and arcs in number, which transcripts of
    # independent random bases would hardly give
    rng = np.random.default_rng(K)
    base = synth.make_transcriptome(1, seed=K, lo=6000, hi=6000)[0]
    iso = [np.concatenate([base[200 * c: 200 * c + 200] for c in rng.choice(30, size=8, replace=False)]) for _ in range(12)]
    starts = np.concatenate([[0], np.cumsum([len(x) for x in iso])]).astype(np.int64)
    codes, offs = synth.sample_reads(np.concatenate(iso), starts, np.full(12, 1 / 12), n_reads=2000, read_len=L, seed=K + 100,
                                     err=0.004, ragged=True)
    a = ob.Oracle(K, nsets=4)
    a.add_reads(codes, offs)
    a.delow(d)
    a.mark()
    a.remove_minor_out(5)
    a.remove_single_tips()
    a.remove_minor_tips()
    num_ed, _, extra = a.write_edges(str(tmp_path / "a.edge"))
    n_a = a.read2edge(codes, offs, str(tmp_path / "a.preArc"))
    text = open(tmp_path / "a.preArc").read()
    assert num_ed > 0 and n_a > 50 and a.num_ed() == num_ed
    keys4, linear, deleted, l_links, twin, in_edge = a.get_node_states()
    pk, pe, pt = a.patch_export()
    # the natural state is not a trivial one: every kind of node, both strands' twins, patch entries
    assert deleted.any() and (linear & in_edge).any() and ((linear == 0) & (deleted == 0)).any() and len(pk) > 0 and len(pk) <= extra
    assert a.node_get_edge(keys4[0]) == (int(l_links[0]), int(twin[0]), int(in_edge[0]))

    b = ob.Oracle(K, nsets=4)
    b.add_reads(codes, offs)
    b.set_node_states(keys4, linear.astype(np.int64), deleted.astype(np.int64), l_links.astype(np.int64), twin.astype(np.int64),
                      in_edge.astype(np.int64))
    for k, e, t in zip(pk, pe.tolist(), pt.tolist()):
        b.patch_put(k, e, t)
    b.set_num_ed(num_ed)
    n_b = b.read2edge(codes, offs, str(tmp_path / "b.preArc"))
    assert n_b == n_a and open(tmp_path / "b.preArc").read() == text
    # and every piece matters: without the patch table, or with inEdge cleared, the text changes
    c = ob.Oracle(K, nsets=4)
    c.add_reads(codes, offs)
    c.set_node_states(keys4, linear.astype(np.int64), deleted.astype(np.int64), l_links.astype(np.int64), twin.astype(np.int64),
                      in_edge.astype(np.int64))
    c.set_num_ed(num_ed)
    c.read2edge(codes, offs, str(tmp_path / "c.preArc"))
    assert open(tmp_path / "c.preArc").read() != text


def test_canonical_kplus1_has_the_128mer_quirk():
    """K + 1 = 128 in the 4-word build: only the last word is complemented and reversed (kmer.c:548-557 through a `char` length)"""
    rng = np.random.default_rng(5)
    o = ob.Oracle(127)
    prev = [int(x) for x in rng.integers(0, 1 << 62, size=4)]
    prev[0] &= (1 << 62) - 1
    v = (prev[0] << 192 | prev[1] << 128 | prev[2] << 64 | prev[3]) << 2 | 3
    key, ps = o.canonical_kplus1(prev, 3)
    last = v & ru.M64
    rev = 0
    for i in range(32):
        rev = (rev << 2) | (((last >> (2 * i)) & 3) ^ 2)
    bal = (v >> 64 << 64) | rev
    assert key == tuple(ru.words4_of(min(v, bal))) and ps == (v < bal)
    # every other length: the ordinary reverse complement
    o31 = ob.Oracle(31)
    w = int(rng.integers(0, 1 << 62))
    v = w << 2 | 1
    rc = 0
    for i in range(32):
        rc = (rc << 2) | (((v >> (2 * i)) & 3) ^ 2)
    key, ps = o31.canonical_kplus1([0, 0, 0, w], 1)
    assert key == (0, 0, 0, min(v, rc)) and ps == (v < rc)


@pytest.mark.parametrize("K,L,E", [(21, 100, 6), (63, 250, 5000), (127, 250, 6), (33, 100, 5000), (97, 250, 6)])
def test_python_walk_pairs_kmers_as_the_oracle_does(synth, tmp_path, K, L, E):
    s = ru.Scenario(synth, tmp_path, K, L, E, seed=1000 + K, n_reads=1200)
    assert s.walk_arcs == s.arcs
    s.check_preconditions(min_occurrences=300)
    assert all(a > b for (f0, _, _), (f1, _, _), a, b in zip(s.arcs, s.arcs[1:], s.first, s.first[1:]) if f0 == f1)
