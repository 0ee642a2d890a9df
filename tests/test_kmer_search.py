"""GPU (-m gpu): sdt_gpu_search_kmers and the read profiles against the oracle's node table.  Expectations never come from the
library under test: the node dictionary is the oracle's (oracle_binding.Oracle.export), a read's canonical k-mers are plain
Python integers."""
import gzip
import os
import subprocess
import warnings

import numpy as np
import pytest

import oracle_binding as ob
import golden_util as gu

pytestmark = pytest.mark.gpu

MODES = [1, 2]           # SDT_FLAG_DIRECT, SDT_FLAG_PARTITION: the two pass-1 kernel families


# ---- expectations ------------------------------------------------------------------------------------------------------------
def keys_to_int(keys):
    out = []
    for row in keys:
        v = 0
        for x in row:
            v = (v << 64) | int(x)
        out.append(v)
    return out


def int_to_keys(vals, nw):
    a = np.zeros((len(vals), nw), dtype=np.uint64)
    m = (1 << 64) - 1
    for i, v in enumerate(vals):
        for w in range(nw):
            a[i, nw - 1 - w] = (v >> (64 * w)) & m
    return a


def _revcomp_byte(b):
    return ((b & 3) ^ 2) << 6 | ((b >> 2 & 3) ^ 2) << 4 | ((b >> 4 & 3) ^ 2) << 2 | ((b >> 6 & 3) ^ 2)


_RC_BYTES = bytes(_revcomp_byte(b) for b in range(256))


def revcomp_int(v, K):
    """reverse complement of a K-mer held as an integer: four bases per byte through a table, bytes reversed; the A's that pad the top
    byte come out as T's at the bottom and are shifted away"""
    nb = (K + 3) // 4
    return int.from_bytes(v.to_bytes(nb, "big").translate(_RC_BYTES)[::-1], "big") >> (2 * (4 * nb - K))


def test_revcomp_helper_is_an_involution_and_matches_the_definition():
    rng = np.random.default_rng(1)
    for K in (13, 21, 31, 33, 63, 65, 95, 97, 127):
        bases = rng.integers(0, 4, size=K).tolist()
        v = 0
        for c in bases:
            v = (v << 2) | c
        r = 0
        for c in reversed(bases):
            r = (r << 2) | (c ^ 2)
        assert revcomp_int(v, K) == r and revcomp_int(r, K) == v
        assert canon_kmers(np.array(bases, dtype=np.uint8), K) == [min(v, r)]


def canon_kmers(codes, K):
    """the canonical k-mers of a read as integers (first base most significant, A0 C1 T2 G3, complement = code ^ 2)"""
    mask = (1 << (2 * K)) - 1
    top = 2 * (K - 1)
    fw = rc = 0
    out = []
    for i, c in enumerate(codes.tolist()):
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((c ^ 2) << top)
        if i >= K - 1:
            out.append(fw if fw < rc else rc)
    return out


def node_dict_oracle(o):
    """key -> (l_links, r_flags as sdt_gpu_export_nodes has them, count)"""
    keys, l, r, cnt, fl = o.export()
    ki = keys_to_int(keys)
    # oracle flags: bit0 linear, bit1 deleted, bit2 single -> r_flags bits 24, 25, 27
    return {k: (int(a), int(b) | (int(f) & 1) << 24 | (int(f) >> 1 & 1) << 25 | (int(f) >> 2 & 1) << 27, int(c))
            for k, a, b, f, c in zip(ki, l, r, fl, cnt)}


def expect_search(queries, K, nodes):
    """queries: integers, either strand -> (count, l_links, r_flags, status)"""
    n = len(queries)
    cnt, l, rf = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    st = np.zeros(n, dtype=np.uint8)
    for i, q in enumerate(queries):
        rc = revcomp_int(q, K)
        larger = rc < q
        node = nodes.get(rc if larger else q)
        st[i] = (2 if larger else 0) | (1 if node else 0)
        if node:
            l[i], rf[i], cnt[i] = node
    return cnt, l, rf, st


def expect_profile(codes, offs, K, nodes, min_count):
    out = np.zeros(len(offs) - 1, dtype=[(f, np.uint32) for f in ("kmers", "found", "solid", "min", "median", "max")])
    for r in range(len(offs) - 1):
        ks = canon_kmers(codes[int(offs[r]):int(offs[r + 1])], K)
        if not ks:
            continue
        c = sorted(nodes[k][2] if k in nodes else 0 for k in ks)
        out[r] = (len(ks), sum(k in nodes for k in ks), sum(x >= min_count for x in c), c[0], c[(len(c) - 1) // 2], c[-1])
    return out


def assert_cov_equal(got, want, what=""):
    assert got.dtype.names == want.dtype.names
    for f in want.dtype.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def absent_kmers(K, nodes, seed, draw=2000):
    rng = np.random.default_rng(seed)
    out = []
    for row in rng.integers(0, 4, size=(draw, K)):
        v = 0
        for c in row.tolist():
            v = (v << 2) | c
        if min(v, revcomp_int(v, K)) not in nodes:
            out.append(v)
    assert len(out) >= 1000, f"only {len(out)} of {draw} random {K}-mers are absent from the oracle's table"
    return out


def workload(synth, K, L, n_reads=6000):
    tx = synth.make_transcriptome(25, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=n_reads, read_len=L, seed=K + 1, err=0.003, ragged=True)
    return tx, codes, offs


def hot_input(K):
    """the input of test_saturation_and_hot_keys: 1 000 poly-A reads (one node counted 1000 x (L - K + 1) times: 80 000 at K = 21) and
    500 reads of a tandem repeat; L = 100 for 1-word keys.  Longer k-mers get reads of 250 bases so that the count still passes 65 535"""
    n, L = 1500, 100 if K <= 31 else 250
    codes = np.zeros(n * L, dtype=np.uint8)
    codes[L * 1000:] = np.tile(np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8), (n - 1000) * L // 6 + 1)[: (n - 1000) * L]
    return codes, (np.arange(n + 1) * L).astype(np.uint64)


# ---- 1. search equals the oracle ---------------------------------------------------------------------------------------------
def check_search(g, K, nodes, seed):
    stored = sorted(nodes)
    flipped = [revcomp_int(k, K) for k in stored]
    absent = absent_kmers(K, nodes, seed)
    queries = stored + flipped + absent + [stored[len(stored) // 3]] * 200
    want = expect_search(queries, K, nodes)
    assert (want[3][:len(stored)] == 1).all() and (want[3][len(stored):2 * len(stored)] == 3).all()
    assert ((want[3][2 * len(stored):2 * len(stored) + len(absent)] & 1) == 0).all()
    keys = int_to_keys(queries, g.nw)
    for n in (0, 1, 63, 65, len(queries)):
        got = g.search_kmers(keys[:n])
        for name, a, b in zip(("count", "l_links", "r_flags", "status"), got, want):
            bad = np.nonzero(a != b[:n])[0]
            assert bad.size == 0, f"batch of {n}: {name} differs at {bad[:8].tolist()}: got {a[bad[:8]].tolist()} want {b[:n][bad[:8]].tolist()}"
    # the repeated query alone, and outputs that are not asked for
    rep = int_to_keys([flipped[7]] * 200, g.nw)
    cnt, l, rf, st = g.search_kmers(rep)
    assert (st == 3).all() and (cnt == nodes[stored[7]][2]).all() and (l == nodes[stored[7]][0]).all() and (rf == nodes[stored[7]][1]).all()
    only = np.zeros(len(queries), dtype=np.uint32)
    g._check(g.lib.sdt_gpu_search_kmers(g._ctx, keys.ctypes.data, len(queries), only.ctypes.data, None, None, None))
    assert (only == want[0]).all()
    return queries, keys, want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,L", [(13, 60), (31, 150), (33, 150), (63, 250), (65, 200), (95, 420), (97, 250), (127, 250)])
def test_search_equals_oracle(pkg, synth, K, L, mode):
    """every oracle node as stored, the reverse complement of every node, k-mers verified to be absent, one query 200 times; batches of
    0, 1, 63, 65 and all; count, l_links, r_links and the linear / deleted / single bits -- and once more after delow(2) + mark"""
    _, codes, offs = workload(synth, K, L)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=mode) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        for d in (0, 2):
            if d:
                assert g.delow(d) == o.delow(d)
            g.mark_and_hist()
            o.mark()
            nodes = node_dict_oracle(o)
            assert any(v[1] >> 24 & 1 for v in nodes.values()) and any(v[1] >> 27 & 1 for v in nodes.values())
            assert not d or any(v[1] >> 25 & 1 for v in nodes.values())
            check_search(g, K, nodes, seed=1000 + K + d)


# ---- 2. device-pointer form ----------------------------------------------------------------------------------------------------
def test_search_device_form_equals_host_form(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    K, L = 33, 150
    _, codes, offs = workload(synth, K, L)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    o.mark()
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        nodes = node_dict_oracle(o)
        queries, keys, want = check_search(g, K, nodes, seed=77)
        n = len(queries)
        d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
        d_cnt, d_l, d_rf = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(3))
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g.search_kmers_device(d_keys, n, d_cnt, d_l, d_rf, d_st)
        g.kernel_time(reset=True)                               # (waits for the context's stream)
        host = g.search_kmers(keys)
        for a, b, w in zip((d_cnt, d_l, d_rf, d_st), host, want):
            a = a.cpu().numpy().view(b.dtype)
            assert (a == b).all() and (a == w).all()
        g.search_kmers_device(d_keys, 0, None, None, None, None)


# ---- 3. profile equals numpy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [21, 31, 63, 95, 65, 97])
def test_profile_equals_numpy(pkg, synth, K):
    """ragged reads of the counted workload, hand-made reads of K - 1, K and K + 1 bases and of more than 256 k-mers, reads of another
    seed that hold k-mers the table does not have; min_count 0, 1, 2, 50; all six fields of every read"""
    L = 150 if K <= 31 else 250
    tx, codes, offs = workload(synth, K, L, n_reads=4000)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    nodes = node_dict_oracle(o)
    t = tx[0]
    hand = [t[100:100 + K - 1], t[200:200 + K], (t[300:300 + K + 1][::-1] ^ 2).astype(np.uint8), t[40:40 + 330], t[10:10 + 480],
            np.zeros(K + 5, dtype=np.uint8)]
    other, ooffs = synth.sample_reads(*tx, n_reads=400, read_len=L, seed=K + 99, err=0.02, ragged=True)
    parts = [codes] + hand + [other]
    lens = np.concatenate([np.diff(offs.astype(np.int64)), [len(h) for h in hand], np.diff(ooffs.astype(np.int64))])
    pcodes = np.concatenate(parts)
    poffs = np.zeros(len(lens) + 1, dtype=np.uint64)
    poffs[1:] = np.cumsum(lens)
    n0 = len(offs) - 1
    assert int(lens[n0 + 3]) - K + 1 > 256 or K > 75
    first_other = n0 + len(hand)
    absent = sum(k not in nodes for r in range(first_other, len(lens)) for k in canon_kmers(pcodes[int(poffs[r]):int(poffs[r + 1])], K))
    assert absent > 100, "the reads of the other seed must hold k-mers the oracle's table does not have"
    words = synth.pack_2bit(pcodes)
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        for mc in (0, 1, 2, 50):
            want = expect_profile(pcodes, poffs, K, nodes, mc)
            got = g.profile_reads(words, poffs, min_count=mc)
            assert got.dtype == pkg.READ_COV_DTYPE
            assert_cov_equal(got, want, f"K={K} min_count={mc}")
            if mc == 0:
                assert (got["solid"] == got["kmers"]).all()
        assert tuple(want[n0]) == (0,) * 6 and want[n0 + 1]["kmers"] == 1 and want[n0 + 2]["kmers"] == 2
        assert (want["found"] < want["kmers"]).any() and (want["min"] > 0).any()
        # a batch of nothing, and a batch that starts in the middle of a word
        assert len(g.profile_reads(words, poffs[:1])) == 0
        got = g.profile_reads(synth.pack_2bit(pcodes[int(poffs[5]):]), poffs[5:] - poffs[5], min_count=2)
        assert_cov_equal(got, expect_profile(pcodes, poffs, K, nodes, 2)[5:], "shifted batch")


@pytest.mark.parametrize("aux_form", ["", "hash", "aux"])
@pytest.mark.parametrize("K", [21, 31, 63, 95, 65, 97])
def test_profile_counts_past_65535(pkg, synth, monkeypatch, K, aux_form):
    """1 000 poly-A reads: one node counted tens of thousands of times, so min, median and max of those reads need the high half of
    the count -- through the small hash of such nodes (the default), and through aux itself (test hook)"""
    if aux_form:
        monkeypatch.setenv("SDT_PROFILE_AUX", aux_form)
    codes, offs = hot_input(K)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    nodes = node_dict_oracle(o)
    assert max(v[2] for v in nodes.values()) > 65535
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        for mc in (0, 1, 2, 50, 70000):
            want = expect_profile(codes, offs, K, nodes, mc)
            assert want["median"][0] > 65535 and want["min"][0] > 65535 and want["max"][0] == want["min"][0]
            assert_cov_equal(g.profile_reads(synth.pack_2bit(codes), offs, min_count=mc), want, f"K={K} min_count={mc} {aux_form}")
        # the table changes: what was collected about it must go.  Another 1 000 poly-A reads double the hot node's count.
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        o.add_reads(codes, offs)
        want = expect_profile(codes, offs, K, node_dict_oracle(o), 0)
        assert want["median"][0] > 2 * 65535
        assert_cov_equal(g.profile_reads(synth.pack_2bit(codes), offs), want, "after a second count")
        cnt, _, _, st = g.search_kmers(np.zeros((1, g.nw), dtype=np.uint64))
        assert st[0] == 1 and cnt[0] == want["max"][0]


# ---- 4. kept reads --------------------------------------------------------------------------------------------------------------
def test_profile_kept_reads_by_ordinal(pkg, synth):
    K, L = 31, 100
    tx = synth.make_transcriptome(20, seed=5)
    (c1, o1), (c2, o2) = synth.sample_pairs(*tx, n_pairs=700, read_len=L, seed=6, err=0.004)
    ca, oa = synth.sample_reads(*tx, n_reads=1500, read_len=140, seed=7, err=0.004, ragged=True)
    cb, ob_ = synth.sample_reads(*tx, n_reads=900, read_len=120, seed=8, err=0.004, ragged=False)
    assert (np.diff(ob_.astype(np.int64)) == 120).all()
    np1 = len(o1) - 1
    wb = synth.pack_2bit(cb)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.set_read_ordinal(0, 2)
        g.push_reads(synth.pack_2bit(c1), o1)
        g.set_read_ordinal(1, 2)
        g.push_reads(synth.pack_2bit(c2), o2)
        g.set_read_ordinal(2 * np1, 1)
        g.push_reads(synth.pack_2bit(ca), oa)
        g.push_wait(g.push_reads_fixed_async(wb, len(ob_) - 1, 120))
        g.finish_count()
        # the same reads in ordinal order: the pairs interleaved, then the two single-end batches
        reads = []
        for i in range(np1):
            reads.append(c1[int(o1[i]):int(o1[i + 1])])
            reads.append(c2[int(o2[i]):int(o2[i + 1])])
        reads += [ca[int(oa[i]):int(oa[i + 1])] for i in range(len(oa) - 1)]
        reads += [cb[int(ob_[i]):int(ob_[i + 1])] for i in range(len(ob_) - 1)]
        total = len(reads)
        offs = np.zeros(total + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        codes = np.concatenate(reads)
        for mc in (0, 3):
            want = g.profile_reads(synth.pack_2bit(codes), offs, min_count=mc)
            got, n = g.profile_kept_reads(total, min_count=mc)
            assert n == total
            assert_cov_equal(got, want, f"kept reads, min_count={mc}")
        assert (want["found"] == want["kmers"]).all() and (want["kmers"] > 0).sum() > total // 2
        # a larger array: the records past the last ordinal stay as they were
        big = np.full(total + 5, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_COV_DTYPE)
        got, n = g.profile_kept_reads(total + 5, min_count=3, out=big)
        assert n == total and (got[total:].view(np.uint32) == 0xABABABAB).all()
        assert_cov_equal(got[:total], want, "kept reads into a larger array")
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_COV_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.profile_kept_reads(total - 1, out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()


# ---- 5. read-only ---------------------------------------------------------------------------------------------------------------
def test_search_and_profile_leave_the_table_alone(pkg, synth):
    K, L = 31, 150
    _, codes, offs = workload(synth, K, L)
    words = synth.pack_2bit(codes)

    def snapshot(g):
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt, first)]

    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(words, offs)
        g.finish_count()
        hist0, lin0 = g.mark_and_hist()
        before = snapshot(g)
        rng = np.random.default_rng(3)
        q = np.concatenate([before[0][::3], rng.integers(0, 1 << 62, size=(5000, 1), dtype=np.uint64)])
        cnt, _, _, st = g.search_kmers(q)
        assert (st[:len(before[0][::3])] & 1).all() and (cnt[:len(before[0][::3])] == before[3][::3]).all()
        cov = g.profile_reads(words, offs, min_count=2)
        assert (cov["found"] == cov["kmers"]).all()
        after = snapshot(g)
        for a, b in zip(before, after):
            assert a.shape == b.shape and (a == b).all()
        hist1, lin1 = g.mark_and_hist()
        assert lin1 == lin0 and (hist1 == hist0).all()


def test_host_batches_go_through_in_pieces(pkg, synth, monkeypatch):
    """host batches are staged piece by piece (4 M queries / reads at a time); with pieces of 777 (test hook) the same answers must
    come back, whatever word a piece of reads starts in"""
    K, L = 31, 150
    _, codes, offs = workload(synth, K, L, n_reads=3000)
    words = synth.pack_2bit(codes)
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(words, offs)
        g.finish_count()
        keys = g.export_nodes()[0]
        q = np.concatenate([keys, keys[::-1] ^ np.uint64(0x5A5A5A5A5A5A5A)])
        whole_s = g.search_kmers(q)
        whole_p = g.profile_reads(words, offs, min_count=2)
        assert (whole_s[3][:len(keys)] == 1).all() and (whole_p["found"] == whole_p["kmers"]).all()
        monkeypatch.setenv("SDT_SEARCH_CHUNK", "777")
        for a, b in zip(g.search_kmers(q), whole_s):
            assert (a == b).all()
        assert_cov_equal(g.profile_reads(words, offs, min_count=2), whole_p, "pieces of 777 reads")
        monkeypatch.setenv("SDT_SEARCH_CHUNK", "1")
        assert_cov_equal(g.profile_reads(words, offs[:41], min_count=2), whole_p[:40], "pieces of one read")


# ---- 6. state errors ------------------------------------------------------------------------------------------------------------
def small_input(synth, K=31):
    tx = synth.make_transcriptome(5, seed=11)
    codes, offs = synth.sample_reads(*tx, n_reads=500, read_len=100, seed=12, err=0.0)
    return codes, offs, synth.pack_2bit(codes)


def assert_state_error(pkg, g, words, offs, code=None):
    code = pkg.SDT_ESTATE if code is None else code
    calls = [lambda: g.search_kmers(np.zeros((3, g.nw), dtype=np.uint64)), lambda: g.profile_reads(words, offs),
             lambda: g.profile_kept_reads(len(offs) - 1)]
    for call in calls:
        with pytest.raises(pkg.SdtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert len(g.lib.sdt_gpu_last_error()) > 10


def test_state_errors(pkg, synth):
    import torch
    K = 31
    codes, offs, words = small_input(synth, K)
    n = len(offs) - 1
    # pushed, not drained -- and fine again once drained; empty batches are fine in any state
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(words, offs)
        assert_state_error(pkg, g, words, offs)
        assert len(g.search_kmers(np.zeros((0, 1), dtype=np.uint64))[0]) == 0
        g.finish_count()
        assert (g.profile_reads(words, offs)["found"] == L_KMERS(offs, K)).all()
        assert g.profile_kept_reads(n)[1] == n
        # counted from device memory and not drained
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        g.count_reads_device(d_w, len(words), d_o, n, 100)
        assert_state_error(pkg, g, words, offs)
        g.finish_count()
        assert (g.profile_reads(words, offs)["min"] >= 2).all()
        # a read longer than promised: marked, SDT_EINVAL, nothing read out of bounds
        out = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
        with pytest.raises(pkg.SdtError) as e:
            g.profile_reads_device(d_w, d_o, n, 99, 0, out)
        assert e.value.code == pkg.SDT_EINVAL and "longer" in str(e.value)
        rec = out.cpu().numpy().view(np.uint32)
        assert (rec[:, 0] == pkg.COV_TOO_LONG).all() and (rec[:, 1:] == 0).all()
        g.profile_reads_device(d_w, d_o, n, 100, 0, out)
        assert (out.cpu().numpy().view(np.uint32)[:, 0] == 100 - K + 1).all()
        # path words in place of the counters
        g.load_paths(None, None, None, None, 0)
        assert_state_error(pkg, g, words, offs)
    # the table released
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(words, offs)
        g.finish_count()
        g.release_table()
        assert_state_error(pkg, g, words, offs)
    # reads were not kept
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(words, offs)
        g.finish_count()
        with pytest.raises(pkg.SdtError) as e:
            g.profile_kept_reads(n)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
    # a contig index
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        assert_state_error(pkg, g, words, offs)
    # one shard of a sharded table
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.comm_init_shm(f"kms{os.getpid()}", 0, 1)
        assert_state_error(pkg, g, words, offs)


def L_KMERS(offs, K):
    lens = np.diff(offs.astype(np.int64))
    return np.where(lens >= K, lens - K + 1, 0).astype(np.uint32)


# ---- 7. the host program --------------------------------------------------------------------------------------------------------
LETTERS = "ACTG"


def kmer_text(v, K):
    return "".join(LETTERS[(v >> (2 * (K - 1 - i))) & 3] for i in range(K))


def materialise(info, tmp):
    d = info["dir"]
    for f in os.listdir(d):
        if f.endswith(".fq.gz"):
            with gzip.open(os.path.join(d, f), "rb") as fi, open(os.path.join(tmp, f[:-3]), "wb") as fo:
                fo.write(fi.read())
    cfg = os.path.join(tmp, "lib.cfg")
    with open(os.path.join(d, "lib.cfg.template")) as fi, open(cfg, "w") as fo:
        fo.write(fi.read().replace("@DIR@", str(tmp)))
    return cfg


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("name", ["se100_k23_p8", "pe150_k31_p8", "se150_k47_p4_63mer"])
def test_sdt_kmers_cli(pkg, tmp_path, name, d):
    info = gu.load_case(name)
    K = pkg.clamp_K(info["K"], gu.VARIANT_MAXK[info["variant"]])
    cfg = materialise(info, tmp_path)
    codes, offs = gu.case_reads(info)
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    if d:
        o.delow(d)
    o.mark()
    nodes = node_dict_oracle(o)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    opts = ["-s", cfg, "-K", str(info["K"]), "-p", "4", "--max-k", str(gu.VARIANT_MAXK[info["variant"]])] + (["-d", str(d)] if d else [])
    # profile
    r = subprocess.run([exe, "profile"] + opts + ["-c", "3", "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.loadtxt(tmp_path / "out.readCov", dtype=np.uint32, ndmin=2)
    want = expect_profile(codes, offs, K, nodes, 3)
    assert got.shape == (len(offs) - 1, 6)
    assert_cov_equal(got.copy().view(want.dtype).reshape(-1), want, name)
    # query: nodes as stored, nodes flipped, absent k-mers
    stored = sorted(nodes)[::max(1, len(nodes) // 300)]
    queries = stored + [revcomp_int(k, K) for k in stored] + absent_kmers(K, nodes, seed=5)[:100]
    (tmp_path / "q.txt").write_text("".join(kmer_text(v, K) + "\n" for v in queries))
    r = subprocess.run([exe, "query"] + opts + ["-q", str(tmp_path / "q.txt"), "-o", str(tmp_path / "out.tsv")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cnt, l, rf, st = expect_search(queries, K, nodes)
    lines = (tmp_path / "out.tsv").read_text().splitlines()
    assert len(lines) == len(queries)
    for i, line in enumerate(lines):
        want_line = [kmer_text(queries[i], K), str(st[i] & 1), "-" if st[i] & 2 else "+", str(cnt[i])] + \
                    [str(int(l[i]) >> (6 * b) & 63) for b in range(4)] + [str(int(rf[i]) >> (6 * b) & 63) for b in range(4)] + \
                    [str(int(rf[i]) >> 24 & 1), str(int(rf[i]) >> 25 & 1)]
        assert line.split() == want_line, (i, line)
    # without -o the answers go to standard output
    r2 = subprocess.run([exe, "query"] + opts + ["-q", str(tmp_path / "q.txt")], capture_output=True, text=True)
    assert r2.returncode == 0 and [x for x in r2.stdout.splitlines() if "\t" in x] == lines


# ---- 8. rate guard --------------------------------------------------------------------------------------------------------------
def test_profile_rate_floor(pkg, synth):
    """not a benchmark -- a guard against order-of-magnitude regressions, in the style of test_kernel_rate_floors: 4 M reads of 150
    bases, K = 31, 2 000 transcripts, counted on the device, k_profile_reads timed by the library's events.  Measured on an MI355X
    (profiles/kmer_search/README.md): 37.8 G k-mers/s, k_align_reads on the same reads in the same call 56.5 G.  PROFILE_FLOOR is a
    third of the measured rate rounded down to a whole G -- the ratio the floors of test_kernel_rate_floors have to their
    measurements (15 of 50; 8 of 19.6 - 40).  A miss is a WARNING unless SDT_STRICT_RATES=1; the results are asserted either way."""
    import torch

    def floor(rate, limit, what):
        print(f"{what}: {rate / 1e9:.2f} G k-mers/s (floor {limit / 1e9:.0f})")
        if rate > limit:
            return
        msg = f"{what}: {rate / 1e9:.1f} G k-mers/s is below the floor of {limit / 1e9:.0f}"
        if os.environ.get("SDT_STRICT_RATES") == "1":
            raise AssertionError(msg)
        warnings.warn(msg)

    dev = torch.device("cuda:0")
    K, L, n, T = 31, 150, 4_000_000, 2000
    words, offsets, nwords = synth.torch_workload(n, L, T, dev)
    torch.cuda.synchronize()
    kmers = n * (L - K + 1)
    with pkg.PregraphGPU(K, est_distinct=1 << 26) as g:
        g.count_reads_device(words, nwords, offsets, n, L)
        got, nodes = g.finish_count()
        assert got == kmers
        out = torch.zeros((n, 6), dtype=torch.int32, device=dev)
        for _ in range(3):
            g.kernel_time(reset=True)
            g.profile_reads_device(words, offsets, n, L, 2, out)
            ms, launches, _ = g.kernel_time(reset=True)
        assert launches == 1
        rec = out.cpu().numpy().view(np.uint32)
        # every read was counted: all of its k-mers are found, none is rarer than 1, and the order statistics are ordered
        assert (rec[:, 0] == L - K + 1).all() and (rec[:, 1] == L - K + 1).all()
        assert (rec[:, 3] >= 1).all() and (rec[:, 3] <= rec[:, 4]).all() and (rec[:, 4] <= rec[:, 5]).all()
        assert (rec[:, 2] <= rec[:, 0]).all() and ((rec[:, 3] >= 2) == (rec[:, 2] == rec[:, 0])).all()
        # against the node table itself on a sample: the host form of the search gives the counts of a read's k-mers
        w = words.cpu().numpy().view(np.uint32)
        for r in (0, 1234567, n - 1):
            codes = np.array([(int(w[(r * L + i) >> 4]) >> (30 - 2 * ((r * L + i) & 15))) & 3 for i in range(L)], dtype=np.uint8)
            c = np.sort(g.search_kmers(int_to_keys(canon_kmers(codes, K), 1))[0])
            assert tuple(rec[r]) == (L - K + 1, L - K + 1, int((c >= 2).sum()), c[0], c[(len(c) - 1) // 2], c[-1])
        floor(kmers / (ms * 1e-3), PROFILE_FLOOR, "k_profile_reads")


PROFILE_FLOOR = 12e9      # k-mers/s: 37.8 G measured / 3, rounded down (test_profile_rate_floor)
