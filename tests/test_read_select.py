"""GPU (-m gpu): sdt_gpu_select_reads, sdt_gpu_compact_reads and their siblings against the Python restatement of the rule and of the
compaction (read_select_util.py) on the oracle's node table.  Expectations never come from the library under test: counts are the
oracle's (oracle_binding.Oracle.export), the rule is plain Python, and every output is compared for exact equality."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import golden_util as gu
import read_select_util as rs
from read_correct_util import table_counts
from test_kmer_search import hot_input, keys_to_int, materialise, node_dict_oracle, small_input, workload
from test_read_correct import concat, counted_context
from test_read_select_host import keep_masks, length_mix

pytestmark = pytest.mark.gpu

TARGET = 16
COPIES = (1, 8, 16, 64, 512)
# (max_cv_pct, seed): the dispersion test off, on at a bound that the junction read passes, and on at the tightest bound there is
SETTINGS = ((0, 0), (60, 7), (1, 0xFFFFFFFFFFFFFFF1))


@functools.lru_cache(maxsize=None)
def case(K):
    """the counted input -- five transcripts of K + 140 bases counted 1, 8, 16, 64 and 512 times -- the oracle's table for it, and the
    batch to decide: reads of K - 1, K, K + 1, K + 62 .. K + 65 bases from every transcript (the 64-k-mer strip boundary on both
    sides; medians below, at and far above the target of 16), a read across the junction of two transcripts, a read the table does
    not know.  Built once per K and left unchanged."""
    rng = np.random.default_rng(4000 + K)
    Lt = K + 140
    tx = [rng.integers(0, 4, size=Lt, dtype=np.uint8) for _ in COPIES]
    counted, coffs = concat([t for t, c in zip(tx, COPIES) for _ in range(c)])
    o = ob.Oracle(K, nsets=5)
    o.add_reads(counted, coffs)
    count = table_counts(node_dict_oracle(o))
    reads = []
    for t in tx:
        for L in (K - 1, K, K + 1, K + 62, K + 63, K + 64, K + 65):
            for s in rng.integers(0, Lt - L + 1, size=6).tolist():
                r = t[s:s + L]
                reads.append(r if (s & 1) else (r[::-1] ^ 2))                  # either strand
    chimera = len(reads)
    reads.append(np.concatenate([tx[0][-(K + 20):], tx[4][:K + 20]]))         # counts 1, then K - 1 absent k-mers, then 512
    reads.append(rng.integers(0, 4, size=K + 30, dtype=np.uint8))              # nothing found: S1 = 0
    if len(reads) & 1:
        reads.append(tx[2][3:K + 9])
    order = rng.permutation(len(reads))                                       # mates from different transcripts, short mates next to long ones
    reads = [reads[i] for i in order]
    batch, boffs = concat(reads)
    kc = rs.read_kmer_counts(batch, boffs, K, count)
    return dict(K=K, counted=counted, coffs=coffs, count=count, batch=batch, boffs=boffs, kc=kc, chimera=int(np.nonzero(order == chimera)[0][0]),
                oracle=(o.kmers_in_reads(), o.node_count()))


@functools.lru_cache(maxsize=None)
def expected(K, cv, seed, paired):
    c = case(K)
    return rs.expect_select(c["batch"], c["boffs"], K, c["count"], TARGET, cv, seed, paired=paired, kmer_counts=c["kc"])


def assert_select(pkg, got, want, what):
    pick, keep, kept = got
    wpick, wkeep, wkept = want
    assert pick.dtype == pkg.READ_PICK_DTYPE
    rs.assert_pick_equal(pick, wpick, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("K", [21, 31, 33, 63, 95, 65, 97])
def test_select_equals_the_rule(pkg, synth, K, paired):
    c = case(K)
    words = synth.pack_2bit(c["batch"])
    with counted_context(pkg, synth, c) as g:
        for cv, seed in SETTINGS:
            want = expected(K, cv, seed, paired)
            got = g.select_reads(words, c["boffs"], target=TARGET, max_cv_pct=cv, seed=seed, paired=paired)
            assert_select(pkg, got, want, f"K={K} paired={paired} max_cv_pct={cv} seed={seed}")
        assert len(g.select_reads(words, c["boffs"][:1], target=TARGET)[0]) == 0
        with pytest.raises(pkg.SdtError) as e:
            g.select_reads(words, c["boffs"], target=0)
        assert e.value.code == pkg.SDT_EINVAL
        if paired:
            with pytest.raises(pkg.SdtError) as e:
                g.select_reads(words, c["boffs"][:-1], target=TARGET, paired=True)
            assert e.value.code == pkg.SDT_EINVAL and "odd" in str(e.value)
    # the case holds what it says: every class, medians below, at and above the target, the chimera caught at 60 % and not switched off
    off, on = expected(K, 0, 0, False)[0], expected(K, 60, 7, False)[0]
    assert set((off["verdict"] & 7).tolist()) == {rs.KEPT, rs.KEPT_DRAW, rs.DROPPED_DRAW, rs.SHORT}
    assert {1, 8, 16, 64, 512, 0} <= set(off["median"].tolist())
    assert off["verdict"][c["chimera"]] & 7 != rs.ABERRANT and on["verdict"][c["chimera"]] == rs.ABERRANT | rs.OWN_ABERRANT
    assert (on["verdict"] & 7 == rs.ABERRANT).sum() < len(on) // 4
    assert {63, 64, 65, 66} <= set(off["kmers"].tolist())
    if paired:
        p = expected(K, 60, 7, True)[0]
        assert ((p["verdict"] & 7 == rs.ABERRANT) & (p["verdict"] & rs.OWN_ABERRANT == 0)).any()      # dropped for the mate's sake
        assert ((p["kmers"] == 0) & (p["verdict"] & 7 != rs.SHORT)).any()                              # a short mate of a longer read
        assert (p["cov"][0::2] == p["cov"][1::2]).all() and ((p["verdict"][0::2] & 7) == (p["verdict"][1::2] & 7)).all()


# ---- 2. counts past 65 535 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [21, 63, 95, 65, 97])
def test_select_counts_past_65535(pkg, synth, K):
    """the poly-A reads of test_profile_counts_past_65535: medians past 65 535, and a read that is half poly-A, half tandem repeat,
    at a max_cv_pct where the saturated counts say "not aberrant" and the counts as they are would say "aberrant" """
    codes, offs = hot_input(K)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    L = int(offs[1])
    half = np.concatenate([codes[:L // 2], codes[1000 * L:1000 * L + L // 2]])
    batch, boffs = concat([codes[:L], half, codes[1000 * L:1001 * L], half[::-1] ^ 2])
    kc = rs.read_kmer_counts(batch, boffs, K, count)
    assert max(kc[1]) > 65535 and 0 < min(x for x in kc[1] if x) < 65535
    n, s1, s2 = len(kc[1]), sum(kc[1]), sum(x * x for x in kc[1])
    cv = next(p for p in range(1, 2000) if not rs.read_stats(kc[1], p)[2])
    assert 10000 * (n * s2 - s1 * s1) > cv * cv * s1 * s1, "the bound must tell saturated counts from unsaturated ones"
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        for p, target in ((cv, 70000), (cv - 1, 70000), (cv, 100), (0, 1)):
            want = rs.expect_select(batch, boffs, K, count, target, p, 3, kmer_counts=kc)
            assert_select(pkg, g.select_reads(synth.pack_2bit(batch), boffs, target=target, max_cv_pct=p, seed=3), want, f"K={K} cv={p} target={target}")
    want = rs.expect_select(batch, boffs, K, count, 70000, cv, 3, kmer_counts=kc)[0]
    assert want["median"][0] > 65535 and want["verdict"][1] == rs.KEPT
    assert rs.expect_select(batch, boffs, K, count, 70000, cv - 1, 3, kmer_counts=kc)[0]["verdict"][1] == rs.ABERRANT | rs.OWN_ABERRANT


# ---- 3. device-pointer form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_select_device_form_equals_host_form(pkg, synth, paired):
    import torch
    dev = torch.device("cuda:0")
    K, (cv, seed) = 31, SETTINGS[1]
    c = case(K)
    wpick, wkeep, wkept = expected(K, cv, seed, paired)
    words = synth.pack_2bit(c["batch"])
    n = len(c["boffs"]) - 1
    lens = np.diff(c["boffs"].astype(np.int64))
    maxlen = int(lens.max())
    with counted_context(pkg, synth, c) as g:
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(c["boffs"].view(np.int64)).to(dev)

        def run(max_read_len, with_keep=True):
            d_pick = torch.full((n, 4), -2, dtype=torch.int32, device=dev)
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev) if with_keep else None
            torch.cuda.synchronize()
            err, kept = None, None
            try:
                kept = g.select_reads_device(d_w, d_o, n, max_read_len, d_pick, d_keep, target=TARGET, max_cv_pct=cv, seed=seed, paired=paired)
            except pkg.SdtError as e:
                err = e
            pick = d_pick.cpu().numpy().view(np.uint32).copy().view(pkg.READ_PICK_DTYPE).reshape(-1)
            return err, kept, pick, d_keep.cpu().numpy() if with_keep else None

        err, kept, pick, keep = run(maxlen)
        assert err is None
        assert_select(pkg, (pick, keep, kept), (wpick, wkeep, wkept), "device form")
        err, kept, pick, _ = run(maxlen, with_keep=False)
        assert err is None and kept == wkept
        rs.assert_pick_equal(pick, wpick, "device form without keep")
        assert g.select_reads_device(d_w, d_o, 0, maxlen, None) == 0
        if not paired:
            # reads longer than promised: marked, verdict 4, SDT_EINVAL, every other record complete
            err, kept, pick, keep = run(maxlen - 1)
            assert err is not None and err.code == pkg.SDT_EINVAL and "longer" in str(err)
            longest = lens == maxlen
            assert 0 < longest.sum() < n // 4
            assert (pick["kmers"][longest] == pkg.COV_TOO_LONG).all() and (pick["verdict"][longest] == rs.SHORT).all()
            assert (pick["median"][longest] == 0).all() and (pick["cov"][longest] == 0).all() and (keep[longest] == 0).all()
            rs.assert_pick_equal(pick[~longest], wpick[~longest], "the other reads of the batch")
            assert keep[~longest].tolist() == wkeep[~longest].tolist()


# ---- 4. host batches in pieces ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True])
def test_select_host_batches_go_through_in_pieces(pkg, synth, monkeypatch, paired):
    """pieces of 7 reads (6 when paired: a piece never splits a pair) and of one read (one pair): a unit's id in the draw is the index
    of its first read in the whole batch, so the verdicts are those of the batch in one piece"""
    K, (cv, seed) = 31, SETTINGS[1]
    c = case(K)
    words = synth.pack_2bit(c["batch"])
    want = expected(K, cv, seed, paired)
    assert (want[0]["verdict"] & 7 == rs.KEPT_DRAW).sum() > 5 and (want[0]["verdict"] & 7 == rs.DROPPED_DRAW).sum() > 5
    with counted_context(pkg, synth, c) as g:
        for piece in ("7", "1"):
            monkeypatch.setenv("SDT_SEARCH_CHUNK", piece)
            got = g.select_reads(words, c["boffs"], target=TARGET, max_cv_pct=cv, seed=seed, paired=paired)
            assert_select(pkg, got, want, f"pieces of {piece} reads, paired={paired}")


# ---- 5. kept reads ----------------------------------------------------------------------------------------------------------------
def test_select_kept_reads_by_ordinal(pkg, synth):
    """a single-end batch with an odd number of reads, a paired stream pushed as two batches (base b / b + 1, stride 2) and another
    single batch: the pair range starts at an odd ordinal"""
    K, L, target, cv, seed = 31, 100, 3, 150, 11
    tx = synth.make_transcriptome(20, seed=5)
    (c1, o1), (c2, o2) = synth.sample_pairs(*tx, n_pairs=300, read_len=L, seed=6, err=0.004)
    ca, oa = synth.sample_reads(*tx, n_reads=301, read_len=140, seed=7, err=0.004, ragged=True)
    cb, ob_ = synth.sample_reads(*tx, n_reads=200, read_len=110, seed=8, err=0.004, ragged=True)
    na, np1, nb = len(oa) - 1, len(o1) - 1, len(ob_) - 1
    first, end = na, na + 2 * np1
    assert first & 1
    reads = [ca[int(oa[i]):int(oa[i + 1])] for i in range(na)]
    for i in range(np1):
        reads.append(c1[int(o1[i]):int(o1[i + 1])])
        reads.append(c2[int(o2[i]):int(o2[i + 1])])
    reads += [cb[int(ob_[i]):int(ob_[i + 1])] for i in range(nb)]
    codes, offs = concat(reads)
    total = len(reads)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    units = rs.ranged_units(range(total), [(first, end)])
    wpick, wkeep, wkept = rs.expect_select(codes, offs, K, count, target, cv, seed, units=units)
    assert set((wpick["verdict"] & 7).tolist()) == {rs.KEPT, rs.KEPT_DRAW, rs.DROPPED_DRAW, rs.ABERRANT, rs.SHORT}
    assert (wpick["cov"][first:end:2] == wpick["cov"][first + 1:end:2]).all() and (wpick["cov"][first:end] != wpick["median"][first:end]).any()
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for w, of, base, stride in ((synth.pack_2bit(ca), oa, 0, 1), (synth.pack_2bit(c1), o1, first, 2), (synth.pack_2bit(c2), o2, first + 1, 2),
                                    (synth.pack_2bit(cb), ob_, end, 1)):
            g.set_read_ordinal(base, stride)
            g.push_reads(w, of)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        pick, n, kept = g.select_kept_reads(total, [(first, end)], target=target, max_cv_pct=cv, seed=seed)
        assert n == total and kept == wkept
        rs.assert_pick_equal(pick, wpick, "kept reads")
        # no ranges: every read on its own
        spick, _, skept = rs.expect_select(codes, offs, K, count, target, cv, seed)
        pick, n, kept = g.select_kept_reads(total, [], target=target, max_cv_pct=cv, seed=seed)
        assert n == total and kept == skept
        rs.assert_pick_equal(pick, spick, "kept reads, no pair ranges")
        # the same range in two halves that touch, and one that reaches past the last read
        pick, n, kept = g.select_kept_reads(total, [(first, first + 100), (first + 100, end)], target=target, max_cv_pct=cv, seed=seed)
        assert kept == wkept
        rs.assert_pick_equal(pick, wpick, "kept reads, two ranges")
        # a larger array: the records past the last ordinal stay as they were
        big = np.full(total + 5, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_PICK_DTYPE)
        pick, n, kept = g.select_kept_reads(total + 5, [(first, end)], target=target, max_cv_pct=cv, seed=seed, out=big)
        assert n == total and (pick[total:].view(np.uint32) == 0xABABABAB).all()
        rs.assert_pick_equal(pick[:total], wpick, "kept reads into a larger array")
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_PICK_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.select_kept_reads(total - 1, [(first, end)], target=target, out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        # ranges that overlap, run backwards or hold half a pair: refused before anything is written
        full = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_PICK_DTYPE)
        for bad in ([(first, end), (end - 2, end + 2)], [(first, first + 3)], [(end, first)], [(first + 100, end), (first, first + 100)]):
            with pytest.raises(pkg.SdtError) as e:
                g.select_kept_reads(total, bad, target=target, out=full)
            assert e.value.code == pkg.SDT_EINVAL and "range" in str(e.value)
            assert (full.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.select_kept_reads(total, [(first, end)], target=0)
        assert e.value.code == pkg.SDT_EINVAL


def test_select_kept_pair_with_one_mate_in_hbm(pkg, synth):
    """only the read-1 file of a paired stream is kept: every pair is judged on that mate alone, its id the first mate's ordinal"""
    K, target, cv, seed = 31, 3, 0, 5
    codes, offs, words = small_input(synth, K)
    n = len(offs) - 1
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    ords = 2 * np.arange(n)
    want = rs.expect_select(codes, offs, K, count, target, cv, seed, ordinals=ords, units=[(int(u), [int(u)]) for u in ords])[0]
    assert {rs.KEPT_DRAW, rs.DROPPED_DRAW} <= set((want["verdict"] & 7).tolist())
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.set_read_ordinal(0, 2)
        g.push_reads(words, offs)
        g.finish_count()
        out = np.full(2 * n, 0xABABABAB, dtype=np.uint32).repeat(4).view(pkg.READ_PICK_DTYPE)
        pick, got_n, _ = g.select_kept_reads(2 * n, [(0, 2 * n)], target=target, max_cv_pct=cv, seed=seed, out=out)
        assert got_n == n
        rs.assert_pick_equal(pick[0:2 * n - 1:2], want[0::2], "the mates that are there")
        assert (np.ascontiguousarray(pick[1::2]).view(np.uint32) == 0xABABABAB).all()


# ---- 6. read-only -----------------------------------------------------------------------------------------------------------------
def test_select_leaves_the_table_alone(pkg, synth):
    K, L = 31, 150
    _, codes, offs = workload(synth, K, L, n_reads=2000)
    words = synth.pack_2bit(codes)

    def snapshot(g):
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        order = np.lexsort(keys.T[::-1])
        return [a[order].copy() for a in (keys, l, rf, cnt, first)]

    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_TRACK_FIRST | pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(words, offs)
        g.finish_count()
        hist0, lin0 = g.mark_and_hist()
        before = snapshot(g)
        kept_before = g.fetch_kept_batch(0)
        pick, keep, kept = g.select_reads(words, offs, target=4, max_cv_pct=100, seed=1)
        assert 0 < kept < len(keep) and (pick["verdict"] & 7 == rs.DROPPED_DRAW).any()
        g.select_kept_reads(len(offs) - 1, [], target=4)
        out_words, out_offs = g.compact_reads(words, offs, keep)
        assert len(out_offs) == kept + 1
        assert (words == synth.pack_2bit(codes)).all()                     # nor the caller's reads
        after = snapshot(g)
        for a, b in zip(before, after):
            assert a.shape == b.shape and (a == b).all()
        for a, b in zip(kept_before[:2], g.fetch_kept_batch(0)[:2]):
            assert (a == b).all()
        hist1, lin1 = g.mark_and_hist()
        assert lin1 == lin0 and (hist1 == hist0).all()


# ---- 7. state errors --------------------------------------------------------------------------------------------------------------
def assert_state_error(pkg, g, words, offs, code=None):
    import torch
    code = pkg.SDT_ESTATE if code is None else code
    n = len(offs) - 1
    d_pick = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_w = torch.from_numpy(words.view(np.int32)).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    calls = [lambda: g.select_reads(words, offs, target=5), lambda: g.select_kept_reads(n, [], target=5),
             lambda: g.select_reads_device(d_w, d_o, n, 100, d_pick, target=5)]
    for call in calls:
        with pytest.raises(pkg.SdtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert len(g.lib.sdt_gpu_last_error()) > 10
    # the compaction needs the context's stream and nothing else
    keep = (np.arange(n) % 3 == 0).astype(np.uint8)
    w, o = g.compact_reads(words, offs, keep)
    assert len(o) == int(keep.sum()) + 1 and int(o[-1]) == 100 * int(keep.sum())


def test_select_state_errors(pkg, synth):
    import torch
    K = 31
    codes, offs, words = small_input(synth, K)
    n = len(offs) - 1
    # pushed, not drained -- and fine again once drained; empty batches are fine in any state
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(words, offs)
        assert_state_error(pkg, g, words, offs)
        assert len(g.select_reads(words, offs[:1], target=5)[0]) == 0
        g.finish_count()
        pick, keep, kept = g.select_reads(words, offs, target=1 << 30)
        assert (pick["kmers"] == 100 - K + 1).all() and (pick["verdict"] == 0).all() and kept == n and keep.all()
        assert g.select_kept_reads(n, [], target=5)[1] == n
        # target 0, whatever the form
        for call in (lambda: g.select_reads(words, offs, target=0), lambda: g.select_kept_reads(n, [], target=0)):
            with pytest.raises(pkg.SdtError) as e:
                call()
            assert e.value.code == pkg.SDT_EINVAL and "target" in str(e.value)
        # counted from device memory and not drained
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        g.count_reads_device(d_w, len(words), d_o, n, 100)
        assert_state_error(pkg, g, words, offs)
        g.finish_count()
        assert g.select_reads(words, offs, target=1 << 30)[2] == n
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
            g.select_kept_reads(n, [], target=5)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
    # a contig index
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        assert_state_error(pkg, g, words, offs)
    # one shard of a sharded table
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.comm_init_shm(f"rss{os.getpid()}", 0, 1)
        assert_state_error(pkg, g, words, offs)


# ---- 8. the compaction ------------------------------------------------------------------------------------------------------------
def test_compact_equals_the_restatement(pkg):
    import torch
    dev = torch.device("cuda:0")
    codes, offs = length_mix()
    words = rs.pack_words(codes)
    n = len(offs) - 1
    # more than one workgroup of output words: the same mix twenty times over behind it, every third read dropped
    big_codes, big_offs = concat([codes[int(offs[r]):int(offs[r + 1])] for _ in range(20) for r in range(n)])
    big_keep = (np.arange(len(big_offs) - 1) % 3 != 1).astype(np.uint8)
    big_words = rs.pack_words(big_codes)
    big_want = rs.compact_by_bases(big_words, big_offs, big_keep)
    assert len(big_want[0]) > 600
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        for name, keep in keep_masks(offs).items():
            want_w, want_o = rs.expect_compact(words, offs, keep)
            got_w, got_o = g.compact_reads(words, offs, keep)
            assert got_o.tolist() == want_o.tolist(), f"host form, {name}: offsets"
            assert got_w.tolist() == want_w.tolist(), f"host form, {name}: words"
            d_k = torch.from_numpy(keep).to(dev)
            cap = len(want_w) + 3
            d_ow = torch.full((cap,), -1, dtype=torch.int32, device=dev)
            d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            nr, nw = g.compact_reads_device(d_w, d_o, n, d_k, d_ow, cap, d_oo)
            assert (nr, nw) == (len(want_o) - 1, len(want_w) - 4), f"device form, {name}"
            ow = d_ow.cpu().numpy().view(np.uint32)
            assert ow[:nw + 4].tolist() == want_w.tolist() and (ow[nw + 4:] == 0xFFFFFFFF).all(), f"device form, {name}: words"
            assert (ow[nw:nw + 4] == 0).all()
            assert d_oo.cpu().numpy().view(np.uint64)[:nr + 1].tolist() == want_o.tolist(), f"device form, {name}: offsets"
            # one word short of words + pad: SDT_EFULL with the needed size reported, nothing stored
            d_ow.fill_(-1)
            torch.cuda.synchronize()
            with pytest.raises(pkg.SdtError) as e:
                g.compact_reads_device(d_w, d_o, n, d_k, d_ow, nw + 3, d_oo)
            assert e.value.code == pkg.SDT_EFULL and e.value.needed == nw
            assert (d_ow.cpu().numpy() == -1).all()
            with pytest.raises(pkg.SdtError) as e:
                g.compact_reads(words, offs, keep, out_words_cap=nw + 3)
            assert e.value.code == pkg.SDT_EFULL and e.value.needed == nw
        got_w, got_o = g.compact_reads(big_words, big_offs, big_keep)
        assert got_o.tolist() == big_want[1].tolist() and got_w.tolist() == big_want[0].tolist(), "the long stream"
        # no reads at all
        got_w, got_o = g.compact_reads(np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        assert got_o.tolist() == [0] and got_w.tolist() == [0, 0, 0, 0]


# ---- 9. select, compact, count again: nothing crosses to the host ------------------------------------------------------------------
@pytest.mark.parametrize("K", [31, 63])
def test_normalised_reads_count_like_the_oracle(pkg, synth, K):
    import torch
    dev = torch.device("cuda:0")
    L, target, cv, seed = (150 if K == 31 else 250), 6, 200, 9
    _, codes, offs = workload(synth, K, L, n_reads=3000)
    n = len(offs) - 1
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    wpick, wkeep, wkept = rs.expect_select(codes, offs, K, table_counts(node_dict_oracle(o)), target, cv, seed)
    assert n // 10 < wkept < n - n // 10 and (wpick["verdict"] & 7 == rs.DROPPED_DRAW).sum() > n // 10
    kcodes, koffs = concat([codes[int(offs[r]):int(offs[r + 1])] for r in range(n) if wkeep[r]])
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_pick = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        a.count_reads_device(d_w, len(words), d_o, n, L)
        assert a.finish_count() == (o.kmers_in_reads(), o.node_count())
        assert a.select_reads_device(d_w, d_o, n, L, d_pick, d_keep, target=target, max_cv_pct=cv, seed=seed) == wkept
        nr, nw = a.compact_reads_device(d_w, d_o, n, d_keep, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, L)
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want


# ---- 10. the host program ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se100_k23_p8", "pe150_k31_p8", "se150_k47_p4_63mer"])
def test_sdt_kmers_normalize_cli(pkg, tmp_path, name):
    info = gu.load_case(name)
    K = pkg.clamp_K(info["K"], gu.VARIANT_MAXK[info["variant"]])
    cfg = materialise(info, tmp_path)
    codes, offs = gu.case_reads(info)
    n = len(offs) - 1
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    ranges = [(0, n)] if info["kind"] == "pe" else []
    units = rs.ranged_units(range(n), ranges)
    pick, keep, kept = rs.expect_select(codes, offs, K, table_counts(node_dict_oracle(o)), 4, 150, 21, units=units)
    assert (pick["verdict"] & 7 == rs.DROPPED_DRAW).sum() > n // 20 and (pick["verdict"] & 7 == rs.KEPT_DRAW).sum() > n // 20
    pick_txt, pairs_txt, single_txt, tally = rs.cli_texts(codes, offs, pick, keep, ranges)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    opts = ["-s", cfg, "-K", str(info["K"]), "-p", "4", "--max-k", str(gu.VARIANT_MAXK[info["variant"]])]
    outs = {}
    for run in ("out", "again"):
        r = subprocess.run([exe, "normalize"] + opts + ["--target", "4", "--max-cv", "150", "--seed", "21", "-o", str(tmp_path / run)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs[run] = [(tmp_path / f"{run}.{ext}").read_bytes() for ext in ("readPick", "norm.pairs.fa", "norm.single.fa")]
        last = [x for x in r.stdout.splitlines() if "reads kept" in x]
        assert len(last) == 1
        assert tuple(int(x) for x in last[0].replace("(", " ").replace(",", " ").split() if x.isdigit()) == tally
    assert outs["out"] == outs["again"], "the same seed twice gives the same files"
    for got, text, ext in zip(outs["out"], (pick_txt, pairs_txt, single_txt), ("readPick", "norm.pairs.fa", "norm.single.fa")):
        assert got.decode() == text, f"{name}: out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    assert (len(pairs_txt) > 0) == (info["kind"] == "pe") and (len(single_txt) > 0) == (info["kind"] != "pe")
    if info["kind"] == "pe":
        # the outputs are a library again: p= for the pairs, f= for the singles
        cfg2 = tmp_path / "norm.cfg"
        cfg2.write_text(f"max_rd_len={info['max_rd_len']}\n[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\np={tmp_path / 'out.norm.pairs.fa'}\n"
                        f"f={tmp_path / 'out.norm.single.fa'}\n")
        r = subprocess.run([exe, "profile", "-s", str(cfg2), "-K", str(info["K"]), "-p", "4", "--max-k", str(gu.VARIANT_MAXK[info["variant"]]),
                            "-o", str(tmp_path / "second")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert len((tmp_path / "second.readCov").read_text().splitlines()) == kept
        assert r.stdout.splitlines()[0].split()[0] == str(kept)
