"""GPU (-m gpu): sdt_gpu_trim_reads, sdt_gpu_compact_trimmed and their siblings against the Python restatement of the rule and of the
ranged compaction (read_trim_util.py) on the oracle's node table.  Expectations never come from the library under test: counts are the
oracle's (oracle_binding.Oracle.export), the rule is plain Python (with read_correct_util for the flag), and every output is compared
for exact equality."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import golden_util as gu
import read_correct_util as rc
import read_trim_util as rt
from read_correct_util import table_counts
from test_kmer_search import hot_input, keys_to_int, materialise, node_dict_oracle, small_input, workload
from test_read_correct import concat, counted_context, plant
from test_read_select_host import length_mix
from test_read_trim_host import range_sets

pytestmark = pytest.mark.gpu

COPIES = (1, 3, 8, 64)
LONG_COPIES = 4
PIECE = 3000                                            # the long transcript is counted in pieces that pass 1 takes: PIECE + K - 1 bases
assert PIECE + 97 - 1 <= 4059                           # ... at every K of this file (SDT_PASS1_MAX_READ_LEN)


def settings(K):
    """(min_count, min_cov, min_len, flags)"""
    return ((2, 0, 0, 0), (2, 2, 0, 0), (2, 0, K + 30, 0), (4, 0, 0, 0), (2, 0, 0, rt.CORRECTED), (0, 0, 0, 0))


def revcomp(r):
    return r[::-1] ^ 2


@functools.lru_cache(maxsize=None)
def case(K, seed=None):
    """the counted input -- four transcripts of K + 140 bases counted 1, 3, 8 and 64 times and one of K + 8 400 bases counted 4 times
    (in pieces of 3 000 k-mers: every k-mer of it in exactly one piece) -- the oracle's table for it, and the batch to trim; what each
    group of reads is there for is said where it is made.  Built once per K and left unchanged.  seed: another draw of the same
    generator (other transcripts, other reads), for the tests that need more reads."""
    rng = np.random.default_rng(5000 + K if seed is None else seed)
    Lt = K + 140
    tx = [rng.integers(0, 4, size=Lt, dtype=np.uint8) for _ in COPIES]
    long_tx = rng.integers(0, 4, size=K + 8400, dtype=np.uint8)
    pieces = [long_tx[s:min(s + PIECE + K - 1, len(long_tx))] for s in range(0, len(long_tx) - K + 1, PIECE)]
    counted, coffs = concat([t for t, c in zip(tx, COPIES) for _ in range(c)] + [p for p in pieces for _ in range(LONG_COPIES)])
    o = ob.Oracle(K, nsets=5)
    o.add_reads(counted, coffs)
    count = table_counts(node_dict_oracle(o))
    reads, tags = [], {}

    def add(tag, r, flip=False):
        tags.setdefault(tag, []).append(len(reads))
        reads.append(revcomp(r) if flip else r.copy())

    # clean reads around the 64-k-mer strip and ballot boundary, either strand, of every transcript (those of tx[0] are counted once)
    for ti, t in enumerate(tx):
        for L in (K - 1, K, K + 1, K + 62, K + 63, K + 64, K + 65):
            for s in rng.integers(0, Lt - L + 1, size=2).tolist():
                add("once" if ti == 0 else "clean", t[s:s + L], flip=bool(s & 1))
    # one substitution: head, interior and tail runs
    L = K + 100
    base = tx[2][7:7 + L]
    for p in (0, K - 1, K, L // 2, L - K, L - 1):
        add("one", plant(base, p), flip=bool(p & 1))
    # two substitutions 1, K - 1, K and K + 1 apart
    for gap in (1, K - 1, K, K + 1):
        add("two", plant(tx[3][3:3 + L], 30, 30 + gap))
    # a full-length read with one substitution in the very middle: two stretches of equal length, the first must win
    assert Lt & 1
    add("tie", plant(tx[2], (Lt - 1) // 2))
    add("tie", plant(tx[3], (Lt - 1) // 2), flip=True)
    # stretches that end, and stretches that begin, at k-mers 63, 64, 65
    for e in (63, 64, 65):
        add("ends", plant(tx[3], e + K - 1))
        add("begins", plant(tx[2], e - 1))
    # ... and one that begins at k-mer 64 and ends at 128, the longest of its read (138 + K k-mers)
    add("chunk", plant(long_tx[500:500 + 137 + 2 * K], 63, 128 + K - 1))
    # two stretches that both cover fewer than K + 30 bases: dropped only by that min_len
    add("brief", plant(tx[3][5:5 + K + 45], K + 10))
    # a junction chimera, a read the table does not know
    add("chimera", np.concatenate([tx[2][-(K + 20):], tx[3][:K + 20]]))
    add("unknown", rng.integers(0, 4, size=K + 30, dtype=np.uint8))
    # 4 200 and 8 300 k-mers with a few substitutions: the 2- and 1-wave geometries
    add("long", plant(long_tx[50:50 + 4200 + K - 1], 0, 700, 700 + K, 2500, 2503, 4100 + K))
    add("long", plant(long_tx[20:20 + 8300 + K - 1], 64 + K - 1, 4096, 6000, 6000 + K - 1, 8299 + K - 1), flip=True)
    add("long", long_tx[100:100 + 4200 + K - 1])
    order = rng.permutation(len(reads))                 # long reads next to short ones
    where = np.argsort(order)
    reads = [reads[i] for i in order]
    tags = {t: [int(where[i]) for i in ix] for t, ix in tags.items()}
    batch, boffs = concat(reads)
    kc = rt.read_kmer_counts(batch, boffs, K, count)
    return dict(K=K, counted=counted, coffs=coffs, count=count, batch=batch, boffs=boffs, kc=kc, tags=tags,
                oracle=(o.kmers_in_reads(), o.node_count()))


@functools.lru_cache(maxsize=None)
def expected(K, params):
    c = case(K)
    return rt.expect_trim(c["batch"], c["boffs"], K, c["count"], params, kmer_counts=c["kc"])


def assert_trim(pkg, got, want, what):
    trim, keep, kept = got
    wtrim, wkeep, wkept = want
    assert trim.dtype == pkg.READ_TRIM_DTYPE
    rt.assert_trim_equal(trim, wtrim, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [21, 31, 33, 63, 95, 65, 97])
def test_trim_equals_the_rule(pkg, synth, K):
    c = case(K)
    words = synth.pack_2bit(c["batch"])
    with counted_context(pkg, synth, c) as g:
        for p in settings(K):
            got = g.trim_reads(words, c["boffs"], *p)
            assert_trim(pkg, got, expected(K, p), f"K={K} (min_count, min_cov, min_len, flags)={p}")
        assert len(g.trim_reads(words, c["boffs"][:1])[0]) == 0
        with pytest.raises(pkg.SdtError) as e:
            g.trim_reads(words, c["boffs"], flags=2)
        assert e.value.code == pkg.SDT_EINVAL and "flags" in str(e.value)
    # the case holds what it says
    plain, gated, minlen, four, flag, zero = (expected(K, p)[0] for p in settings(K))
    tags = c["tags"]
    assert set(plain["verdict"].tolist()) | set(gated["verdict"].tolist()) == {rt.WHOLE, rt.GATED, rt.TRIMMED, rt.DROPPED, rt.SHORT}
    assert (zero["verdict"][zero["kmers"] > 0] == rt.WHOLE).all() and (zero["weak"] == 0).all()
    assert {63, 64, 65, 66, 4200, 8300} <= set(plain["kmers"].tolist()) and (plain["verdict"] == rt.SHORT).sum() >= 4
    for r in tags["tie"]:                               # two stretches of (141 - K) / 2 k-mers around K weak ones: the first is kept
        n = K + 140 - K + 1
        assert tuple(plain[r])[:2] == (n, K) and tuple(plain[r])[3:] == (0, (n - K) // 2 + K - 1, rt.TRIMMED)
        assert [x >= 2 for x in c["kc"][r]] == [True] * ((n - K) // 2) + [False] * K + [True] * ((n - K) // 2)
    assert (gated["verdict"][tags["once"]] == rt.GATED).sum() >= 6 and (plain["verdict"][tags["once"]] == rt.DROPPED).sum() >= 6
    whole_by_flag = (flag["verdict"] == rt.WHOLE) & (plain["verdict"] != rt.WHOLE)
    assert whole_by_flag.sum() >= 5 and whole_by_flag[tags["tie"]].all()
    assert (flag["weak"] == plain["weak"]).all() and (flag["median"] == plain["median"]).all()
    dropped_by_min_len = (minlen["verdict"] == rt.DROPPED) & (plain["verdict"] == rt.TRIMMED)
    assert dropped_by_min_len.sum() >= 2 and dropped_by_min_len[tags["brief"]].all()
    assert (four["verdict"] != plain["verdict"]).any()
    starts, ends = set(plain["start"].tolist()), set((plain["start"] + plain["len"] - (K - 1)).tolist())
    assert {63, 64, 65} <= starts and {63, 64, 65, 128} <= ends
    r = tags["chunk"][0]
    assert tuple(plain[r])[3:] == (64, 64 + K - 1, rt.TRIMMED)
    assert (plain["verdict"][tags["chimera"]] == rt.TRIMMED).all() and (plain["verdict"][tags["unknown"]] == rt.DROPPED).all()
    assert sorted(plain["kmers"][tags["long"]].tolist()) == [4200, 4200, 8300] and rt.TRIMMED in plain["verdict"][tags["long"]].tolist()


# ---- 2. counts past 65 535 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [21, 63, 95, 65, 97])
def test_trim_counts_past_65535(pkg, synth, K):
    """the poly-A and tandem-repeat reads of test_profile_counts_past_65535 and a read that is half one, half the other: with min_count
    between the two counts and above 65 535 it is cut to its poly-A half -- counts saturated at 65 535 would call every k-mer weak"""
    codes, offs = hot_input(K)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    L = int(offs[1])
    half = np.concatenate([codes[:L // 2], codes[1000 * L:1000 * L + L // 2]])
    batch, boffs = concat([codes[:L], half, codes[1000 * L:1001 * L], revcomp(half)])
    kc = rt.read_kmer_counts(batch, boffs, K, count)
    hot, rep = kc[0][0], max(kc[2])
    min_count = 65536 + (hot - 65536) // 2
    assert rep < 65535 < min_count < hot
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        for p in ((min_count, 0, 0, 0), (min_count, 0, 0, rt.CORRECTED), (hot, 0, 0, 0), (hot + 1, 0, 0, 0), (min_count, hot + 1, 0, 0), (2, 0, 0, 0)):
            want = rt.expect_trim(batch, boffs, K, count, p, kmer_counts=kc)
            assert_trim(pkg, g.trim_reads(synth.pack_2bit(batch), boffs, *p), want, f"K={K} params={p}")
    want = rt.expect_trim(batch, boffs, K, count, (min_count, 0, 0, 0), kmer_counts=kc)[0]
    nh = sum(x == hot for x in kc[1])                   # (the repeat begins with an A: the poly-A half reaches one base into it)
    assert L // 2 - K + 1 <= nh <= L // 2 - K + 2 and kc[1][:nh] == [hot] * nh
    assert tuple(want[0]) == (L - K + 1, 0, hot, 0, L, rt.WHOLE) and want["verdict"][2] == rt.DROPPED
    assert tuple(want[1]) == (L - K + 1, L - K + 1 - nh, want["median"][1], 0, nh + K - 1, rt.TRIMMED)
    assert tuple(want[3])[3:] == (L - (nh + K - 1), nh + K - 1, rt.TRIMMED)
    assert rt.expect_trim(batch, boffs, K, count, (hot + 1, 0, 0, 0), kmer_counts=kc)[0]["verdict"].tolist() == [rt.DROPPED] * 4


# ---- 3. device-pointer form -------------------------------------------------------------------------------------------------------
def test_trim_device_form_equals_host_form(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    K = 31
    p = settings(K)[4]
    c = case(K)
    # (without the three long reads: the promise below is about the reads of K + 140 bases)
    short = [r for r in range(len(c["boffs"]) - 1) if r not in c["tags"]["long"]]
    batch, boffs = concat([c["batch"][int(c["boffs"][r]):int(c["boffs"][r + 1])] for r in short])
    kc = [c["kc"][r] for r in short]
    want = rt.expect_trim(batch, boffs, K, c["count"], p, kmer_counts=kc)
    words = synth.pack_2bit(batch)
    n = len(boffs) - 1
    lens = np.diff(boffs.astype(np.int64))
    maxlen = int(lens.max())
    with counted_context(pkg, synth, c) as g:
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(boffs.view(np.int64)).to(dev)

        def run(max_read_len, with_keep=True):
            d_trim = torch.full((n, 6), -2, dtype=torch.int32, device=dev)
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev) if with_keep else None
            torch.cuda.synchronize()
            err, kept = None, None
            try:
                kept = g.trim_reads_device(d_w, d_o, n, max_read_len, d_trim, d_keep, *p)
            except pkg.SdtError as e:
                err = e
            trim = d_trim.cpu().numpy().view(np.uint32).copy().view(pkg.READ_TRIM_DTYPE).reshape(-1)
            return err, kept, trim, d_keep.cpu().numpy() if with_keep else None

        err, kept, trim, keep = run(maxlen)
        assert err is None
        assert_trim(pkg, (trim, keep, kept), want, "device form")
        assert_trim(pkg, g.trim_reads(words, boffs, *p), want, "host form")
        err, kept, trim, _ = run(maxlen, with_keep=False)
        assert err is None and kept == want[2]
        rt.assert_trim_equal(trim, want[0], "device form without keep")
        assert g.trim_reads_device(d_w, d_o, 0, maxlen, None) == 0
        # reads longer than promised: marked, verdict 4, keep 0, SDT_EINVAL, every other record complete
        err, kept, trim, keep = run(maxlen - 1)
        assert err is not None and err.code == pkg.SDT_EINVAL and "longer" in str(err)
        longest = lens == maxlen
        assert 0 < longest.sum() < n // 4
        wlong = rt.expect_trim(batch, boffs, K, c["count"], p, kmer_counts=kc, max_read_len=maxlen - 1)
        assert (wlong[0]["kmers"][longest] == pkg.COV_TOO_LONG).all() and (wlong[0]["verdict"][longest] == rt.SHORT).all()
        assert (wlong[0]["len"][longest] == 0).all()
        rt.assert_trim_equal(trim, wlong[0], "a promise one base short")
        assert keep.tolist() == wlong[1].tolist() and (keep[longest] == 0).all()
        rt.assert_trim_equal(trim[~longest], want[0][~longest], "the other reads of the batch")


def test_trim_host_batches_go_through_in_pieces(pkg, synth, monkeypatch):
    K = 31
    p = settings(K)[4]
    c = case(K)
    words = synth.pack_2bit(c["batch"])
    with counted_context(pkg, synth, c) as g:
        for piece in ("7", "1"):
            monkeypatch.setenv("SDT_SEARCH_CHUNK", piece)
            assert_trim(pkg, g.trim_reads(words, c["boffs"], *p), expected(K, p), f"pieces of {piece} reads")


# ---- 4. kept reads ----------------------------------------------------------------------------------------------------------------
def test_trim_kept_reads_by_ordinal(pkg, synth):
    """a single-end batch with an odd number of reads, a paired stream pushed as two batches (base b / b + 1, stride 2), a gap of
    ordinals that no read has, and another single batch"""
    K, L, gap = 31, 100, 7
    p = (2, 3, K + 25, rt.CORRECTED)
    tx = synth.make_transcriptome(20, seed=5)
    (c1, o1), (c2, o2) = synth.sample_pairs(*tx, n_pairs=150, read_len=L, seed=6, err=0.01)
    ca, oa = synth.sample_reads(*tx, n_reads=151, read_len=140, seed=7, err=0.01, ragged=True)
    cb, ob_ = synth.sample_reads(*tx, n_reads=100, read_len=110, seed=8, err=0.01, ragged=True)
    na, np1, nb = len(oa) - 1, len(o1) - 1, len(ob_) - 1
    first, end = na, na + 2 * np1
    reads = [ca[int(oa[i]):int(oa[i + 1])] for i in range(na)]
    for i in range(np1):
        reads.append(c1[int(o1[i]):int(o1[i + 1])])
        reads.append(c2[int(o2[i]):int(o2[i + 1])])
    reads += [cb[int(ob_[i]):int(ob_[i + 1])] for i in range(nb)]
    codes, offs = concat(reads)
    ords = np.concatenate([np.arange(end), end + gap + np.arange(nb)])
    total = int(ords[-1]) + 1
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    dense, _, wkept = rt.expect_trim(codes, offs, K, table_counts(node_dict_oracle(o)), p)
    assert set(dense["verdict"].tolist()) == {rt.WHOLE, rt.GATED, rt.TRIMMED, rt.DROPPED, rt.SHORT}
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        for w, of, base, stride in ((synth.pack_2bit(ca), oa, 0, 1), (synth.pack_2bit(c1), o1, first, 2), (synth.pack_2bit(c2), o2, first + 1, 2),
                                    (synth.pack_2bit(cb), ob_, end + gap, 1)):
            g.set_read_ordinal(base, stride)
            g.push_reads(w, of)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        kept_before = [g.fetch_kept_batch(i) for i in range(4)]
        out = np.full(total + 5, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_TRIM_DTYPE)
        trim, n, kept = g.trim_kept_reads(total + 5, *p, out=out)
        assert n == len(ords) and kept == wkept
        rt.assert_trim_equal(trim[ords], dense, "kept reads by ordinal")
        untouched = np.ones(total + 5, dtype=bool)
        untouched[ords] = False
        assert untouched.sum() == gap + 5 and (np.ascontiguousarray(trim[untouched]).view(np.uint32) == 0xABABABAB).all()
        # the kept reads are as they were
        for before, i in zip(kept_before, range(4)):
            after = g.fetch_kept_batch(i)
            assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and before[2:] == after[2:]
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_TRIM_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.trim_kept_reads(total - 1, *p, out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.trim_kept_reads(total, flags=4)
        assert e.value.code == pkg.SDT_EINVAL


def assert_state_error(pkg, g, words, offs, code=None):
    import torch
    code = pkg.SDT_ESTATE if code is None else code
    n = len(offs) - 1
    d_trim = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
    d_w = torch.from_numpy(words.view(np.int32)).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    calls = [lambda: g.trim_reads(words, offs), lambda: g.trim_kept_reads(n), lambda: g.trim_reads_device(d_w, d_o, n, 100, d_trim)]
    for call in calls:
        with pytest.raises(pkg.SdtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert len(g.lib.sdt_gpu_last_error()) > 10
    # the compaction needs the context's stream and nothing else
    trim = np.zeros(n, dtype=pkg.READ_TRIM_DTYPE)
    trim["start"], trim["len"] = 10, np.where(np.arange(n) % 3 == 0, 60, 0)
    w, o = g.compact_trimmed(words, offs, trim)
    assert len(o) == (n + 2) // 3 + 1 and int(o[-1]) == 60 * ((n + 2) // 3)


def test_trim_state_errors(pkg, synth):
    import torch
    K = 31
    codes, offs, words = small_input(synth, K)
    n = len(offs) - 1
    # pushed, not drained -- and fine again once drained; empty batches are fine in any state
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(words, offs)
        assert_state_error(pkg, g, words, offs)
        assert len(g.trim_reads(words, offs[:1])[0]) == 0
        g.finish_count()
        trim, keep, kept = g.trim_reads(words, offs, min_count=1)
        assert (trim["kmers"] == 100 - K + 1).all() and (trim["verdict"] == 0).all() and (trim["len"] == 100).all() and kept == n and keep.all()
        assert g.trim_kept_reads(n)[1] == n
        # counted from device memory and not drained
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(offs.view(np.int64)).cuda()
        g.count_reads_device(d_w, len(words), d_o, n, 100)
        assert_state_error(pkg, g, words, offs)
        g.finish_count()
        assert g.trim_reads(words, offs, min_count=1)[2] == n
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
            g.trim_kept_reads(n)
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
    # a contig index
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        assert_state_error(pkg, g, words, offs)
    # one shard of a sharded table
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.comm_init_shm(f"rts{os.getpid()}", 0, 1)
        assert_state_error(pkg, g, words, offs)


def test_trim_refuses_reads_past_the_strip_on_the_host(pkg, synth):
    """16 384 k-mers fit the wavefront's strip of LDS, 16 385 do not: SDT_EINVAL from the host before any launch, no record written"""
    import torch
    K = 31
    c = case(K)
    rng = np.random.default_rng(77)
    fits = rng.integers(0, 4, size=16384 + K - 1, dtype=np.uint8)
    batch, boffs = concat([c["batch"][:int(c["boffs"][3])], fits])
    too_long, toffs = concat([c["batch"][:int(c["boffs"][3])], np.concatenate([fits, fits[:1]])])
    with counted_context(pkg, synth, c, flags=0) as g:
        trim, keep, kept = g.trim_reads(synth.pack_2bit(batch), boffs)
        want = rt.expect_trim(batch, boffs, K, c["count"], (2, 0, 0, 0))
        assert_trim(pkg, (trim, keep, kept), want, "a read of 16 384 k-mers")
        assert tuple(trim[-1]) == (16384, 16384, 0, 0, 0, rt.DROPPED)
        with pytest.raises(pkg.SdtError) as e:
            g.trim_reads(synth.pack_2bit(too_long), toffs)
        assert e.value.code == pkg.SDT_EINVAL and "do not fit the per-wavefront LDS strip" in str(e.value) and "16385 k-mers" in str(e.value)
        words = synth.pack_2bit(too_long)
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(toffs.view(np.int64)).cuda()
        d_trim = torch.full((len(toffs) - 1, 6), -2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.SdtError) as e:
            g.trim_reads_device(d_w, d_o, len(toffs) - 1, 16385 + K - 1, d_trim)
        assert e.value.code == pkg.SDT_EINVAL and "do not fit the per-wavefront LDS strip" in str(e.value)
        assert (d_trim.cpu().numpy() == -2).all()
    # kept reads that long: refused likewise
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        g.push_reads(synth.pack_2bit(c["counted"]), c["coffs"])
        g.finish_count()
        g.set_read_ordinal(0, 1)                        # (the counted reads took the ordinals before: out[] below holds these two only)
        g.keep_reads(synth.pack_2bit(too_long), toffs)
        out = np.full(len(toffs) - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_TRIM_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.trim_kept_reads(len(toffs) - 1, out=out)
        assert e.value.code == pkg.SDT_EINVAL and "do not fit the per-wavefront LDS strip" in str(e.value)
        assert (out.view(np.uint32) == 0xABABABAB).all()


# ---- 5. the compaction ------------------------------------------------------------------------------------------------------------
def test_compact_trimmed_equals_the_restatement(pkg):
    import torch
    dev = torch.device("cuda:0")
    codes, offs = length_mix()
    words = rt.pack_words(codes)
    n = len(offs) - 1
    # more than one workgroup of output words: the same mix forty times over, ranges that start in mid-word
    big_codes, big_offs = concat([codes[int(offs[r]):int(offs[r + 1])] for _ in range(40) for r in range(n)])
    big_trim = np.tile(range_sets(offs)["random ranges"], 40)
    big_words = rt.pack_words(big_codes)
    big_want = rt.compact_trimmed_by_bases(big_words, big_offs, big_trim)
    assert len(big_want[0]) > 512
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        d_w = torch.from_numpy(words.view(np.int32)).to(dev)
        d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
        sets = range_sets(offs)
        wild = sets["random ranges"].copy()             # ranges past their reads: only the device form takes them, and clamps
        wild["start"][3], wild["len"][4], wild["len"][n - 1] = 1000, 1000, 0xFFFFFFFF
        wild["start"][7], wild["len"][7] = 0xFFFFFFFF, 0xFFFFFFFF
        for name, trim in list(sets.items()) + [("ranges past the reads", wild)]:
            want_w, want_o = rt.expect_compact_trimmed(words, offs, trim)
            if name != "ranges past the reads":
                got_w, got_o = g.compact_trimmed(words, offs, trim)
                assert got_o.tolist() == want_o.tolist(), f"host form, {name}: offsets"
                assert got_w.tolist() == want_w.tolist(), f"host form, {name}: words"
            else:
                with pytest.raises(pkg.SdtError) as e:
                    g.compact_trimmed(words, offs, trim)
                assert e.value.code == pkg.SDT_EINVAL and "keeps" in str(e.value)
            d_t = torch.from_numpy(trim.view(np.int32).reshape(n, 6)).to(dev)
            cap = len(want_w) + 3
            d_ow = torch.full((cap,), -1, dtype=torch.int32, device=dev)
            d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            nr, nw = g.compact_trimmed_device(d_w, d_o, n, d_t, d_ow, cap, d_oo)
            assert (nr, nw) == (len(want_o) - 1, len(want_w) - 4), f"device form, {name}"
            ow = d_ow.cpu().numpy().view(np.uint32)
            assert ow[:nw + 4].tolist() == want_w.tolist() and (ow[nw + 4:] == 0xFFFFFFFF).all(), f"device form, {name}: words"
            assert (ow[nw:nw + 4] == 0).all()
            assert d_oo.cpu().numpy().view(np.uint64)[:nr + 1].tolist() == want_o.tolist(), f"device form, {name}: offsets"
            # one word short of words + pad: SDT_EFULL with the needed size reported, nothing stored
            d_ow.fill_(-1)
            torch.cuda.synchronize()
            with pytest.raises(pkg.SdtError) as e:
                g.compact_trimmed_device(d_w, d_o, n, d_t, d_ow, nw + 3, d_oo)
            assert e.value.code == pkg.SDT_EFULL and e.value.needed == nw
            assert (d_ow.cpu().numpy() == -1).all()
            if name != "ranges past the reads":
                with pytest.raises(pkg.SdtError) as e:
                    g.compact_trimmed(words, offs, trim, out_words_cap=nw + 3)
                assert e.value.code == pkg.SDT_EFULL and e.value.needed == nw
        # start + len one base past the read: SDT_EINVAL from the host form
        over = sets["whole reads"].copy()
        over["start"][5] += 1
        with pytest.raises(pkg.SdtError) as e:
            g.compact_trimmed(words, offs, over)
        assert e.value.code == pkg.SDT_EINVAL
        got_w, got_o = g.compact_trimmed(big_words, big_offs, big_trim)
        assert got_o.tolist() == big_want[1].tolist() and got_w.tolist() == big_want[0].tolist(), "the long stream"
        # no reads at all
        got_w, got_o = g.compact_trimmed(np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=pkg.READ_TRIM_DTYPE))
        assert got_o.tolist() == [0] and got_w.tolist() == [0, 0, 0, 0]


# ---- 6. correct, trim, compact, count again: nothing crosses to the host -----------------------------------------------------------
@pytest.mark.parametrize("K", [31, 63])
def test_corrected_trimmed_reads_count_like_the_oracle(pkg, synth, K):
    import torch
    dev = torch.device("cuda:0")
    L, min_count, min_len = (150 if K == 31 else 250), 2, K + 20
    _, codes, offs = workload(synth, K, L, n_reads=3000)
    n = len(offs) - 1
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    wfix, corrected, wedits = rc.expect_correct(codes, offs, K, count, min_count)
    wtrim, _, wkept = rt.expect_trim(corrected, offs, K, count, (min_count, 0, min_len, 0))
    assert len(wedits) > 50 and (wtrim["verdict"] == rt.TRIMMED).sum() > 50 and (wtrim["verdict"] == rt.DROPPED).sum() > 0
    kcodes, koffs = concat(rt.trimmed_reads(corrected, offs, wtrim))
    o2 = ob.Oracle(K, nsets=5)
    o2.add_reads(kcodes, koffs)
    want = {k: (v[0], v[1] & 0xFFFFFF, v[2]) for k, v in node_dict_oracle(o2).items()}
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_cw = torch.zeros_like(d_w)
    d_fix = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_trim = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_flag = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 16) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
        a.count_reads_device(d_w, len(words), d_o, n, L)
        assert a.finish_count() == (o.kmers_in_reads(), o.node_count())
        assert a.correct_reads_device(d_w, len(words), d_o, n, L, min_count, d_fix, d_cw) == len(wedits)
        assert a.trim_reads_device(d_cw, d_o, n, L, d_trim, None, min_count, 0, min_len, 0) == wkept
        assert a.trim_reads_device(d_w, d_o, n, L, d_flag, None, min_count, 0, min_len, rt.CORRECTED) == wkept
        assert torch.equal(d_trim[:, 3:], d_flag[:, 3:]), "the flag on the reads as they came == no flag on the corrected reads"
        nr, nw = a.compact_trimmed_device(d_cw, d_o, n, d_trim, d_ow, len(words), d_oo)
        assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
        b.count_reads_device(d_ow, nw + 4, d_oo, nr, L)
        assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
        keys, l, rf, cnt = b.export_nodes()[:4]
    got = {k: (int(x), int(y) & 0xFFFFFF, int(z)) for k, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
    assert len(got) == len(want) and got == want
    rt.assert_trim_equal(d_trim.cpu().numpy().view(np.uint32).copy().view(pkg.READ_TRIM_DTYPE).reshape(-1), wtrim, "the corrected reads trimmed")


# ---- 7. the host program ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("correct", [False, True])
@pytest.mark.parametrize("name,as_fasta", [("pe150_k31_p8", False), ("se100_k23_p8", True)])
def test_sdt_kmers_trim_cli(pkg, tmp_path, name, as_fasta, correct):
    info = gu.load_case(name)
    K = pkg.clamp_K(info["K"], gu.VARIANT_MAXK[info["variant"]])
    codes, offs = gu.case_reads(info)
    n = len(offs) - 1
    if as_fasta:                                        # the same reads as an f= file
        letters = np.frombuffer(rt.LETTERS.encode(), dtype=np.uint8)[codes].tobytes().decode()
        (tmp_path / "reads.fa").write_text("".join(f">r{r}\n{letters[int(offs[r]):int(offs[r + 1])]}\n" for r in range(n)))
        cfg = str(tmp_path / "lib.cfg")
        with open(cfg, "w") as f:
            f.write(f"max_rd_len={info['max_rd_len']}\n[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nf={tmp_path / 'reads.fa'}\n")
    else:
        cfg = materialise(info, tmp_path)
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    count = table_counts(node_dict_oracle(o))
    ranges = [(0, n)] if info["kind"] == "pe" else []
    min_count, min_cov, min_len = 3, 2, K + 30
    trim = rt.expect_trim(codes, offs, K, count, (min_count, min_cov, min_len, rt.CORRECTED if correct else 0))[0]
    written, edits_txt = codes, None
    if correct:
        fix, written, edits = rc.expect_correct(codes, offs, K, count, min_count)
        assert len(edits) >= 500
        edits_txt = rc.cli_texts(codes, offs, fix, written, edits)[1]
    trim_txt, pairs_txt, single_txt, tally = rt.cli_texts(written, offs, trim, ranges)
    assert (trim["verdict"] == rt.TRIMMED).sum() > n // 50 and (trim["verdict"] == rt.DROPPED).sum() > 5
    if ranges:                                          # orphans: a surviving read whose mate was dropped
        ln = trim["len"]
        orphans = int(((ln[0::2] > 0) != (ln[1::2] > 0)).sum())
        assert orphans > 3 and single_txt.count(">") == orphans and pairs_txt.count(">") == int(2 * ((ln[0::2] > 0) & (ln[1::2] > 0)).sum())
    else:
        assert pairs_txt == "" and single_txt.count(">") == int((trim["len"] > 0).sum())
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    opts = ["-s", cfg, "-K", str(info["K"]), "-p", "4", "--max-k", str(gu.VARIANT_MAXK[info["variant"]]), "-c", str(min_count),
            "--min-cov", str(min_cov), "--min-len", str(min_len)] + (["--correct"] if correct else [])
    r = subprocess.run([exe, "trim"] + opts + ["-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in (("readTrim", trim_txt), ("trim.pairs.fa", pairs_txt), ("trim.single.fa", single_txt)) + ((("edits", edits_txt),) if correct else ()):
        got = (tmp_path / f"out.{ext}").read_bytes()
        assert got.decode() == text, f"{name}: out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    assert os.path.exists(tmp_path / "out.edits") == correct
    assert [x + "\n" for x in r.stdout.splitlines() if "bases out" in x] == [tally]
