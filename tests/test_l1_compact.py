"""GPU (-m gpu): the level-1 scatters, the level-2 scatter and the count stage on 16-byte compact LEVEL-1 records (1-word keys without
first-occurrence ordinals: csrc/sdt_sk_record1.h, a run cap of 54 - K) and, with SDT_FLAG_TRACK_FIRST, on the 24-byte records that path
keeps.  Every node is compared against the oracle (key, 8 saturating link counters, flags, count), the histogram and `linear` too.
Bit-exact: integer work only.

The oracle's answer for an input is computed once and shared by the two flag combinations."""
import functools
import multiprocessing as mp
import os
import sys
import uuid

import numpy as np
import pytest

import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def compact1_cap(K):
    """k-mers per compact level-1 record at most: n + K - 1 bases + 2 context bases <= 55 (a 10-bit level-2 bucket), n <= 32"""
    return min(32, 54 - K)


def oracle_answer(K, codes, offs):
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    hist, linear = o.mark()
    keys, l, r, cnt, fl = o.export()
    assert not keys[:, :-1].any()                # a 1-word key is the last of the oracle's four words
    key = keys[:, -1].copy()
    fl = fl.astype(np.int64)
    # oracle flags: bit0 linear, bit1 deleted, bit2 single -> kmer_t bitfield order linear, deleted, checked, single
    flags = (fl & 1) | (((fl >> 1) & 1) << 1) | (((fl >> 2) & 1) << 3)
    order = np.argsort(key, kind="stable")
    nodes = (key[order],) + tuple(np.asarray(a).astype(np.int64)[order] for a in (l, r, flags, cnt))
    for a in nodes:
        a.setflags(write=False)
    hist = np.array(hist)
    hist.setflags(write=False)
    return {"kmers": o.kmers_in_reads(), "nodes": o.node_count(), "hist": hist, "linear": linear, "table": nodes}


def check_against(pkg, synth, K, codes, offs, want, flags, pushes=1):
    with pkg.PregraphGPU(K, est_distinct=1 << 18, flags=flags) as g:
        n = len(offs) - 1
        for p in range(pushes):
            a, b = n * p // pushes, n * (p + 1) // pushes
            g.push_reads(synth.pack_2bit(codes[int(offs[a]):int(offs[b])]), offs[a:b + 1] - offs[a])
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (want["kmers"], want["nodes"])
        hist, linear = g.mark_and_hist()
        assert linear == want["linear"]
        assert (hist == want["hist"]).all()
        keys, l, rf, cnt = g.export_nodes()
        _, counters = g.stage_times()
    assert keys.shape[1] == 1
    order = np.argsort(keys[:, 0], kind="stable")
    rf = rf.astype(np.int64)
    got = (keys[:, 0][order], l.astype(np.int64)[order], (rf & 0xFFFFFF)[order], (rf >> 24)[order], cnt.astype(np.int64)[order])
    for name, a, b in zip(("key", "left links", "right links", "flags", "count"), got, want["table"]):
        assert a.shape == b.shape and (a == b).all(), name
    return counters


def flag_sets(pkg):
    return {"compact": pkg.SDT_FLAG_PARTITION, "ordinals": pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST}


# ---- runs at the cap ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cap_case(K, strips):
    from soapdenovo_trans_amd import synth
    tx = synth.make_transcriptome(12, seed=K)
    # (strips: a batch with reads of more than 256 k-mers leaves the one-lane-per-read scatter for the strip kernel, which cuts full
    # records at multiples of the cap in the read -- with compact level-1 records the same cap of 54 - K, no power of two)
    codes, offs = synth.sample_reads(*tx, n_reads=1500, read_len=330 if strips else 100, seed=K + 1, err=0.003)
    cap = compact1_cap(K)
    rng = np.random.default_rng(K + 2)
    unit = np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8)
    reads = []
    for i in range(1500):
        n = (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1)[i % 5]
        L = K - 1 + n
        if (i // 5) % 2 == 0:
            # homopolymer: ONE run of n k-mers, cut at the cap.  All four bases in turn: codes 2 and 3 put set bits right next to the
            # level-2 bucket field of a record of exactly 55 bases
            reads.append(np.full(L, (i // 10) % 4, dtype=np.uint8))
        else:
            reads.append(np.roll(np.tile(unit, L // 6 + 2), int(rng.integers(0, 6)))[:L])      # 6-base tandem repeat
    lens = np.array([len(r) for r in reads], dtype=np.uint64)
    codes = np.concatenate([codes] + reads)
    offs = np.concatenate([offs, offs[-1] + np.cumsum(lens)]).astype(np.uint64)
    codes.setflags(write=False)
    offs.setflags(write=False)
    return codes, offs, oracle_answer(K, codes, offs)


@pytest.mark.parametrize("variant", ["compact", "ordinals"])
@pytest.mark.parametrize("K,strips", [(27, False), (29, False), (31, False), (27, True), (31, True)])
def test_runs_at_the_cap(pkg, synth, K, strips, variant):
    """records of exactly 55 bases (a full run with both context bases), one base short of that, and runs split at the cap: reads of
    K - 1 + n bases for n around the cap and around twice the cap, homopolymers of every base (one run per read) and tandem repeats;
    strips: the same beside reads of 330 bases in one push, which send the batch through the strip kernel"""
    codes, offs, want = cap_case(K, strips)
    # (the strips case in ONE push: the longest read of a push decides its kernel, and the short reads must meet the strips too)
    counters = check_against(pkg, synth, K, codes, offs, want, flag_sets(pkg)[variant], pushes=1 if strips else 2)
    assert counters["pool_direct"] == 0 and counters["chunks_l1"] > 0 and counters["chunks_l2"] > 0, counters


# ---- several rounds per item, partial groups ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_case():
    from soapdenovo_trans_amd import synth
    tx = synth.make_transcriptome(2, seed=5, lo=400, hi=400)
    codes, offs = synth.sample_reads(*tx, n_reads=60000, read_len=100, seed=6, err=0.004)
    codes.setflags(write=False)
    offs.setflags(write=False)
    return codes, offs, oracle_answer(31, codes, offs)


@pytest.mark.parametrize("variant", ["compact", "ordinals"])
def test_items_of_several_rounds_and_partial_groups(pkg, synth, variant):
    """two transcripts of 400 bases under 60 000 reads: a few dozen level-1 buckets hold some 4 000 records each -- level-2 work items
    of several rounds of 2 048 records read out of 512-byte chunks, and sub-buckets left with 1, 2 or 3 waiting records"""
    codes, offs, want = deep_case()
    counters = check_against(pkg, synth, 31, codes, offs, want, flag_sets(pkg)[variant])
    assert counters["pool_direct"] == 0 and counters["chunks_l2"] > 0, counters


# ---- empty and one-record items -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_case():
    from soapdenovo_trans_amd import synth
    tx = synth.make_transcriptome(3, seed=9)
    codes, offs = synth.sample_reads(*tx, n_reads=40, read_len=100, seed=10, err=0.003)
    return codes, offs, oracle_answer(31, codes, offs)


@pytest.mark.parametrize("variant", ["compact", "ordinals"])
def test_forty_reads(pkg, synth, variant):
    """most level-1 buckets are empty, the others hold a record or two: chunks with one or two slots in use"""
    codes, offs, want = tiny_case()
    check_against(pkg, synth, 31, codes, offs, want, flag_sets(pkg)[variant])


# ---- pool exhaustion --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow_case():
    from soapdenovo_trans_amd import synth
    tx = synth.make_transcriptome(20, seed=34)
    codes, offs = synth.sample_reads(*tx, n_reads=5000, read_len=150, seed=35, err=0.003, ragged=True)
    codes.setflags(write=False)
    offs.setflags(write=False)
    return codes, offs, oracle_answer(31, codes, offs)


@pytest.mark.parametrize("variant", ["compact", "ordinals"])
def test_pool_exhaustion_takes_the_direct_path(pkg, synth, monkeypatch, variant):
    """a level-1 pool of 48 chunks (test hook) overflows at once: the records that find no slot go through the direct path, the others
    through 16-byte slots, and every node is still the oracle's"""
    monkeypatch.setenv("SDT_SK_POOL_CHUNKS1", "48")
    codes, offs, want = overflow_case()
    counters = check_against(pkg, synth, 31, codes, offs, want, flag_sets(pkg)[variant])
    assert 0 < counters["pool_direct"] <= want["kmers"], counters


# ---- two ranks on one device ----------------------------------------------------------------------------------------------------
SHARD_K, SHARD_READS, SHARD_LEN = 21, 6000, 120


def shard_reads():
    from soapdenovo_trans_amd import synth
    tx = synth.make_transcriptome(30, seed=SHARD_K)
    return synth.sample_reads(*tx, n_reads=SHARD_READS, read_len=SHARD_LEN, seed=SHARD_K + 1, err=0.003, ragged=True)


def _shard_worker(name, rank, n, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from soapdenovo_trans_amd import synth
    codes, offs = shard_reads()
    lo, hi = rank * SHARD_READS // n, (rank + 1) * SHARD_READS // n
    res = {}
    # the same reads with compact level-1 records and, with ordinals, with the 24-byte ones
    for variant, flags in (("compact", 0), ("ordinals", pkg.SDT_FLAG_TRACK_FIRST)):
        with pkg.PregraphGPU(SHARD_K, est_distinct=1 << 16, flags=flags) as g:
            g.comm_init_shm(name + variant[0], rank, n)
            g.set_read_ordinal(lo, 1)
            g.push_reads_sharded(synth.pack_2bit(codes[int(offs[lo]):int(offs[hi])]), offs[lo:hi + 1] - offs[lo])
            kmers, nodes = g.finish_count()
            hist, linear = g.mark_and_hist()
            res[variant + "_tot"] = g.allreduce(np.concatenate([hist, [kmers, nodes, linear]]))
            sent, recv, ms, nx = g.comm_stats()
            res[variant + "_comm"] = np.array([sent, recv, nx])
    np.savez(out, **res)


def test_two_ranks_exchange_compact_chunks(tmp_path):
    """two ranks share the device over the shared-memory transport: the all-reduced histogram and counts are the oracle's, and the
    level-1 chunks that travel are 512 bytes (+ their 4-byte meta word) where the 24-byte records' are 768.  K = 21: both records cap
    the runs at 32 k-mers, so the two runs cut the same records into the same chunks and the chunk count of the 24-byte run --
    bytes / (768 + 4) -- is the compact run's."""
    n = 2
    ctx = mp.get_context("spawn")
    name = "c" + uuid.uuid4().hex[:11]
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(n)]
    ps = [ctx.Process(target=_shard_worker, args=(name, r, n, outs[r])) for r in range(n)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(600)
        assert p.exitcode == 0
    codes, offs = shard_reads()
    o = ob.Oracle(SHARD_K, nsets=4)
    o.add_reads(codes, offs)
    ohist, olinear = o.mark()
    for r in range(n):
        z = np.load(outs[r])
        for variant in ("compact", "ordinals"):
            tot = z[variant + "_tot"]
            assert int(tot[257]) == o.kmers_in_reads() and int(tot[258]) == o.node_count() and int(tot[259]) == olinear, variant
            assert (tot[:257] == ohist).all(), variant
        sent_c, sent_o = int(z["compact_comm"][0]), int(z["ordinals_comm"][0])
        print(f"rank {r}: bytes sent: compact {sent_c}, 24-byte records {sent_o}")
        assert sent_o > 0 and sent_o % (768 + 4) == 0
        chunks = sent_o // (768 + 4)
        assert sent_c == chunks * 512 + chunks * 4, (sent_c, sent_o, chunks)
        assert (sent_c - 4 * chunks) * 3 == (sent_o - 4 * chunks) * 2
