"""GPU (-m gpu): the level-2 chunk lists of the locality pipeline -- the scan of the 2^18 bucket counts over the whole chip
(k_sk_scan_wide) and k_sk_chunk_place, which files the chunk ids by stretches: per-bucket counts in LDS, one run per bucket and stretch.

Which path a chunk takes depends on how many level-1 buckets a stretch of 32 768 chunk ids names:
  - a handful (the hot reads: poly-A and one tandem repeat): every chunk goes through the LDS counters of a slot
  - all 256 (reads off a transcriptome): eight level-1 buckets get a slot, the chunks of the others take the per-chunk path, in the same
    stretch; more than 32 768 chunk ids, so several stretches and several workgroups reserve runs in the same buckets
  - SDT_SK_ITEM_CHUNKS=16: many short level-2 work items, so many blocks of chunk ids with dead ids between them
A chunk missing from its list, or listed twice, changes the counts: every node, the histogram and `linear` are compared with the oracle
(tests/fullsize_paths_util.py), and finish_count raises if the library's conservation check (k-mers cut into records == k-mers counted)
fails.  Integer work only: bit-exact."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import fullsize_paths_util as fu

pytestmark = pytest.mark.gpu

PART = 2                                                      # SDT_FLAG_PARTITION
STRETCH = 32 * 1024                                           # chunk ids per stretch (SK_PLACE_STRETCH, csrc/sdt_superkmer_kernels.cuh)
SLOTS = 8                                                     # level-1 buckets with LDS counters per stretch (SK_PLACE_SLOTS)
K = 31


def frozen(ans, codes, offs):
    for a in list(ans.values()) + [codes, offs]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return codes, offs, ans


@functools.lru_cache(maxsize=None)
def hot_case():
    codes, offs = fu.hot_reads(20000, 100)
    return frozen(fu.oracle_answer(ob, K, [(codes, offs)], with_first=False), codes, offs)


@functools.lru_cache(maxsize=None)
def wide_case():
    from soapdenovo_trans_amd import synth
    # 12 000 reads of random bases: 1.4 M k-mers in some 140 000 records whose minimizers fall all over the 2^18 final buckets, so most
    # chunks hold a record or two; behind them 8 000 reads off 50 transcripts, whose buckets take many records
    rng = np.random.default_rng(41)
    rc, ro = rng.integers(0, 4, size=12000 * 150, dtype=np.uint8), np.arange(12001, dtype=np.uint64) * 150
    tx = synth.make_transcriptome(50, seed=42)
    tc, to = synth.sample_reads(*tx, n_reads=8000, read_len=150, seed=43, err=0.01, ragged=True)
    codes, offs = np.concatenate([rc, tc]), np.concatenate([ro, to[1:] + ro[-1]])
    return frozen(fu.oracle_answer(ob, K, [(codes, offs)], nsets=8, with_first=False), codes, offs)


@functools.lru_cache(maxsize=None)
def mixed_case():
    from soapdenovo_trans_amd import synth
    codes, offs = fu.mixed_reads(synth, K, 12000, 150)
    return frozen(fu.oracle_answer(ob, K, [(codes, offs)], with_first=False), codes, offs)


def count_and_compare(pkg, synth, codes, offs, ans, what, est_distinct=1 << 18):
    with pkg.PregraphGPU(K, est_distinct=est_distinct, flags=PART) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        fu.compare_with_answer(g, ans, False, what)          # (finish_count first: SDT_ESTATE of the conservation check raises there)
        return g.stage_times()[1]


def test_chunks_of_a_handful_of_level1_buckets(pkg, synth):
    """poly-A and the tandem repeat ACTGGC: at most seven level-1 buckets, so every chunk of the one stretch finds a slot, and a few final
    buckets hold thousands of chunks each -- long runs, reserved once"""
    codes, offs, ans = hot_case()
    assert fu.level1_buckets_touched(pkg, dict(ans, K=K)) < SLOTS
    counters = count_and_compare(pkg, synth, codes, offs, ans, "hot")
    print(counters)
    assert counters["pool_direct"] == 0 and 1000 < counters["chunks_l2"] < STRETCH, counters


def test_chunks_of_every_level1_bucket_in_several_stretches(pkg, synth):
    """random reads and reads off 50 transcripts: far more level-1 buckets than slots in every stretch (slots and the per-chunk path side
    by side), and more chunks than two stretches hold"""
    codes, offs, ans = wide_case()
    assert len({pkg.kmer_bucket(row, K) for row in ans["keys0"][::500]}) > 8 * SLOTS        # (a sample of the keys is enough)
    counters = count_and_compare(pkg, synth, codes, offs, ans, "wide", est_distinct=1 << 21)
    print(counters)
    assert counters["pool_direct"] == 0 and counters["chunks_l2"] > 2 * STRETCH, counters


def test_chunks_of_many_short_items(pkg, synth, tmp_path):
    """SDT_SK_ITEM_CHUNKS=16 (read when the library is loaded: a child process): a level-1 bucket is split by many level-2 work items,
    each with blocks of chunk ids of its own"""
    codes, offs, ans = mixed_case()
    res = fu.run_child(tmp_path, "chunk_lists_items16", {"SDT_SK_ITEM_CHUNKS": 16},
                       dict(K=K, flags=[PART], est_distinct=1 << 18, steps=[["push", 0, len(offs) - 1], ["finish"]]),
                       dict(ans, codes=codes, offs=offs), timeout=300)
    print(res)
    for run in res["runs"]:
        assert run["chunks_l1"] > 16 * 256 and run["chunks_l2"] > 0, run
