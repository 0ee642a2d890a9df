"""GPU (-m gpu): the level-2 scatter and the count stage on 16-byte compact records (1-word keys without first-occurrence ordinals:
csrc/sdt_sk_record2.h) and, with SDT_FLAG_TRACK_FIRST, on the 24-byte records that path keeps.  Every node is compared against the
oracle (key, 8 saturating link counters, flags, count), as test_gpu_parity.test_node_table_equals_oracle does.  Bit-exact: integer work only.

The oracle's answer for an input is computed once and shared by the two flag combinations."""
import functools

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu


def compact_cap(K):
    """k-mers per compact record at most: n + K - 1 bases + 2 context bases <= 60, n <= 32"""
    return min(32, 59 - K)


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
    # records at multiples of a power of two in the read: the largest one below the compact record's cap)
    codes, offs = synth.sample_reads(*tx, n_reads=1500, read_len=330 if strips else 100, seed=K + 1, err=0.003)
    cap = compact_cap(K)
    if strips:
        cap = 1 << (cap.bit_length() - 1)
    rng = np.random.default_rng(K + 2)
    unit = np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8)
    reads = []
    for i in range(1500):
        n = (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1)[i % 5]
        L = K - 1 + n
        if (i // 5) % 2 == 0:
            reads.append(np.full(L, rng.integers(0, 4), dtype=np.uint8))               # homopolymer: ONE run of n k-mers, cut at the cap
        else:
            reads.append(np.roll(np.tile(unit, L // 6 + 2), int(rng.integers(0, 6)))[:L])      # 6-base tandem repeat
    lens = np.array([len(r) for r in reads], dtype=np.uint64)
    codes = np.concatenate([codes] + reads)
    offs = np.concatenate([offs, offs[-1] + np.cumsum(lens)]).astype(np.uint64)
    codes.setflags(write=False)
    offs.setflags(write=False)
    return codes, offs, oracle_answer(K, codes, offs)


# (The strip kernel of level 1 cannot be reached through an even K -- the library takes odd K only, callers clamp an even one down
# first --, so its case is K = 31 with reads of 330 bases: more than 256 k-mers per read send the batch through the strips.)
@pytest.mark.parametrize("variant", ["compact", "ordinals"])
@pytest.mark.parametrize("K,strips", [(27, False), (29, False), (31, False), (31, True)])
def test_runs_at_the_cap(pkg, synth, K, strips, variant):
    """records of exactly 60 bases (a full run with both context bases), one base short of that, and runs split at the cap: reads of
    K - 1 + n bases for n around the cap and around twice the cap, homopolymers (one run per read) and tandem repeats"""
    codes, offs, want = cap_case(K, strips)
    # (the strips case in ONE push: the longest read of a push decides its kernel, and the short reads must meet the strips too)
    counters = check_against(pkg, synth, K, codes, offs, want, flag_sets(pkg)[variant], pushes=1 if strips else 2)
    assert counters["pool_direct"] == 0 and counters["chunks_l2"] > 0, counters


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
    """two transcripts of 400 bases under 60 000 reads: a few dozen level-1 buckets hold some 4 000 records each -- work items of
    several rounds of 2 048 records, sub-buckets that take many groups in one round, and sub-buckets left with 1, 2 or 3 waiting
    records when their item ends"""
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
    """most level-1 buckets are empty, the others hold a record or two: items of one partial group"""
    codes, offs, want = tiny_case()
    check_against(pkg, synth, 31, codes, offs, want, flag_sets(pkg)[variant])
