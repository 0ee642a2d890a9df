"""GPU (-m gpu): the read walk of the level-1 scatter with one lane per read (csrc/sdt_sk_scatter_seq.cuh over csrc/sdt_sk_walk.h): every
lane takes its bases from a register window that is refilled every sixteen steps -- by all lanes at once, whether or not a lane's
read still has bases -- and cuts its records out of the tile in one pass over the words they span.

Two read sets per K, of 257 and of 513 reads (a last tile of one read), each made of
  * reads of K, K + 1 and K + 2 bases (none, one and two k-mers: len >= K + 1) that start at every phase 0..15 of a stream word,
    behind filler reads of 40..55 bases;
  * reads of 150 bases;
  * reads of 40 bases next to reads of K + 255 bases (256 k-mers, the most a lane walks; 286 bases at K = 31) in the same wavefront:
    the lanes that are done step on while their neighbours walk;
  * reads of K + 255 random bases: more than 24 runs, the emission on the spot;
  * a last read that ends with the last base of a stream word (the set of 257) or one base into it (the set of 513).
Every case counts one set, resets, counts the other and compares every node, the histogram and `linear` with the oracle of the second
set alone, before and after delow(2): the launches behind a reset carry the table's clear and a replay launch behind them.  K = 23, 31
and 63 (2-word keys), with and without first-occurrence ordinals (24-byte and 16-byte level-1 records).  Integer work: bit-exact."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import fullsize_paths_util as fu

pytestmark = pytest.mark.gpu

PART, FIRST = 2, 4                                           # SDT_FLAG_PARTITION, SDT_FLAG_TRACK_FIRST
KS = (23, 31, 63)


def read_set(K, n_reads, seed, end_phase):
    """-> (codes uint8, offs uint64, the phases at which the reads of K + 1 and K + 2 bases start)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=3000, dtype=np.uint8)
    long_len = K + 255
    reads, total, phases = [], 0, {K + 1: set(), K + 2: set()}

    def add(r):
        nonlocal total
        reads.append(np.asarray(r, dtype=np.uint8))
        total += len(r)

    def from_genome(n):
        s = int(rng.integers(0, len(genome) - n))
        r = genome[s: s + n]
        return r if rng.integers(0, 2) else (3 - r[::-1]).astype(np.uint8)           # either strand (A C T G = 0 1 2 3: complement = 3 - b)

    for ph in range(16):
        for n in (K, K + 1, K + 2):
            add(from_genome(40 + (ph - total - 40) % 16))    # the filler that puts the next read at phase ph
            assert total % 16 == ph
            if n in phases:
                phases[n].add(total % 16)
            add(from_genome(n))
    n_mid = n_reads - len(reads) - 1
    n150, n_alt = n_mid - n_mid // 2, (n_mid // 4) & ~1
    n_rand = n_mid - n150 - n_alt
    for _ in range(n150):
        add(from_genome(150))
    for i in range(n_alt):
        add(from_genome(40) if i % 2 == 0 else from_genome(long_len))
    for _ in range(n_rand):
        add(rng.integers(0, 4, size=long_len, dtype=np.uint8))
    add(from_genome(K + 8 + (end_phase - total - K - 8) % 16))
    assert len(reads) == n_reads and total % 16 == end_phase
    offs = np.zeros(n_reads + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), offs, phases


@functools.lru_cache(maxsize=None)
def sets(K):
    """the two read sets of K with the oracle's answer for each alone (shared by the cases, read-only)"""
    out = []
    for n_reads, seed, end_phase in ((257, 1000 + K, 0), (513, 2000 + K, 1)):
        codes, offs, phases = read_set(K, n_reads, seed, end_phase)
        ans = fu.oracle_answer(ob, K, [(codes, offs)], with_first=True)
        ans["K"] = K
        for a in (codes, offs, *ans.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out.append((codes, offs, phases, ans))
    return out


@pytest.mark.parametrize("K", KS)
def test_the_read_sets_hold_what_the_cases_are_about(K):
    for (codes, offs, phases, ans), n_reads in zip(sets(K), (257, 513)):
        lens = np.diff(offs.astype(np.int64))
        assert len(lens) == n_reads and n_reads % 256 in (1,)
        assert phases[K + 1] == set(range(16)) and phases[K + 2] == set(range(16))
        assert (lens == K).sum() >= 16 and (lens == 150).sum() > 0 and (lens == K + 255).sum() > 8 and lens.max() == K + 255
        wave = lens[: (len(lens) // 64) * 64].reshape(-1, 64)
        assert (((wave == 40).sum(axis=1) > 0) & ((wave == K + 255).sum(axis=1) > 0)).any(), "a 40-base read and a longest read in one wavefront"
        assert int(ans["kmers"]) == int(np.maximum(lens - K + 1, 0)[lens >= K + 1].sum())
    assert int(sets(K)[0][1][-1]) % 16 == 0 and int(sets(K)[1][1][-1]) % 16 == 1


@pytest.mark.parametrize("order", ["257_then_513", "513_then_257"])
@pytest.mark.parametrize("track", [False, True], ids=["compact", "first"])
@pytest.mark.parametrize("K", KS)
def test_walk_equals_oracle_behind_a_reset(pkg, synth, K, track, order):
    first, second = sets(K) if order == "257_then_513" else sets(K)[::-1]
    flags = PART | (FIRST if track else 0)
    what = f"K={K} track={track} {order}"
    with pkg.PregraphGPU(K, est_distinct=1 << 18, flags=flags) as g:
        g.push_reads(synth.pack_2bit(first[0]), first[1])
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (int(first[3]["kmers"]), int(first[3]["nodes"])), (what, "the first job", kmers, nodes)
        g.reset()
        g.kernel_time(reset=True)
        g.push_reads(synth.pack_2bit(second[0]), second[1])
        fu.compare_with_answer(g, second[3], track, what)
        ms, counters = g.stage_times()
        print(what, ms, counters)
        # the pipeline took the job, through the level-1 scatter, and no k-mer went round it
        assert ms[1] > 0 and ms[0] == 0 and counters["pool_direct"] == 0 and counters["batches"] > 0, (what, ms, counters)
