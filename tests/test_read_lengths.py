"""GPU (-m gpu): read length decides more code paths of the library than any other property of the input -- the kernel family of
pass 1, the launch geometry of the read-only entry points, and where each entry point stops taking a read at all.  Every decision
is pinned here against the oracle (oracle/sdt_oracle.c, which takes reads of any length: tests/test_read_lengths_host.py) and the
Python restatements of the read-only rules.  All comparisons are exact.

The thresholds between two kernels of pass 1 are internal: the tests read from sdt_gpu_stage_times which family ran and assert what
must hold whatever the thresholds are (the route is monotone in the length, both routes occur, reads of 256 and 257 k-mers stay in
the locality pipeline).  The limits past which an entry point REFUSES are part of the ABI (include/sdt_gpu.h) and are derived here:

  pass 1      the direct kernel's tile of 64 reads: 584 + 16 L bytes of LDS, 64 KiB at most -> 4 059 bases (SDT_PASS1_MAX_READ_LEN)
  profile, correct, select   4 bytes per k-mer and wavefront, 64 KiB at most -> 16 384 k-mers; 4 / 2 / 1 wavefronts per workgroup
              while 4 x / 2 x the strip fit 64 KiB: the geometry changes past 4 096 and 8 192 k-mers
  align_reads 8 bytes x (k-mers + 2 x 20 hits) per wavefront; 4 / 2 / 1 wavefronts while 4 x / 2 x fit 48 KiB: past 1 496 and
              3 032 k-mers; refused past 64 KiB: 8 152 k-mers

The sharded path (two ranks and more) takes only what the locality pipeline takes and refuses the rest; a context with a
communicator of ONE rank counts through the single-GPU path and falls back like it."""
import multiprocessing as mp
import os
import uuid

import numpy as np
import pytest

import map_util as mu
import oracle_binding as ob
import read_correct_util as rcu
import read_select_util as rsu
import test_kmer_search as ks
from test_gpu_parity import keys_to_int, node_dict_gpu, node_dict_oracle

pytestmark = pytest.mark.gpu

PASS1_MAX = 4059                  # 584 + 16 * 4059 = 65 528 <= 65 536 < 584 + 16 * 4060
assert 584 + 16 * PASS1_MAX <= 64 * 1024 < 584 + 16 * (PASS1_MAX + 1)
STRIP_MAX_KMERS = 64 * 1024 // 4  # profile / correct / select
ALIGN_MAX_KMERS = 64 * 1024 // 8 - 2 * 20
ALIGN_WAVE_STEPS = (48 * 1024 // 4 // 8 - 2 * 20, 48 * 1024 // 2 // 8 - 2 * 20)
assert (STRIP_MAX_KMERS, ALIGN_MAX_KMERS, ALIGN_WAVE_STEPS) == (16384, 8152, (1496, 3032))


# ---- references: computed once per input, shared, never changed -------------------------------------------------------------------
def reference(K, codes, offs, ordinal_of=None):
    """the oracle over one read stream: counts, every node's first occurrence, and for d in (0, 2) what delow(d) removes, the
    histogram, the linear count and every node.  ordinal_of: read index -> read ordinal (increasing), default the index"""
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    ref = {"counts": (o.kmers_in_reads(), o.node_count())}
    keys = o.export()[0]
    first = o.export_first()
    rd = (first >> np.uint64(16)).astype(np.int64)
    if ordinal_of is not None:
        rd = np.asarray(ordinal_of, dtype=np.int64)[rd]
    ref["first"] = dict(zip(keys_to_int(keys), ((rd << 16) | (first & np.uint64(0xFFFF)).astype(np.int64)).tolist()))
    ref["scans"] = []
    for d in (0, 2):
        removed = o.delow(d) if d else None
        hist, linear = o.mark()
        ref["scans"].append((d, removed, hist, linear, node_dict_oracle(o)))
    return ref


def assert_table_is(g, ref, tracked=True):
    assert g.finish_count() == ref["counts"]
    if tracked:
        keys, _, _, _, first = g.export_nodes(with_first=True)
        assert dict(zip(keys_to_int(keys), (int(x) for x in first))) == ref["first"]
    for d, removed, hist, linear, nodes in ref["scans"]:
        if d:
            assert g.delow(d) == removed
        ghist, glinear = g.mark_and_hist()
        assert glinear == linear
        assert (ghist == hist).all()
        assert node_dict_gpu(g) == nodes


def route_of(g):
    """which pass-1 family ran in this context so far: 'pipeline', 'direct' or 'both'"""
    ms, cnt = g.stage_times()
    pipeline = cnt["records"] > 0 and ms[1] > 0
    direct = ms[0] > 0
    assert pipeline or direct, (ms, cnt)
    if not pipeline:
        assert cnt["records"] == 0 and ms[1] == 0
    return "both" if pipeline and direct else ("pipeline" if pipeline else "direct")


def reads_from(src, lens, rng, err=0.003):
    """reads of the given lengths off random places of src, either strand, substitutions at rate err"""
    out = []
    for l in (int(x) for x in lens):
        p = int(rng.integers(0, len(src) - l + 1))
        r = src[p:p + l]
        if rng.random() < 0.5:
            r = r[::-1] ^ 2
        r = r.astype(np.uint8).copy()
        e = rng.random(l) < err
        r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()), dtype=np.uint8)) & 3
        out.append(r)
    return concat(out)


def concat(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return (np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8)).astype(np.uint8), offs


def revcomp(c):
    return (c[::-1] ^ 2).astype(np.uint8)


# ---- 1. pass 1 across the routes ------------------------------------------------------------------------------------------------
KS = (31, 63, 95)
FLAG_NAMES = ("direct", "partition")


def lengths(K):
    return (K + 1, K + 255, K + 256, 600, 1100, 1200, 2000, PASS1_MAX)


_inputs, _routes = {}, {}


def pass1_input(K, L, ragged):
    key = (K, L, ragged)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * K + L + (7 if ragged else 0))
        src = rng.integers(0, 4, size=3 * L, dtype=np.uint8)
        lens = np.full(200, L, dtype=np.int64)
        if ragged:
            lens = rng.integers(max(8, L // 4), L + 1, size=200)
            lens[[3, 50, 51, 120]] = [0, K, K + 1, L // 2]
            lens[[0, 77, 199]] = L                       # the longest read is L: it decides the route
        codes, offs = reads_from(src, lens, rng)
        _inputs[key] = (codes, offs, reference(K, codes, offs))
    return _inputs[key]


def pass1_case(pkg, synth, K, L, ragged, fl):
    """runs (K, L, ragged, flags) once, compares with the oracle, -> the route it took"""
    key = (K, L, ragged, fl)
    if key not in _routes:
        codes, offs, ref = pass1_input(K, L, ragged)
        flags = pkg.SDT_FLAG_DIRECT if fl == "direct" else pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST
        with pkg.PregraphGPU(K, est_distinct=1 << 12, flags=flags) as g:        # small table: it grows by rebuild
            g.push_reads(synth.pack_2bit(codes), offs)
            assert_table_is(g, ref, tracked=fl == "partition")
            _routes[key] = route_of(g)
    return _routes[key]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("fl", FLAG_NAMES)
@pytest.mark.parametrize("K,L", [(K, L) for K in KS for L in lengths(K)])
def test_pass1_equals_oracle_at_every_length(pkg, synth, K, L, ragged, fl):
    """200 reads off 3 L random bases, both strands, 0.3 % substitutions (ragged: lengths L / 4 .. L with reads of 0, K, K + 1 and
    L / 2 bases among them): counts, histogram, linear count, every node with its eight link counters and flags, every node's
    first-occurrence ordinal, and all of it again after delow(2)"""
    route = pass1_case(pkg, synth, K, L, ragged, fl)
    assert route in ("pipeline", "direct")
    if fl == "direct":
        assert route == "direct"


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("K", KS)
def test_pass1_route_is_monotone_in_the_length(pkg, synth, K, ragged):
    """under SDT_FLAG_PARTITION the pipeline takes the short reads and the direct kernel the long ones, with one switch in between;
    both occur for every K; 256 and 257 k-mers per read (the last length of the one-lane scatter, the first of the strip kernel) are
    both the pipeline's with 1- and 2-word keys"""
    routes = [pass1_case(pkg, synth, K, L, ragged, "partition") for L in lengths(K)]
    print(f"K = {K}, ragged = {ragged}: " + ", ".join(f"{L}: {r}" for L, r in zip(lengths(K), routes)))
    assert set(routes) == {"pipeline", "direct"}, routes
    switch = routes.index("direct")
    assert all(r == "pipeline" for r in routes[:switch]) and all(r == "direct" for r in routes[switch:]), routes
    assert routes[0] == "pipeline" and routes[-1] == "direct"
    if K in (31, 63):
        assert routes[1] == routes[2] == "pipeline", routes


# ---- 2. routes mixed in one context ---------------------------------------------------------------------------------------------
_mixed = {}


def mixed_input(synth, K, Lmid):
    if K not in _mixed:
        tx = synth.make_transcriptome(6, seed=K, lo=2500)
        batches = [synth.sample_reads(*tx, n_reads=1500, read_len=150, seed=K + 1, err=0.003, ragged=True),
                   synth.sample_reads(*tx, n_reads=120, read_len=Lmid, seed=K + 2, err=0.003),
                   synth.sample_reads(*tx, n_reads=1500, read_len=150, seed=K + 3, err=0.003, ragged=True)]
        assert (np.diff(batches[1][1].astype(np.int64)) == Lmid).all()
        codes, offs = concat([c[int(o[i]):int(o[i + 1])] for c, o in batches for i in range(len(o) - 1)])
        n = [len(o) - 1 for _, o in batches]
        # the device form numbers the middle batch with stride 2
        ordinal_of = np.concatenate([np.arange(n[0]), n[0] + 2 * np.arange(n[1]), n[0] + 2 * n[1] + np.arange(n[2])])
        _mixed[K] = (batches, n, reference(K, codes, offs), reference(K, codes, offs, ordinal_of))
    return _mixed[K]


@pytest.mark.parametrize("form", ["push", "device"])
@pytest.mark.parametrize("K,Lmid", [(31, 2000), (63, 700)])
def test_routes_mixed_in_one_context(pkg, synth, K, Lmid, form):
    """150-base reads, then reads too long for the pipeline, then 150-base reads again, in one context whose table grows by rebuild
    in the middle and with finish_count only at the end: the direct kernel inserts while the pools still hold the records of the
    first batch.  Everything equals the oracle over the concatenated stream, first-occurrence ordinals included"""
    import torch
    batches, n, ref_plain, ref_strided = mixed_input(synth, K, Lmid)
    with pkg.PregraphGPU(K, est_distinct=1 << 12, flags=pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST) as g:
        hold = []
        for i, (codes, offs) in enumerate(batches):
            words = synth.pack_2bit(codes)
            if form == "push":
                g.push_reads(words, offs)
                continue
            d_w = torch.from_numpy(words.view(np.int32)).cuda()
            d_o = torch.from_numpy(offs.view(np.int64)).cuda()
            torch.cuda.synchronize()
            hold.append((d_w, d_o))                       # (the call is asynchronous)
            if i == 1:
                g.set_read_ordinal(n[0], 2)
            if i == 2:
                g.set_read_ordinal(n[0] + 2 * n[1], 1)
            g.count_reads_device(d_w, len(words), d_o, len(offs) - 1, int(np.diff(offs.astype(np.int64)).max()))
        assert_table_is(g, ref_plain if form == "push" else ref_strided)
        assert route_of(g) == "both"


@pytest.mark.parametrize("base,want_route", [((1 << 34) - 250, "pipeline"), ((1 << 34) - 150, "both")])
def test_ordinals_past_2_34_switch_to_the_direct_kernel(pkg, synth, base, want_route):
    """a super-k-mer record numbers 2^34 reads: two batches of 100 reads from ordinal 2^34 - 150 on, the second crosses 2^34 and is
    the direct kernel's (from 2^34 - 250 on, neither does: the control).  The ordinals are the oracle's, shifted by the base"""
    K = 31
    tx = synth.make_transcriptome(4, seed=5)
    codes, offs = synth.sample_reads(*tx, n_reads=200, read_len=100, seed=6, err=0.003)
    ref = reference(K, codes, offs, base + np.arange(200))
    cut = int(offs[100])
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.set_read_ordinal(base, 1)
        g.push_reads(synth.pack_2bit(codes[:cut]), offs[:101])
        g.push_reads(synth.pack_2bit(codes[cut:]), offs[100:] - offs[100])
        assert_table_is(g, ref)
        assert route_of(g) == want_route


# ---- 3. refusals leave no trace -------------------------------------------------------------------------------------------------
_refusal = {}


def refusal_input(synth, K=31):
    if not _refusal:
        tx = synth.make_transcriptome(5, seed=21, lo=PASS1_MAX + 200, hi=2 * PASS1_MAX)
        good = [synth.sample_reads(*tx, n_reads=300, read_len=150, seed=22 + i, err=0.003) for i in range(2)]
        short = synth.sample_reads(*tx, n_reads=20, read_len=150, seed=25)
        long_ = synth.sample_reads(*tx, n_reads=2, read_len=PASS1_MAX + 1, seed=26)
        assert (np.diff(long_[1].astype(np.int64)) == PASS1_MAX + 1).all()
        ragged_bad = concat([short[0][150 * i:150 * (i + 1)] for i in range(20)] + [long_[0][:PASS1_MAX + 1]])
        codes, offs = concat([c[150 * i:150 * (i + 1)] for c, _ in good for i in range(300)])
        _refusal.update(good=good, bad_ragged=ragged_bad, bad_fixed=long_, ref=reference(K, codes, offs))
    return _refusal


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("fl", FLAG_NAMES)
@pytest.mark.parametrize("form", ["push", "async", "fixed", "device"])
def test_a_batch_with_a_read_too_long_is_refused_whole(pkg, synth, form, fl, keep):
    """a good batch, a batch that holds one read of 4 060 bases, a good batch.  SDT_EINVAL comes from the call that handed the bad
    batch over and names the length and the limit; nothing of that batch is counted, kept or numbered: table and first-occurrence
    ordinals are the oracle's over the two good batches (the second numbered right behind the first), two batches are kept, and
    the second read pass goes over exactly their reads"""
    import torch
    K = 31
    c = refusal_input(synth)
    flags = (pkg.SDT_FLAG_DIRECT if fl == "direct" else pkg.SDT_FLAG_PARTITION) | pkg.SDT_FLAG_TRACK_FIRST | (pkg.SDT_FLAG_KEEP_READS if keep else 0)
    hold = []

    def hand_over(g, codes, offs):
        """-> the ticket to wait for, or None: the wait is no part of the hand-over and is only made for accepted batches"""
        words = np.ascontiguousarray(synth.pack_2bit(codes))
        offs = np.ascontiguousarray(offs)
        n, L = len(offs) - 1, int(np.diff(offs.astype(np.int64)).max())
        hold.append((words, offs))
        if form == "push":
            g.push_reads(words, offs)
        elif form == "async":
            return g.push_reads_async(words, offs)
        elif form == "fixed":
            assert (np.diff(offs.astype(np.int64)) == L).all()
            return g.push_reads_fixed_async(words, n, L)
        else:
            d_w = torch.from_numpy(words.view(np.int32)).cuda()
            d_o = torch.from_numpy(offs.view(np.int64)).cuda()
            torch.cuda.synchronize()
            hold.append((d_w, d_o))
            g.count_reads_device(d_w, len(words), d_o, n, L)

    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=flags) as g:
        def accepted(batch):
            t = hand_over(g, *batch)
            if t is not None:
                g.push_wait(t)
            return t

        t1 = accepted(c["good"][0])
        with pytest.raises(pkg.SdtError) as e:            # (the push itself: no push_wait in here)
            hand_over(g, *(c["bad_fixed"] if form == "fixed" else c["bad_ragged"]))
        assert e.value.code == pkg.SDT_EINVAL
        assert str(PASS1_MAX + 1) in str(e.value) and str(PASS1_MAX) in str(e.value), str(e.value)
        t2 = accepted(c["good"][1])
        assert (t1, t2) == ((1, 2) if form in ("async", "fixed") else (None, None))      # the refused batch took no ticket
        assert_table_is(g, c["ref"])
        if keep and form != "device":                     # (reads counted from device buffers are the caller's: nothing is kept)
            assert g.kept_batches() == 2
            for i in range(2):
                words, offs, ord_base, ord_stride = g.fetch_kept_batch(i)
                assert (ord_base, ord_stride, len(offs) - 1) == (300 * i, 1, 300)
            keys = g.export_nodes()[0]
            g.load_paths(keys, np.ones(len(keys), dtype=np.uint64))          # every node skipped: the pass runs, no arcs
            assert g.map_reads() == (600, 0)


@pytest.mark.parametrize("keep", [False, True])
def test_refusal_comes_at_once_while_an_earlier_launch_is_deferred(pkg, synth, keep):
    """push_reads_async puts off the launch of a batch that would make the locality pipeline flush until 32 copies are queued
    behind it (or a sync point comes).  Batch 2 here is such a batch: one 1 100-base read among 16 000 empty ones, which the
    library's estimate -- reads x k-mers of the longest read -- puts past the 2^24 k-mers the smallest pools hold.  A too-long batch
    handed over behind it used to be staged, kept and numbered without a word, and refused by whichever later call launched the
    queue; it must be refused by its own push, with batch 2 still waiting, and leave no trace: the table and the ordinals are the
    oracle's over batches 1, 2 and 4"""
    K = 31
    c = refusal_input(synth)
    rng = np.random.default_rng(60)
    one = rng.integers(0, 4, size=1100, dtype=np.uint8)
    lens = np.zeros(16_001, dtype=np.int64)
    lens[9000] = 1100
    assert (16_001 + 32) * (1100 - K + 1) > 1 << 24
    offs2 = np.zeros(16_002, dtype=np.uint64)
    offs2[1:] = np.cumsum(lens)
    batches = [c["good"][0], (one, offs2), c["good"][1]]
    codes, offs = concat([b[int(o[i]):int(o[i + 1])] for b, o in batches for i in range(len(o) - 1)])
    ref = reference(K, codes, offs)
    flags = pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST | (pkg.SDT_FLAG_KEEP_READS if keep else 0)
    hold = []
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=flags) as g:
        def push(batch):
            words, o = np.ascontiguousarray(synth.pack_2bit(batch[0])), np.ascontiguousarray(batch[1])
            hold.append((words, o))
            return g.push_reads_async(words, o)
        assert push(batches[0]) == 1                      # launched at once: the pools exist from here on
        assert push(batches[1]) == 2                      # queued, its launch put off
        with pytest.raises(pkg.SdtError) as e:
            push(c["bad_ragged"])
        assert e.value.code == pkg.SDT_EINVAL and str(PASS1_MAX + 1) in str(e.value) and str(PASS1_MAX) in str(e.value)
        assert push(batches[2]) == 3
        g.push_wait(3)
        assert_table_is(g, ref)
        assert route_of(g) == "pipeline"
        if keep:
            assert g.kept_batches() == 3
            assert [g.fetch_kept_batch(i)[2] for i in range(3)] == [0, 300, 300 + 16_001]


def test_one_rank_communicator_falls_back_like_the_single_gpu_path(pkg, synth):
    """a context whose communicator has ONE rank counts through the single-GPU path: reads the pipeline cannot take (700 bases at
    K = 63) are counted by the direct kernel, not refused"""
    K = 63
    tx = synth.make_transcriptome(4, seed=31, lo=1500)
    a = synth.sample_reads(*tx, n_reads=100, read_len=700, seed=32, err=0.003)
    b = synth.sample_reads(*tx, n_reads=300, read_len=150, seed=33, err=0.003)
    codes, offs = concat([c[int(o[i]):int(o[i + 1])] for c, o in (a, b) for i in range(len(o) - 1)])
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_PARTITION | pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.comm_init_shm(f"rl{os.getpid()}", 0, 1)
        g.push_reads_sharded(synth.pack_2bit(a[0]), a[1])
        g.push_reads_sharded(synth.pack_2bit(b[0]), b[1])
        assert_table_is(g, reference(K, codes, offs))
        assert route_of(g) == "both"


def _sharded_refusal_worker(name, rank, n, out):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from soapdenovo_trans_amd import synth
    K = 63
    tx = synth.make_transcriptome(4, seed=31, lo=1500)
    long_ = synth.sample_reads(*tx, n_reads=40, read_len=700, seed=32 + rank, err=0.003)
    codes, offs = synth.sample_reads(*tx, n_reads=600, read_len=150, seed=33, err=0.003)
    lo, hi = rank * 600 // n, (rank + 1) * 600 // n
    res = []
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.comm_init_shm(name, rank, n)
        g.set_read_ordinal(lo, 1)
        words = synth.pack_2bit(long_[0])
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(long_[1].view(np.int64)).cuda()
        torch.cuda.synchronize()
        for call in (lambda: g.push_reads_sharded(words, long_[1]), lambda: g.count_reads_sharded(d_w, len(words), d_o, 40, 700)):
            try:
                call()
                res.append((0, ""))
            except pkg.SdtError as e:
                res.append((int(e.code), str(e)))
        g.push_reads_sharded(synth.pack_2bit(codes[150 * lo:150 * hi]), offs[lo:hi + 1] - offs[lo])
        kmers, nodes = g.finish_count()
        tot = g.allreduce([kmers, nodes])
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        np.savez(out, keys=keys, l=l, rf=rf, cnt=cnt, first=first, tot=tot, codes=np.array([r[0] for r in res]),
                 msgs=np.array([r[1] for r in res]))


def test_sharded_path_refuses_what_the_pipeline_cannot_take(pkg, synth, tmp_path):
    """two ranks on one device (shared-memory transport): 700-base reads at K = 63 do not fit the LDS of the level-1 scatter, and a
    rank cannot count them in its own table (the k-mers may be another rank's): push_reads_sharded and count_reads_sharded return
    SDT_EINVAL with the length in the message on every rank, and the contexts count a following 150-base batch as if nothing had
    happened -- nodes, counts, links and first-occurrence ordinals of the union are the oracle's"""
    n, K = 2, 63
    ctx = mp.get_context("spawn")
    name = "r" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(n)]
    ps = [ctx.Process(target=_sharded_refusal_worker, args=(name, r, n, outs[r])) for r in range(n)]
    try:
        for p in ps:
            p.start()
        for p in ps:
            p.join(300)
        assert [p.exitcode for p in ps] == [0] * n
    finally:                                              # a rank that hangs is not left behind with the GPU open
        for p in ps:
            if p.is_alive():
                p.kill()
                p.join(30)
    tx = synth.make_transcriptome(4, seed=31, lo=1500)
    codes, offs = synth.sample_reads(*tx, n_reads=600, read_len=150, seed=33, err=0.003)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    okeys, ol, orr, ocnt, _ = o.export()
    want = {k: (int(a), int(b), int(c), int(f)) for k, a, b, c, f in zip(keys_to_int(okeys), ol, orr, ocnt, o.export_first())}
    got = {}
    for r in range(n):
        z = np.load(outs[r])
        assert z["codes"].tolist() == [pkg.SDT_EINVAL, pkg.SDT_EINVAL], z["msgs"].tolist()
        assert all("700 bases" in m and "sharded" in m for m in z["msgs"].tolist()), z["msgs"].tolist()
        assert z["tot"].tolist() == [o.kmers_in_reads(), o.node_count()]
        for k, a, b, c, f in zip(keys_to_int(z["keys"]), z["l"], z["rf"], z["cnt"], z["first"]):
            assert k not in got
            got[k] = (int(a), int(b) & 0xFFFFFF, int(c), int(f))
    assert got == want


# ---- 4. read-only entry points at long reads ------------------------------------------------------------------------------------
_long = {}
MK = (4096, 4097, 8192, 8193, STRIP_MAX_KMERS)


def long_case(K):
    """one transcript of 16 384 + K + 300 bases under 12x of 150-base reads -> the oracle's table; a batch of long reads (per length: the transcript's prefix, a reverse-strand stretch, a stretch with a substitution every
    700 bases, random bases) and reads of K - 1 and K bases; a batch of reads that pass 1 itself can keep"""
    if K in _long:
        return _long[K]
    rng = np.random.default_rng(40 + K)
    T = STRIP_MAX_KMERS + K + 300
    tx = rng.integers(0, 4, size=T, dtype=np.uint8)
    # the table's reads tile the transcript: a 150-base read every 12 bases, strands alternating, no errors -- every k-mer of the
    # transcript is a node with a count of (150 - K + 1) / 12 or more
    starts = list(range(0, T - 150, 12)) + [T - 150]
    tcodes, toffs = concat([revcomp(tx[p:p + 150]) if i % 2 else tx[p:p + 150].copy() for i, p in enumerate(starts)])

    def four(mk):
        L = mk + K - 1
        sub = tx[300:300 + L].copy()
        sub[350::700] = (sub[350::700] + 1) & 3
        return [tx[:L].copy(), revcomp(tx[150:150 + L]), sub, rng.integers(0, 4, size=L, dtype=np.uint8)]

    reads = [r for mk in MK for r in four(mk)] + [tx[1000:1000 + K - 1].copy(), tx[2000:2000 + K].copy()]
    bcodes, boffs = concat(reads)
    kcodes, koffs = concat(four(PASS1_MAX - K + 1) + [tx[500:500 + K - 1].copy(), tx[700:700 + K].copy()])
    o = ob.Oracle(K, nsets=4)
    o.add_reads(tcodes, toffs)
    nodes = ks.node_dict_oracle(o)
    c = dict(K=K, tx=tx, T=T, tcodes=tcodes, toffs=toffs, bcodes=bcodes, boffs=boffs, kcodes=kcodes, koffs=koffs, nodes=nodes,
             count=rcu.table_counts(nodes), counts=(o.kmers_in_reads(), o.node_count()))
    _long[K] = c
    return c


SELECT_SETTINGS = ((150, 11), (0, 12))                    # (max_cv_pct, seed); target 6


def long_expected(c, which):
    """the restatements over the batch (which = 'b') or over the kept stream (which = 'k': the table's reads, then the keepable long
    reads, numbered in that order) -- once"""
    key = "exp_" + which
    if key not in c:
        K = c["K"]
        codes, offs = (c["bcodes"], c["boffs"]) if which == "b" else concat(
            [a[int(o[i]):int(o[i + 1])] for a, o in ((c["tcodes"], c["toffs"]), (c["kcodes"], c["koffs"])) for i in range(len(o) - 1)])
        kc = rcu.read_kmer_counts(codes, offs, K, c["count"])
        c[key] = dict(codes=codes, offs=offs, profile=ks.expect_profile(codes, offs, K, c["nodes"], 2),
                      correct=rcu.expect_correct(codes, offs, K, c["count"], 2, kmer_counts=kc),
                      select=[rsu.expect_select(codes, offs, K, c["count"], 6, cv, seed, kmer_counts=kc) for cv, seed in SELECT_SETTINGS])
    return c[key]


def as_records(t, dtype):
    return t.cpu().numpy().view(np.uint32).copy().view(dtype).reshape(-1)


@pytest.mark.parametrize("K", [31, 95])
def test_read_only_entry_points_at_long_reads(pkg, synth, K, monkeypatch):
    """profile, correct (min_count 2) and select (target 6; max_cv_pct 150 and 0) over reads of 4 096, 4 097, 8 192, 8 193 and 16 384
    k-mers -- 4, 2 and 1 wavefronts per workgroup -- in the host forms, the device forms and the kept-reads forms, against the Python
    restatements; one k-mer more is SDT_EINVAL with the outputs untouched (profile, correct, select and trim), also when the read that
    is too long comes in a later piece than a read that fits"""
    import torch
    c = long_case(K)
    eb = long_expected(c, "b")
    n = len(c["boffs"]) - 1
    # the batch holds what it claims
    prof = eb["profile"]
    assert prof["kmers"][:-2].tolist() == [mk for mk in MK for _ in range(4)] and prof["kmers"][-2:].tolist() == [0, 1]
    assert all(prof["found"][4 * i] == mk and prof["found"][4 * i + 1] == mk for i, mk in enumerate(MK))      # prefix, reverse strand
    assert all(0 < prof["found"][4 * i + 2] < mk and prof["found"][4 * i + 3] == 0 for i, mk in enumerate(MK))
    assert int(eb["correct"][0]["fixed"].sum()) >= 20 and len(eb["correct"][2]) == int(eb["correct"][0]["fixed"].sum())
    assert all(0 < k < n for _, _, k in eb["select"])
    words = synth.pack_2bit(c["bcodes"])
    maxlen = int(np.diff(c["boffs"].astype(np.int64)).max())
    assert maxlen == STRIP_MAX_KMERS + K - 1
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_KEEP_READS) as g:
        g.push_reads(synth.pack_2bit(c["tcodes"]), c["toffs"])
        assert g.finish_count() == c["counts"]
        nt = len(c["toffs"]) - 1
        g.set_read_ordinal(nt, 1)
        g.keep_reads(synth.pack_2bit(c["kcodes"]), c["koffs"])       # kept behind the table's own reads, not counted

        def check_batch(what):
            ks.assert_cov_equal(g.profile_reads(words, c["boffs"], 2), prof, what + "profile_reads")
            fix, out, edits = g.correct_reads(words, c["boffs"], 2)
            rcu.assert_fix_equal(fix, eb["correct"][0], what + "correct_reads")
            assert (out == synth.pack_2bit(eb["correct"][1])).all() and edits.tolist() == eb["correct"][2].tolist()
            for (cv, seed), (wpick, wkeep, wkept) in zip(SELECT_SETTINGS, eb["select"]):
                pick, keep, kept = g.select_reads(words, c["boffs"], target=6, max_cv_pct=cv, seed=seed)
                rsu.assert_pick_equal(pick, wpick, what + f"select_reads cv {cv}")
                assert keep.tolist() == wkeep.tolist() and kept == wkept

        check_batch("host form: ")
        # device forms, max_read_len = the batch's longest
        d_w = torch.from_numpy(words.view(np.int32)).cuda()
        d_o = torch.from_numpy(c["boffs"].view(np.int64)).cuda()
        d_cov = torch.full((n, 6), -1, dtype=torch.int32, device="cuda")
        d_fix = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
        d_out = torch.full((len(words),), -1, dtype=torch.int32, device="cuda")
        d_ed = torch.full((len(eb["correct"][2]) + 5,), -1, dtype=torch.int64, device="cuda")
        d_pick = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
        d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.profile_reads_device(d_w, d_o, n, maxlen, 2, d_cov)
        ks.assert_cov_equal(as_records(d_cov, pkg.READ_COV_DTYPE), prof, "device form: profile")
        got = g.correct_reads_device(d_w, len(words), d_o, n, maxlen, 2, d_fix, d_out, d_ed, len(d_ed))
        assert got == len(eb["correct"][2])
        rcu.assert_fix_equal(as_records(d_fix, pkg.READ_FIX_DTYPE), eb["correct"][0], "device form: correct")
        assert (d_out.cpu().numpy().view(np.uint32) == synth.pack_2bit(eb["correct"][1])).all()
        assert sorted(d_ed.cpu().numpy().view(np.uint64)[:got].tolist()) == eb["correct"][2].tolist()
        for (cv, seed), (wpick, wkeep, wkept) in zip(SELECT_SETTINGS, eb["select"]):
            assert g.select_reads_device(d_w, d_o, n, maxlen, d_pick, d_keep, target=6, max_cv_pct=cv, seed=seed) == wkept
            rsu.assert_pick_equal(as_records(d_pick, pkg.READ_PICK_DTYPE), wpick, f"device form: select cv {cv}")
            assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
        # kept forms: by read ordinal over the table's own reads and the long reads behind them
        ek = long_expected(c, "k")
        total = len(ek["offs"]) - 1
        assert total == nt + 6 and int(ek["correct"][0]["fixed"][nt:].sum()) >= 1
        cov, nk = g.profile_kept_reads(total, 2)
        assert nk == total
        ks.assert_cov_equal(cov, ek["profile"], "kept form: profile")
        fix, nk, edits = g.correct_kept_reads(total, 2)
        assert nk == total and edits.tolist() == ek["correct"][2].tolist()
        rcu.assert_fix_equal(fix, ek["correct"][0], "kept form: correct")
        for (cv, seed), (wpick, wkeep, wkept) in zip(SELECT_SETTINGS, ek["select"]):
            pick, nk, kept = g.select_kept_reads(total, [], target=6, max_cv_pct=cv, seed=seed)
            assert (nk, kept) == (total, wkept)
            rsu.assert_pick_equal(pick, wpick, f"kept form: select cv {cv}")
        # one k-mer more: refused by the host-side check, nothing written, and the context answers the batch as before
        over, ooffs = concat([c["tx"][:100].copy(), c["tx"][:STRIP_MAX_KMERS + K].copy()])
        owords = synth.pack_2bit(over)
        lib, ctx = g.lib, g._ctx
        cov, fix, pick, trim = (np.full(2 * w, 0xABABABAB, dtype=np.uint32) for w in (6, 4, 4, 6))      # records of 6, 4, 4 and 6 words
        keep = np.full(2, 0xAB, dtype=np.uint8)
        outw = np.full(len(owords), 0xABABABAB, dtype=np.uint32)
        import ctypes
        ne, nkept = ctypes.c_uint64(77), ctypes.c_uint64(77)
        prm = pkg.NormParams(6, 150, 1)
        tprm = pkg.TrimParams(2, 0, 0, 0)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        calls = [lambda: lib.sdt_gpu_profile_reads(ctx, p(owords), owords.size, p(ooffs), 2, 2, p(cov)),
                 lambda: lib.sdt_gpu_correct_reads(ctx, p(owords), owords.size, p(ooffs), 2, 2, p(fix), p(outw), None, 0, ctypes.byref(ne)),
                 lambda: lib.sdt_gpu_select_reads(ctx, p(owords), owords.size, p(ooffs), 2, 0, ctypes.addressof(prm), p(pick), p(keep), ctypes.byref(nkept)),
                 lambda: lib.sdt_gpu_trim_reads(ctx, p(owords), owords.size, p(ooffs), 2, ctypes.addressof(tprm), p(trim), p(keep), ctypes.byref(nkept))]
        # as one piece, and with the 100-base read as a piece of its own ahead of the long one: the whole call is refused
        for piece in (None, "1"):
            if piece:
                monkeypatch.setenv("SDT_SEARCH_CHUNK", piece)
            for call in calls:
                assert call() == pkg.SDT_EINVAL
                msg = lib.sdt_gpu_last_error().decode()
                assert str(STRIP_MAX_KMERS + K) in msg and str(STRIP_MAX_KMERS) in msg, msg
            for a in (cov, fix, pick, trim):
                assert (a == 0xABABABAB).all(), piece
            assert (keep == 0xAB).all() and (outw == 0xABABABAB).all(), piece
        monkeypatch.delenv("SDT_SEARCH_CHUNK")
        d_ow = torch.from_numpy(owords.view(np.int32)).cuda()
        d_oo = torch.from_numpy(ooffs.view(np.int64)).cuda()
        d2 = torch.full((2, 6), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for call in (lambda: g.profile_reads_device(d_ow, d_oo, 2, STRIP_MAX_KMERS + K, 2, d2),
                     lambda: g.correct_reads_device(d_ow, len(owords), d_oo, 2, STRIP_MAX_KMERS + K, 2, d2),
                     lambda: g.select_reads_device(d_ow, d_oo, 2, STRIP_MAX_KMERS + K, d2, target=6)):
            with pytest.raises(pkg.SdtError) as e:
                call()
            assert e.value.code == pkg.SDT_EINVAL
        assert (d2.cpu().numpy() == -1).all()
        ks.assert_cov_equal(g.profile_reads(words, c["boffs"], 2), prof, "after the refusals: profile_reads")


# ---- 5. map stage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [31])
def test_map_stage_at_long_reads_and_long_contigs(pkg, synth, K):
    """30 contigs of 300 bases and one of 70 000: contig positions past 16 bits (100-base reads from beyond 65 536, either strand), and
    reads on both sides of every change of the launch geometry -- 1 496 | 1 497 and 3 032 | 3 033 k-mers (4, 2, 1 wavefronts per
    workgroup) -- and of the last length the call takes, 8 152 k-mers: hits, best hit and footprint flag are the oracle's"""
    rng = np.random.default_rng(50)
    ctgs = [rng.integers(0, 4, size=300).astype(np.uint8) for _ in range(30)] + [rng.integers(0, 4, size=70_000).astype(np.uint8)]
    big = ctgs[-1]
    ids = np.arange(1, 32, dtype=np.uint32)
    lens = np.array([len(x) for x in ctgs], dtype=np.uint32)
    o = mu.MapOracle(K, 4, 1)
    o.set_contig_index(lens, np.zeros(31, dtype=np.int32), 31)
    for i, x in zip(ids, ctgs):
        o.add_contig(x, int(i))
    ccodes, coffs = concat(ctgs)
    reads = []
    # 100-base reads: forward and reverse-complemented from past 65 536 (the STORED positions of their k-mers need more than 16
    # bits on either strand), and reverse-complemented from the contig's first bases (a hit on the other strand is reported in the
    # twin's coordinates: there the REPORTED offset passes 65 536)
    for j in range(30):
        p = 100 * j + 3 if j % 3 == 2 else 65_536 + 140 * j + 3
        r = big[p:p + 100].copy()
        reads.append(revcomp(r) if j % 3 else r)
    for i, mk in enumerate((ALIGN_WAVE_STEPS[0], ALIGN_WAVE_STEPS[0] + 1, ALIGN_WAVE_STEPS[1], ALIGN_WAVE_STEPS[1] + 1, ALIGN_MAX_KMERS)):
        p = 1000 + 5000 * i
        r = big[p:p + mk + K - 1].copy()
        r[500::900] = (r[500::900] + 1) & 3                           # a few substitutions: the hit breaks and resumes
        reads.append(revcomp(r) if i % 2 else r)
    reads.append(np.concatenate([ctgs[2][:150], big[60_000:60_000 + ALIGN_MAX_KMERS + K - 1 - 150]]))      # two contigs in one read
    assert len(reads[-1]) == ALIGN_MAX_KMERS + K - 1
    rcodes, roffs = concat(reads)
    with pkg.PregraphGPU(K, est_distinct=1 << 12, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        # a contig of 2^24 bases: positions are 24-bit.  Refused before any device work; the context indexes normally afterwards
        huge = np.zeros((1 << 24) // 16 + 4, dtype=np.uint32)
        with pytest.raises(pkg.SdtError) as e:
            g.index_contigs(huge, np.array([0, 1 << 24], dtype=np.uint64), ids[:1])
        assert e.value.code == pkg.SDT_EINVAL and str(1 << 24) in str(e.value) and "24-bit" in str(e.value)
        g.index_contigs(synth.pack_2bit(ccodes), coffs, ids)
        g.set_contig_table(np.concatenate([[0], lens]).astype(np.uint32), np.arange(32, dtype=np.uint32))
        kmers, nodes = g.finish_count()
        assert (nodes, kmers) == o.counts()
        assert kmers == 30 * (300 - K + 1) + 70_000 - K + 1
        # one k-mer more than the call takes: refused before the index is frozen, so this comes first and changes nothing
        over = big[:ALIGN_MAX_KMERS + K].copy()
        with pytest.raises(pkg.SdtError) as e:
            g.align_reads(synth.pack_2bit(over), np.array([0, len(over)], dtype=np.uint64), align_len_all=K + 4)
        assert e.value.code == pkg.SDT_EINVAL and str(len(over)) in str(e.value)
        info_w, hits = g.align_reads(synth.pack_2bit(rcodes), roffs, align_len_all=K + 4)
        past16 = 0
        for r, codes in enumerate(reads):
            n, want, best, foot = o.map_read(codes, K + 4)
            w = int(info_w[r])
            start, nh, b, f, ov = w & ((1 << 40) - 1), (w >> 40) & 255, (w >> 48) & 255, (w >> 56) & 1, (w >> 57) & 1
            assert ov == 0 and n >= 1 and nh == n, r
            got = [(int(h[0]), int(np.int32(h[1])), int(h[2]), int(h[3]) & 0x7FFFFFFF, "-" if int(h[3]) >> 31 else "+")
                   for h in [hits[r]] + list(hits[start:start + nh - 1])]
            assert got == want, r
            assert (b, f) == (best, foot), r
            past16 += sum(h[0] == 31 and h[1] >= 65_536 for h in got)
        # 10 forward reads from past 65 536 and 10 reverse reads from the contig's start, one exact hit each (no substitutions in
        # them, no repeats in random contigs) -- the oracle's hit lists above are what is compared; this only says the case is there
        assert past16 >= 20
        stored_past16 = [o.map_read(reads[j], K + 4)[1][0] for j in range(30) if j % 3 != 2]
        assert len(stored_past16) == 20 and sum(h[4] == "-" for h in stored_past16) == 10
        assert sum(len(x) - K + 1 > ALIGN_WAVE_STEPS[1] for x in reads) >= 3
