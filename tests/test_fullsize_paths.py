"""The branches of pass 1, the read stages and the staged transfers that only a full-size input reaches, at test size.

Everywhere else in the suite the input's CONTENT picks the path.  Here its SIZE does: a final bucket cut into several count items (A), several
count launches per flush (B), several batches inside one call (C), a level-1 bucket split over several level-2 items (D), base offsets at and
past 2^32 (E), transfers that go through the ring of pinned buffers in pieces (F).  A-D shrink the threshold with the library's size knobs
(csrc/sdt_pipeline.hpp; test hooks, read when the library is loaded: a child process per case, tests/fullsize_paths_util.py); E and F bring
the size.  Everything is integer-exact: every node of every case is compared with the oracle (oracle/libsdt_oracle.so) as
test_node_table_equals_oracle does, on row-sorted numpy arrays.

Out of scope: OUTPUT streams past 2^32 bases (the compactions write from base 0 here) -- checking them would take a gigabyte of expected
output."""
import numpy as np
import pytest

import oracle_binding as ob
import fullsize_paths_util as fu

gpu = pytest.mark.gpu

PART, TRACK = 2, 4                                            # SDT_FLAG_PARTITION, SDT_FLAG_TRACK_FIRST
CAP2 = 16                                                     # records per level-2 chunk (SK_CAP2, csrc/sdt_superkmer.cuh)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def brief(res):
    """the counters of a child's runs that say which path ran"""
    return [{k: r[k] for k in ("merges", "chunks_l1", "chunks_l2", "batches")} for r in res["runs"]], res["gpu_seconds"]


def max_run(K):
    """k-mers a record holds at most (sk_max_run, csrc/sdt_superkmer.cuh)"""
    nw = 1 if K <= 31 else (2 if K <= 63 else 4)
    cap, n = 32 * (2 if nw == 1 else (4 if nw == 2 else 6)) - K - 1, 64
    while n > cap:
        n //= 2
    return n


# ---- the helper, on the CPU -------------------------------------------------------------------------------------------------------------
S_STRADDLE = fu.TWO32 - 1000 - 5                             # the first reads below 2^32, one across it, the rest above; S & 15 != 0
S_ABOVE = fu.TWO32 + 16 * 1000 + 11                          # wholly above


@pytest.mark.parametrize("S", [0, S_STRADDLE, S_ABOVE])
def test_place_reads_round_trip(S):
    """place_reads: unpacking the words at the returned offsets gives the reads back; only the small piece exists on the host"""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 200, size=300)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes = rng.integers(0, 4, size=int(offs[-1]), dtype=np.uint8)
    words, w0, aoffs = fu.place_reads(codes, offs, S)
    assert w0 == S >> 4 and int(aoffs[0]) == S and (np.diff(aoffs.astype(np.int64)) == lens).all()
    assert words.nbytes < 1 << 20 and len(words) == ((S & 15) + len(codes) + 15) // 16 + 4
    assert (fu.unpack_placed(words, w0, aoffs) == codes).all()
    for r in (0, 7, len(lens) - 1):                         # base by base, from the definition of the format
        for j in (0, int(lens[r]) - 1):
            i = int(aoffs[r]) + j
            assert (int(words[(i >> 4) - w0]) >> (30 - 2 * (i & 15))) & 3 == codes[int(offs[r]) + j]
    lead = (int(words[0]) >> (32 - 2 * (S & 15))) if S & 15 else 0
    assert lead == 0 and not words[-4:].any()
    if S == S_STRADDLE:
        assert S & 15 and int(aoffs[0]) < fu.TWO32 < int(aoffs[-1])
        assert ((aoffs[:-1] < fu.TWO32) & (aoffs[1:] > fu.TWO32)).sum() == 1      # one read straddles 2^32
    if S == S_ABOVE:
        assert S & 15 and int(aoffs[0]) > fu.TWO32


# ---- A: a final bucket cut into several count items ---------------------------------------------------------------------------------------
A_HOT, A_L = 12000, 150


def a_input(synth, K, kind):
    def make():
        codes, offs = fu.hot_reads(A_HOT, A_L) if kind == "hot" else fu.mixed_reads(synth, K, A_HOT, A_L)
        ans = fu.oracle_answer(ob, K, [(codes, offs)])
        return dict(ans, codes=codes, offs=offs)
    return cached(("A", K, kind), make)


@gpu
@pytest.mark.parametrize("kind", ["hot", "mixed"])
@pytest.mark.parametrize("K", [21, 45, 75])
def test_count_stage_with_cut_buckets(pkg, synth, tmp_path, K, kind):
    """SDT_SK_COUNT_ITEM_CHUNKS=64 (product: 2048): a final bucket of more than 64 level-2 chunks becomes several items that are not
    WHOLE; several workgroups merge the same keys into the node table at once, by compare-and-swap instead of the owned plain stores.
    With and without first-occurrence tracking, 1-, 2- and 4-word keys.

    That a bucket was cut is a pigeonhole condition: the distinct keys of the hot input touch B final buckets, and the batch has more than
    64 B level-2 chunks.  The numbers: 12 000 hot reads of 150 bases hold 12 000 (150 - K + 1) k-mers = 1.56 M / 1.27 M / 0.91 M at
    K = 21 / 45 / 75; a record holds at most 32 / 64 / 64 of them and a chunk 16 records, so there are at least 3046 / 1242 / 890 chunks;
    poly-A and the six rotations of the repeat are at most 7 keys, 64 B <= 448."""
    arrays = a_input(synth, K, kind)
    if kind == "hot":
        B = fu.final_buckets_touched(pkg, dict(arrays, K=K))
        assert B <= 7 and int(arrays["kmers"]) // (CAP2 * max_run(K)) > 64 * B
    res = fu.run_child(tmp_path, f"A_{kind}_{K}", {"SDT_SK_COUNT_ITEM_CHUNKS": 64},
                       dict(K=K, flags=[PART, PART | TRACK], est_distinct=1 << 16, steps=[["push", 0, len(arrays["offs"]) - 1]]), arrays, timeout=300)
    print(K, kind, brief(res))
    if kind == "hot":
        for run in res["runs"]:
            assert run["chunks_l2"] > 64 * B, (run["chunks_l2"], B)


# ---- B: several count launches per flush ----------------------------------------------------------------------------------------------
B_K, B_L, B_FIRST, B_REST = 31, 150, 1500, 27000


def b_input(synth):
    def make():
        tx = synth.make_transcriptome(25, seed=B_K)
        codes, offs = synth.sample_reads(*tx, n_reads=B_FIRST + B_REST, read_len=B_L, seed=B_K + 1, err=0.003)
        assert (np.diff(offs.astype(np.int64)) == B_L).all()
        return dict(fu.oracle_answer(ob, B_K, [(codes, offs)]), codes=codes, offs=offs)
    return cached("B", make)


@gpu
@pytest.mark.parametrize("case,est", [("joined", 1 << 23), ("grown", 1 << 12), ("first_flush", 1 << 16)])
def test_several_count_launches_per_flush(pkg, synth, tmp_path, case, est):
    """SDT_SK_COUNT_KMERS_LOG2=20 (product: 29): a flush of more than 2^20 k-mers is counted by several launches (sk_count_all).

    1 500 reads are pushed and counted first, so that the rate of new nodes is known (`kmers_known`); then ONE push of 27 000 reads of 150
    bases, 27 000 x 120 = 3 240 000 k-mers > 3 x 2^20.  The plan (sk_plan_count_items) walks the final buckets in order and cuts a launch
    whenever `acc + km > limit`; no bucket of this input holds 2^20 k-mers, so every launch holds at most 2^20, which makes at least
    ceil(3 240 000 / 2^20) = 4 of them, and two neighbouring launches together hold more than 2^20, which makes at most 7.
      joined:      a table of 2^23 slots' worth -- neither the load rule nor the 95 % rule needs a look at the device, the planned launches
                   behind the first join it (one kernel over several planned launches, `next_item + launch` of the first)
      grown:       est_distinct = 2^12 -- the table holds the 1 500 reads' nodes and little more; every launch's bound (its own k-mers, about
                   2^20: the guess from the rate, + 2^22, is larger) asks for room the table does not have: ensure_room grows it for that
                   launch alone, the next one does not fit the load rule and cannot join, the table grows between them
      first_flush: no small push first, the whole input is the first flush (`kmers_known == 0`: first limit 2^26, one launch at this size)"""
    arrays = b_input(synth)
    n = B_FIRST + B_REST
    steps = [["push", 0, n]] if case == "first_flush" else [["push", 0, B_FIRST], ["finish"], ["push", B_FIRST, n]]
    assert B_REST * (B_L - B_K + 1) >= 3 << 20
    res = fu.run_child(tmp_path, f"B_{case}", {"SDT_SK_COUNT_KMERS_LOG2": 20},
                       dict(K=B_K, flags=[PART, PART | TRACK], est_distinct=est, steps=steps), arrays, timeout=300)
    print(case, brief(res))


# ---- C: several batches inside one call -----------------------------------------------------------------------------------------------
C_K, C_L, C_READS = 31, 150, 158000


def c_input(synth):
    def make():
        tx = synth.make_transcriptome(20, seed=C_K)
        codes, offs = synth.sample_reads(*tx, n_reads=C_READS, read_len=C_L, seed=C_K + 1, err=0.0004)
        assert (np.diff(offs.astype(np.int64)) == C_L).all()
        ans = fu.oracle_answer(ob, C_K, [(codes, offs)], nsets=8)
        assert int(ans["kmers"]) == C_READS * (C_L - C_K + 1) > (1 << 24) + (1 << 21) and int(ans["nodes"]) < 500_000
        return dict(ans, codes=codes, offs=offs)
    return cached("C", make)


@gpu
@pytest.mark.parametrize("call", ["device", "push"])
def test_several_batches_inside_one_call(pkg, synth, tmp_path, call):
    """SDT_SK_BATCH_LOG2=24, the smallest batch the clamp allows (product: 2^35): ONE count_reads_device call / ONE push_reads call of
    158 000 x 120 = 18 960 000 k-mers > 2^24 + 2^21 does not fit the pools; sk_scatter flushes in mid-call and goes on with the rest of
    the reads (the read cursor r0, the ordinals of the second launch).  At the clamp's minimum the pools are already the largest the knob
    allows (`cap_is_max`): the flush in mid-call runs, the doubling of the pools behind it does not.  Few transcripts, few errors: under
    500 K nodes."""
    arrays = c_input(synth)
    res = fu.run_child(tmp_path, f"C_{call}", {"SDT_SK_BATCH_LOG2": 24},
                       dict(K=C_K, flags=[PART, PART | TRACK], est_distinct=1 << 20, steps=[[call, 0, C_READS]]), arrays, timeout=300)
    print(call, brief(res))
    for run in res["runs"]:
        assert run["batches"] >= 2, run


# ---- D: a level-1 bucket split over several level-2 work items ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K,kind,reps", [(31, "mixed", 1), (63, "mixed", 1), (21, "hot", 5)])
def test_level1_bucket_over_several_level2_items(pkg, synth, tmp_path, K, kind, reps):
    """SDT_SK_ITEM_CHUNKS=16 (product: 4096): a level-1 bucket of more than 16 chunks is split by several workgroups of the level-2
    scatter, which append to the cursors of the same final buckets.
      mixed: more than 256 x 16 level-1 chunks in the batch, so some of the 256 level-1 buckets has more than 16 (asserted)
      hot:   all records in a handful of level-1 buckets -- 375 tiles of 32 reads put at least 4 chunks each into poly-A's; five runs in a
             row, each compared (contention shows now and then; the first mismatch fails)
    finish_count raises on SDT_ESTATE: the library's conservation check (k-mers cut into records == k-mers counted) stays silent."""
    arrays = a_input(synth, K, kind)
    res = fu.run_child(tmp_path, f"D_{kind}_{K}", {"SDT_SK_ITEM_CHUNKS": 16},
                       dict(K=K, flags=[PART], est_distinct=1 << 16, reps=reps, steps=[["push", 0, len(arrays["offs"]) - 1], ["finish"]]), arrays,
                       timeout=300)
    print(K, kind, brief(res))
    assert len(res["runs"]) == reps
    buckets1 = 256 if kind == "mixed" else fu.level1_buckets_touched(pkg, dict(arrays, K=K))
    assert buckets1 <= 7 or kind == "mixed"
    for run in res["runs"]:
        assert run["chunks_l1"] > 16 * buckets1, (run, buckets1)


# ---- E: base offsets at and past 2^32 -------------------------------------------------------------------------------------------------
BIG_WORDS = (1 << 28) + (1 << 16)                            # 1 GiB + 256 KiB of packed bases: base offsets up to 2^32 + 2^20


@pytest.fixture(scope="module")
def big_buffer():
    import torch
    buf = torch.zeros(BIG_WORDS, dtype=torch.int32, device="cuda:0")
    yield buf
    del buf
    torch.cuda.empty_cache()


class Placed:
    """reads copied into the big buffer at base S; the piece is zeroed again on exit"""

    def __init__(self, buf, codes, offs, S):
        import torch
        self.buf = buf
        words, self.w0, self.aoffs = fu.place_reads(codes, offs, S)
        self.nw = len(words)
        assert self.w0 + self.nw <= BIG_WORDS
        buf[self.w0: self.w0 + self.nw] = torch.from_numpy(words.view(np.int32)).cuda()
        self.d_offs = torch.from_numpy(self.aoffs.astype(np.int64)).cuda()
        self.n = len(offs) - 1
        self.maxlen = int(np.diff(self.aoffs.astype(np.int64)).max())
        torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.synchronize()
        self.buf[self.w0: self.w0 + self.nw].zero_()
        torch.cuda.synchronize()


def assert_high(S, aoffs):
    if S == S_STRADDLE:
        assert int(aoffs[0]) < fu.TWO32 and ((aoffs[:-1] < fu.TWO32) & (aoffs[1:] > fu.TWO32)).sum() == 1 and int(aoffs[-1]) > fu.TWO32
    else:
        assert int(aoffs[0]) >= fu.TWO32


def e_pass1_input(synth, K):
    def make():
        L = 150 if K <= 31 else 250
        tx = synth.make_transcriptome(12, seed=K)
        codes, offs = synth.sample_reads(*tx, n_reads=2000, read_len=L, seed=K + 1, err=0.004, ragged=True)
        return dict(fu.oracle_answer(ob, K, [(codes, offs)]), codes=codes, offs=offs)
    return cached(("E1", K), make)


@gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("K", [31, 63])
def test_count_reads_device_at_offsets_past_2_32(pkg, synth, big_buffer, K, mode):
    """count_reads_device, both kernel families: 2 000 ragged reads that lie across 2^32 bases (one read straddles it) and wholly above
    it, and the same reads at S & 15 near base 0 -- every node against the oracle each time"""
    arrays = e_pass1_input(synth, K)
    for S in (S_STRADDLE, S_ABOVE, S_STRADDLE & 15):
        with Placed(big_buffer, arrays["codes"], arrays["offs"], S) as p:
            if S > 15:
                assert_high(S, p.aoffs)
            with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=mode | TRACK) as g:
                g.count_reads_device(big_buffer, BIG_WORDS, p.d_offs, p.n, p.maxlen)
                fu.compare_with_answer(g, arrays, True, f"S={S} mode={mode}")


# ---- F: transfers in pieces -----------------------------------------------------------------------------------------------------------
PIECE = 32 << 20                                             # BigStage::CH (csrc/sdt_gpu.hip): from 32 MiB on a copy goes through 4 pinned buffers


def f_input(K, n_reads):
    def make():
        rng = np.random.default_rng(K)
        L = 250
        codes = rng.integers(0, 4, size=n_reads * L, dtype=np.uint8)
        offs = np.arange(n_reads + 1, dtype=np.uint64) * L
        return dict(fu.oracle_answer(ob, K, [(codes, offs)], nsets=8, ds=(0,)), codes=codes, offs=offs)
    return cached(("F", K), make)


@gpu
@pytest.mark.parametrize("K,n_reads,key_pieces", [(127, 35000, 5), (63, 11800, 2)])
def test_transfers_in_pieces(pkg, synth, K, n_reads, key_pieces):
    """Random reads: almost every k-mer is a node.  K = 127: 4.3 M nodes x 32 bytes of key > 128 MiB = 32 MiB x 4, five pieces -- the fifth
    reuses the first pinned buffer and its event, the download's drain loop lags three pieces behind.  K = 63: 2.2 M nodes x 16 bytes =
    34 MiB, two pieces with a short last one, while the 4-byte arrays stay below one piece and take the plain path.
      down: export_nodes against the oracle's export (keys, links, flags, counts as row-sorted arrays); layout_sorted_keys and
            export_ordered, whose keys come down through the ring, against export_nodes
      up:   set_node_index and update_nodes (keys through the ring) with new link words, flags kept; layout_apply (the order, 8 bytes per
            node) and update_nodes_by_index (the node numbers); export again must give the updated arrays"""
    a = f_input(K, n_reads)
    nodes, nw = int(a["nodes"]), (4 if K > 63 else 2)
    assert (nodes * nw * 8 - 1) // PIECE + 1 == key_pieces and nodes * nw * 8 % PIECE
    if K == 127:
        assert nodes * nw * 8 > 32 * (1 << 20) * 4 and nodes * 8 > PIECE
    else:
        assert nodes * 4 < PIECE
    with pkg.PregraphGPU(K, est_distinct=nodes + nodes // 4, flags=TRACK) as g:
        g.push_reads(synth.pack_2bit(a["codes"]), a["offs"])
        assert g.finish_count() == (int(a["kmers"]), nodes)
        hist, linear = g.mark_and_hist()
        assert linear == int(a["linear0"]) and (hist == a["hist0"]).all()
        fu.assert_table(fu.gpu_table(g), a, 0, "export_nodes")
        ek, el, erf, ec, first = g.export_nodes(with_first=True)              # (the table's own order, for `first`)
        # up by key
        h = (np.arange(nodes, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(17)
        l2 = (el & np.uint32(0xFF000000)) | (h & np.uint64(0xFFFFFF)).astype(np.uint32)
        rf2 = (erf & np.uint32(0xFF000000)) | ((h >> np.uint64(24)) & np.uint64(0xFFFFFF)).astype(np.uint32)
        g.set_node_index(ek)
        g.update_nodes(ek, l2, rf2)
        k3, l3, rf3, c3 = g.export_nodes()
        o2, o3 = fu.row_order(ek), fu.row_order(k3)
        assert (k3[o3] == ek[o2]).all() and (l3[o3] == l2[o2]).all() and (c3[o3] == ec[o2]).all()
        assert ((rf3[o3] & 0x3FFFFFF) == (rf2[o2] & 0x3FFFFFF)).all()
        # down through the ring: the keys by first occurrence (one set), then in an order of the host's choosing
        by_first = np.argsort(first, kind="stable")
        skeys, ss = g.layout_sorted_keys(1, nw)
        assert [int(x) for x in ss] == [0, nodes] and (skeys == ek[by_first]).all()
        order = np.random.default_rng(1).permutation(nodes).astype(np.uint64)
        g.layout_apply(order)
        src = by_first[order.astype(np.int64)]
        k4, l4, r4, c4 = g.export_ordered()
        assert (k4 == ek[src]).all() and (l4 == l2[src]).all() and (c4 == ec[src]).all() and ((r4 & 0x3FFFFFF) == (rf2[src] & 0x3FFFFFF)).all()
        # up by node number
        l5 = l4 ^ np.uint32(0x5A5A5A)
        r5 = r4 ^ np.uint32(0x0F0F0F)
        g.update_nodes_by_index(np.arange(nodes, dtype=np.uint64), l5, r5)
        k6, l6, r6, c6 = g.export_ordered()
        assert (k6 == k4).all() and (l6 == l5).all() and (c6 == c4).all() and ((r6 & 0x3FFFFFF) == (r5 & 0x3FFFFFF)).all()


# ---- E, the read stages: the _device forms on reads at and past 2^32 --------------------------------------------------------------------
def records(t, dtype):
    return t.cpu().numpy().view(np.uint8).reshape(-1).view(dtype).copy()


def assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: output {i} differs from the run near base 0"
        else:
            assert x == y, f"{what}: output {i}: {x} != {y}"


def at_placements(buf, codes, offs, call):
    """call(p) on the reads placed at S & 15 near base 0 and at S, for both S: the outputs must be the same, record for record and word
    for word -> the outputs of the four runs by placement"""
    out = {}
    for S in (S_STRADDLE, S_ABOVE):
        for s in (S & 15, S):
            with Placed(buf, codes, offs, s) as p:
                if s > 15:
                    assert_high(s, p.aoffs)
                out[s] = call(p)
        assert_same(out[S], out[S & 15], f"S={S}")
    return out


def kc_profile(kc, min_count):
    """the profile records from the per-read k-mer counts of the stages' utils (kmers, found, solid, min, lower median, max)"""
    out = np.zeros(len(kc), dtype=[(f, np.uint32) for f in ("kmers", "found", "solid", "min", "median", "max")])
    for r, c in enumerate(kc):
        if len(c):
            s = sorted(c)
            out[r] = (len(s), sum(x > 0 for x in s), sum(x >= min_count for x in s), s[0], s[(len(s) - 1) // 2], s[-1])
    return out


@gpu
def test_profile_and_correct_at_offsets_past_2_32(pkg, synth, big_buffer):
    """profile_reads_device and correct_reads_device on the case of test_read_correct.py (6 000 ragged reads + the hand-made ones), at the
    parameters of its device-form test; the corrected words are written at the reads' own (high) positions of a second buffer"""
    import torch
    import test_read_correct as trc
    from test_kmer_search import assert_cov_equal
    K, mc = 31, 3
    c = trc.case(K)
    wfix, wout, wedits = trc.expected(K, mc)
    n = len(c["boffs"]) - 1
    wcov = kc_profile(c["kc"], 2)
    out_buf = torch.zeros(BIG_WORDS, dtype=torch.int32, device="cuda:0")
    with trc.counted_context(pkg, synth, c) as g:
        def call(p):
            d_cov = torch.full((n, 6), -1, dtype=torch.int32, device="cuda:0")
            d_fix = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
            d_ed = torch.full((len(wedits) + 7,), -1, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            g.profile_reads_device(big_buffer, p.d_offs, n, p.maxlen, 2, d_cov)
            got = g.correct_reads_device(big_buffer, BIG_WORDS, p.d_offs, n, p.maxlen, mc, d_fix, out_buf, d_ed, len(d_ed))
            torch.cuda.synchronize()
            piece = out_buf[p.w0: p.w0 + p.nw].cpu().numpy().view(np.uint32).copy()
            assert not bool(out_buf[: p.w0].any()) and not bool(out_buf[p.w0 + p.nw:].any())       # nothing written anywhere else
            out_buf[p.w0: p.w0 + p.nw].zero_()
            ed = d_ed.cpu().numpy().view(np.uint64)
            assert (ed[got:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
            return records(d_cov, pkg.READ_COV_DTYPE), records(d_fix, pkg.READ_FIX_DTYPE), got, np.sort(ed[:got]), piece
        out = at_placements(big_buffer, c["batch"], c["boffs"], call)
    del out_buf
    for s, (cov, fix, got, ed, piece) in out.items():
        assert_cov_equal(cov, wcov, f"profile at {s}")
        trc.rc.assert_fix_equal(fix, wfix, f"correct at {s}")
        assert got == len(wedits) and ed.tolist() == wedits.tolist()
        assert (piece == fu.place_reads(wout, c["boffs"], s)[0]).all(), f"corrected words at {s}"


@gpu
@pytest.mark.parametrize("paired", [False, True])
def test_select_at_offsets_past_2_32(pkg, synth, big_buffer, paired):
    import torch
    import test_read_select as trs
    K, (cv, seed) = 31, trs.SETTINGS[1]
    c = trs.case(K)
    want = trs.expected(K, cv, seed, paired)
    n = len(c["boffs"]) - 1
    with trs.counted_context(pkg, synth, c) as g:
        def call(p):
            d_pick = torch.full((n, 4), -2, dtype=torch.int32, device="cuda:0")
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            kept = g.select_reads_device(big_buffer, p.d_offs, n, p.maxlen, d_pick, d_keep, target=trs.TARGET, max_cv_pct=cv, seed=seed, paired=paired)
            return records(d_pick, pkg.READ_PICK_DTYPE), d_keep.cpu().numpy(), kept
        out = at_placements(big_buffer, c["batch"], c["boffs"], call)
    for s, got in out.items():
        trs.assert_select(pkg, got, want, f"select at {s} paired={paired}")


@gpu
def test_trim_at_offsets_past_2_32(pkg, synth, big_buffer):
    import torch
    import test_read_trim as trt
    K = 31
    c = trt.case(K)
    n = len(c["boffs"]) - 1
    with trt.counted_context(pkg, synth, c) as g:
        for prm in (trt.settings(K)[4], trt.settings(K)[2]):
            want = trt.expected(K, prm)

            def call(p):
                d_trim = torch.full((n, 6), -2, dtype=torch.int32, device="cuda:0")
                d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                kept = g.trim_reads_device(big_buffer, p.d_offs, n, p.maxlen, d_trim, d_keep, *prm)
                return records(d_trim, pkg.READ_TRIM_DTYPE), d_keep.cpu().numpy(), kept
            for s, got in at_placements(big_buffer, c["batch"], c["boffs"], call).items():
                trt.assert_trim(pkg, got, want, f"trim at {s} {prm}")


@gpu
@pytest.mark.parametrize("paired", [False, True])
def test_dedup_at_offsets_past_2_32(pkg, synth, big_buffer, paired):
    import torch
    import read_dedup_util as rd
    from test_read_dedup import assert_dedup
    c = rd.paired_case() if paired else rd.case()
    codes, offs = c["codes"], c["offs"]
    n = len(offs) - 1
    want = rd.expect_dedup(codes, offs, paired=paired)
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        def call(p):
            d_dup = torch.full((n, 2), -3, dtype=torch.int64, device="cuda:0")
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            kept = g.dedup_reads_device(big_buffer, p.d_offs, n, d_dup, d_keep, paired=paired)
            return records(d_dup, pkg.READ_DUP_DTYPE), d_keep.cpu().numpy(), kept
        for s, got in at_placements(big_buffer, codes, offs, call).items():
            assert_dedup(pkg, got, want, f"dedup at {s} paired={paired}")


@gpu
def test_clip_and_overlap_at_offsets_past_2_32(pkg, synth, big_buffer):
    import torch
    import read_clip_util as rcl
    import read_overlap_util as ru
    from test_read_clip import assert_clip
    from test_read_overlap import assert_overlap
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        c = rcl.case()
        n = len(c["offs"]) - 1

        def clip(p):
            d_clip = torch.full((n, 6), -3, dtype=torch.int32, device="cuda:0")
            d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            kept = g.clip_reads_device(big_buffer, p.d_offs, n, d_clip, d_keep, c["adapters"], c["params"])
            return records(d_clip, pkg.READ_CLIP_DTYPE), d_keep.cpu().numpy(), kept
        for s, got in at_placements(big_buffer, c["codes"], c["offs"], clip).items():
            assert_clip(pkg, got, rcl.case_expect(), f"clip at {s}")
        o = ru.case()
        m = len(o["offs"]) - 1

        def overlap(p):
            d_ov = torch.full((m, 6), -3, dtype=torch.int32, device="cuda:0")
            d_keep = torch.full((m,), 7, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            kept = g.overlap_pairs_device(big_buffer, p.d_offs, m, d_ov, d_keep, o["params"])
            return records(d_ov, pkg.READ_OVERLAP_DTYPE), d_keep.cpu().numpy(), kept
        for s, got in at_placements(big_buffer, o["codes"], o["offs"], overlap).items():
            assert_overlap(pkg, got, ru.case_expect(), f"overlap at {s}")


@gpu
def test_complexity_and_screen_at_offsets_past_2_32(pkg, synth, big_buffer):
    """complexity_reads_device (filter and SDT_COMPLEXITY_TRIM) on its own case, and screen_reads_device (single reads; pairs) on the
    reads of the screen's case at k = 21 against the set of that case: records, keep bytes and the kept count against the restatement
    at every placement, and against the placement near base 0"""
    import torch
    import read_complexity_util as cu
    import read_screen_util as su
    from test_read_complexity import TRIM, assert_cx
    from test_read_screen import assert_screen, load_case
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        c = cu.case()
        n = len(c["offs"]) - 1
        for mode, prm, want in (("filter", c["params"], cu.case_expect()), ("trim", dict(c["params"], **TRIM), cu.case_expect(trim=True))):
            def complexity(p):
                d_cx = torch.full((n, 6), -3, dtype=torch.int32, device="cuda:0")
                d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                kept = g.complexity_reads_device(big_buffer, p.d_offs, n, d_cx, d_keep, prm)
                return records(d_cx, pkg.READ_COMPLEXITY_DTYPE), d_keep.cpu().numpy(), kept
            for s, got in at_placements(big_buffer, c["codes"], c["offs"], complexity).items():
                assert_cx(pkg, got, want, f"complexity ({mode}) at {s}")
        k = 21
        rc, d = su.read_case(k), su.set_dict(k)
        load_case(g, synth, k)
        for paired in (False, True):
            m = (len(rc["offs"]) - 1) & ~1 if paired else len(rc["offs"]) - 1         # (the case has an odd number of reads)
            want = su.expect_screen(rc["codes"], rc["offs"][:m + 1], k, d, su.params(), paired=paired, facts=rc["facts"][:m])

            def screen(p):
                d_rec = torch.full((m, 6), -3, dtype=torch.int32, device="cuda:0")
                d_keep = torch.full((m,), 7, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                kept = g.screen_reads_device(big_buffer, p.d_offs, m, d_rec, d_keep, paired=paired, params=su.params())
                return records(d_rec, pkg.READ_SCREEN_DTYPE), d_keep.cpu().numpy(), kept
            assert 0 < want[2] < m
            for s, got in at_placements(big_buffer, rc["codes"], rc["offs"], screen).items():
                assert_screen(pkg, got, want, f"screen at {s} paired={paired}")


@gpu
def test_quality_at_offsets_past_2_32(pkg):
    """quality_reads_device addresses BYTES, one per base, with its own arithmetic for the bytes in front of a read within its 32-bit
    word: the case of test_read_quality.py in a byte buffer of 2^32 + 2^20 bytes of its own, at byte offsets S (one read straddles
    2^32; all reads above it) and S & 3 (the same place within a word, near byte 0)"""
    import torch
    import read_quality_util as qu
    from test_read_quality import assert_q
    c = qu.case()
    n = len(c["offs"]) - 1
    quals = torch.from_numpy(c["quals"])
    assert S_STRADDLE & 3 and S_ABOVE & 3                   # (a read's first byte is not the first of its word)
    buf = torch.zeros(fu.TWO32 + (1 << 20), dtype=torch.uint8, device="cuda:0")
    try:
        out = {}
        with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
            for S in (S_STRADDLE, S_ABOVE):
                for s in (S & 3, S):
                    aoffs = c["offs"] + np.uint64(s)
                    if s > 3:
                        assert_high(s, aoffs)
                    assert int(aoffs[-1]) + 4 <= buf.numel()
                    buf[s: s + len(quals)] = quals.cuda()
                    d_o = torch.from_numpy(aoffs.view(np.int64)).cuda()
                    d_out = torch.full((n, 6), -3, dtype=torch.int32, device="cuda:0")
                    d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    kept = g.quality_reads_device(buf, d_o, n, d_out, d_keep, c["params"])
                    out[S, s] = (records(d_out, pkg.READ_QUALITY_DTYPE), d_keep.cpu().numpy(), kept)
                    buf[s: s + len(quals)].zero_()
                    torch.cuda.synchronize()
        assert len(out) == 4
        for (S, s), got in out.items():
            assert_q(pkg, got, qu.case_expect(), f"quality at byte {s}")
        runs = list(out.items())
        for i, (a, x) in enumerate(runs):
            for b, y in runs[i + 1:]:
                assert_same(x, y, f"bytes {a[1]} and {b[1]}")
    finally:
        del buf
        torch.cuda.empty_cache()


@gpu
def test_compactions_at_offsets_past_2_32(pkg, synth, big_buffer):
    """compact_reads_device and compact_trimmed_device: the input at the high offsets, the output from base 0 -- words, pad words and
    offsets; length_mix() forty times over (every length next to every other, reads that start at every base of a word), every third
    read dropped / the random ranges of the trim's own test"""
    import torch
    import read_select_util as rs
    import read_trim_util as rt
    from test_read_correct import concat
    from test_read_select_host import length_mix
    from test_read_trim_host import range_sets
    codes0, offs0 = length_mix()
    n0 = len(offs0) - 1
    codes, offs = concat([codes0[int(offs0[r]):int(offs0[r + 1])] for _ in range(40) for r in range(n0)])
    n = len(offs) - 1
    keep = (np.arange(n) % 3 != 1).astype(np.uint8)
    trim = np.tile(range_sets(offs0)["random ranges"], 40)
    words = rs.pack_words(codes)
    want_k = rs.expect_compact(words, offs, keep)
    want_t = rt.expect_compact_trimmed(words, offs, trim)
    assert len(want_k[0]) > 512 and len(want_t[0]) > 512
    cap = len(words) + 8
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        d_k = torch.from_numpy(keep).cuda()
        d_t = torch.from_numpy(trim.view(np.int32).reshape(n, 6)).cuda()

        def call(p):
            res = []
            for which in ("reads", "trimmed"):
                d_ow = torch.full((cap,), -1, dtype=torch.int32, device="cuda:0")
                d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                if which == "reads":
                    nr, nw = g.compact_reads_device(big_buffer, p.d_offs, n, d_k, d_ow, cap, d_oo)
                else:
                    nr, nw = g.compact_trimmed_device(big_buffer, p.d_offs, n, d_t, d_ow, cap, d_oo)
                res += [nr, nw, d_ow.cpu().numpy().view(np.uint32), d_oo.cpu().numpy().view(np.uint64)]
            return tuple(res)
        for s, got in at_placements(big_buffer, codes, offs, call).items():
            for (nr, nw, ow, oo), (ww, wo), what in ((got[:4], want_k, "compact_reads"), (got[4:], want_t, "compact_trimmed")):
                assert (nr, nw) == (len(wo) - 1, len(ww) - 4), (what, s)
                assert ow[:nw + 4].tolist() == ww.tolist() and (ow[nw + 4:] == 0xFFFFFFFF).all() and not ow[nw:nw + 4].any(), (what, s, "words")
                assert oo[:nr + 1].tolist() == wo.tolist(), (what, s, "offsets")


@gpu
def test_align_reads_device_at_offsets_past_2_32(pkg, synth, big_buffer):
    """align_reads_device on one of the small map cases: per read the hit count, the best hit, the footprint flag and the hits in order,
    against the host form (which test_map_stage_equals_oracle compares with the oracle read by read)"""
    import ctypes
    import torch
    import map_util as mu
    from test_gpu_parity import _index_case
    info = mu.load_case(mu.case_names()[0])
    codes, offs, _, _, _ = mu.case_reads(info)
    n = len(offs) - 1

    def per_read(info_w, hits):
        out = []
        for r in range(n):
            w = int(info_w[r])
            start, nh = w & ((1 << 40) - 1), (w >> 40) & 255
            out.append((nh, w >> 48) + ((tuple(hits[r].tolist()),) + tuple(tuple(h.tolist()) for h in hits[start:start + nh - 1]) if nh else ()))
        return out
    with pkg.PregraphGPU(mu.case_contigs(info)[0], est_distinct=1 << 12, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        _index_case(pkg, synth, info, g)
        g.finish_count()
        want = per_read(*g.align_reads(synth.pack_2bit(codes), offs, align_len_all=32))
        assert sum(1 for w in want if w[0]) > n // 2
        cap = 4 * n + 16

        def call(p):
            d_info = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
            d_hits = torch.zeros((cap, 4), dtype=torch.int32, device="cuda:0")
            nh = ctypes.c_uint64()
            torch.cuda.synchronize()
            rc = g.lib.sdt_gpu_align_reads_device(g._ctx, big_buffer.data_ptr(), p.d_offs.data_ptr(), n, p.maxlen, None, 32, d_info.data_ptr(),
                                                  d_hits.data_ptr(), cap, ctypes.byref(nh))
            assert rc == 0, g.lib.sdt_gpu_last_error().decode()
            torch.cuda.synchronize()
            got = per_read(d_info.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)[: nh.value])
            assert got == want, [(r, a, b) for r, (a, b) in enumerate(zip(got, want)) if a != b][:3]
            return (nh.value,)
        at_placements(big_buffer, codes, offs, call)
