"""GPU (-m gpu): the HIP path through the C ABI vs. the oracle and vs. the reference's golden files.
Bit-exact: integer work only."""
import numpy as np
import pytest

import oracle_binding as ob
import golden_util as gu

pytestmark = pytest.mark.gpu


def keys_to_int(keys):
    out = []
    for row in keys:
        v = 0
        for x in row:
            v = (v << 64) | int(x)
        out.append(v)
    return out


def node_dict_gpu(g):
    keys, l, rf, cnt = g.export_nodes()
    ki = keys_to_int(keys)
    return {k: (int(a), int(b) & 0xFFFFFF, int(b) >> 24, int(c)) for k, a, b, c in zip(ki, l, rf, cnt)}


def node_dict_oracle(o):
    keys, l, r, cnt, fl = o.export()
    ki = keys_to_int(keys)
    # oracle flags: bit0 linear, bit1 deleted, bit2 single -> kmer_t bitfield order linear, deleted, checked, single
    def f(x):
        x = int(x)
        return (x & 1) | ((x >> 1 & 1) << 1) | ((x >> 2 & 1) << 3)
    return {k: (int(a), int(b), f(c), int(d)) for k, a, b, c, d in zip(ki, l, r, fl, cnt)}


# the two pass-1 kernel families: SDT_FLAG_DIRECT (one atomic per occurrence) and SDT_FLAG_PARTITION (the locality pipeline: super-k-mer
# buckets counted in LDS, every generation of the LDS table merged into the node table)
MODES = [1, 2]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", gu.case_names())
def test_golden_case_kmerfreq_bit_identical(pkg, name, mode):
    """reference binary's *.kmerFreq reproduced byte for byte by the GPU path"""
    info = gu.load_case(name)
    K = pkg.clamp_K(info["K"], gu.VARIANT_MAXK[info["variant"]])
    codes, offs = gu.case_reads(info)
    from soapdenovo_trans_amd import synth
    words = synth.pack_2bit(codes)
    with pkg.PregraphGPU(K, est_distinct=1 << 17, flags=mode) as g:
        g.push_reads(words, offs)
        kmers, nodes = g.finish_count()
        assert kmers == info["kmer_in_reads"]
        assert nodes == info["nodes_allocated"]
        if info["d"]:
            assert g.delow(info["d"]) == info["kmer_removed"]
        hist, linear = g.mark_and_hist()
        assert linear == info["linear_nodes"]
        assert pkg.kmerfreq_text(hist) == gu.golden_text(info, "kmerFreq")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,L,ragged", [(13, 60, True), (23, 100, False), (23, 150, True), (31, 150, True), (31, 158, False), (31, 250, True), (21, 250, True), (33, 150, True),
                                        (63, 250, False), (65, 200, True), (97, 250, True), (127, 250, True),
                                        # reads of more than 256 k-mers leave the one-lane-per-read scatter for the strip kernel: its strips
                                        # (window <= 49 m-mers) with 1-word keys, its sparse table of window minima (longer windows) with 2- and 4-word keys
                                        (31, 330, True), (63, 400, True), (95, 420, False)])
def test_node_table_equals_oracle(pkg, synth, K, L, ragged, mode):
    """every node: key, 8 saturating link counters, count, single/linear/deleted flags"""
    tx = synth.make_transcriptome(25, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=6000, read_len=L, seed=K + 1, err=0.003, ragged=ragged)
    words = synth.pack_2bit(codes)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=mode) as g:        # small table: forces growth by rebuild
        half = len(offs) // 2
        # two pushes with different batch geometry (second batch starts mid-stream)
        w1 = synth.pack_2bit(codes[: int(offs[half])])
        g.push_reads(w1, offs[: half + 1])
        rest = codes[int(offs[half]):]
        g.push_reads(synth.pack_2bit(rest), offs[half:] - offs[half])
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
        for d in (0, 2):
            if d:
                assert g.delow(d) == o.delow(d)
            hist, linear = g.mark_and_hist()
            ohist, olinear = o.mark()
            assert linear == olinear
            assert (hist == ohist).all()
            assert node_dict_gpu(g) == node_dict_oracle(o)


@pytest.mark.parametrize("mode", MODES)
def test_saturation_and_hot_keys(pkg, synth, mode):
    """poly-A and tandem repeats: one key hit tens of thousands of times from every lane of a wave --
    6-bit counters must stop at 63, count must not (and must carry past 16 bits into aux)"""
    K = 21
    n, L = 1500, 100
    codes = np.zeros(n * L, dtype=np.uint8)                     # all A: one canonical k-mer, count = n*(L-K+1) = 120000
    codes[L * 1000:] = np.tile(np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8), (n - 1000) * L // 6 + 1)[: (n - 1000) * L]
    offs = (np.arange(n + 1) * L).astype(np.uint64)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=mode) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
        hist, linear = g.mark_and_hist()
        ohist, olinear = o.mark()
        assert (hist == ohist).all() and linear == olinear
        gd = node_dict_gpu(g)
        assert gd == node_dict_oracle(o)
        assert max(v[3] for v in gd.values()) > 65536


@pytest.mark.parametrize("K", list(range(17, 64, 2)))
def test_seq_scatter_every_window(pkg, synth, K):
    """the one-lane-per-read level-1 scatter has one instantiation per window length (every odd K from 17 to 63, 1- and
    2-word keys): each against the oracle -- ragged reads (some shorter than K), reads with more runs than the
    per-lane list holds, every node compared"""
    L = 100 if K <= 31 else 200
    tx = synth.make_transcriptome(12, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=2500, read_len=L, seed=K + 11, err=0.004, ragged=True)
    o = ob.Oracle(K, nsets=3)
    o.add_reads(codes, offs)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=MODES[-1]) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        hist, linear = g.mark_and_hist()
        ohist, olinear = o.mark()
        assert linear == olinear and (hist == ohist).all()
        assert node_dict_gpu(g) == node_dict_oracle(o)


@pytest.mark.parametrize("K,L", [(31, 150), (63, 250), (95, 250)])
def test_pool_overflow_takes_the_direct_path(pkg, synth, monkeypatch, K, L):
    """the pools of the locality pipeline are sized by a model, never for the worst case: a record that finds no chunk must go
    through put_kmerset directly and change nothing but the speed.  A level-1 pool of 48 chunks (test hook) overflows at once:
    most k-mers take the direct path, every node must still be the oracle's"""
    monkeypatch.setenv("SDT_SK_POOL_CHUNKS1", "48")
    tx = synth.make_transcriptome(20, seed=K + 3)
    codes, offs = synth.sample_reads(*tx, n_reads=5000, read_len=L, seed=K + 4, err=0.003, ragged=True)
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=MODES[-1] | pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        direct = g.stage_times()[1]["pool_direct"]
        assert 0 < direct <= o.kmers_in_reads() and direct > o.kmers_in_reads() // 2
        hist, linear = g.mark_and_hist()
        ohist, olinear = o.mark()
        assert linear == olinear and (hist == ohist).all()
        assert node_dict_gpu(g) == node_dict_oracle(o)
        _, _, _, _, first = g.export_nodes(with_first=True)
        assert sorted(first.tolist()) == sorted(o.export_first().tolist())


def test_hot_bucket_repeated(pkg, synth):
    """the hot-bucket input a hundred times through the locality pipeline: every lane of every workgroup appends to ONE
    level-2 cursor.  (A 1024-lane geometry of the level-2 scatter lost a chunk of 16 records in half of such runs while
    the lanes that wait for a chunk to be replaced kept adding to its cursor; the library's own conservation check --
    k-mers cut into records == k-mers counted -- must stay silent too.)"""
    K, n, L = 21, 1500, 100
    codes = np.zeros(n * L, dtype=np.uint8)
    codes[L * 1000:] = np.tile(np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8), (n - 1000) * L // 6 + 1)[: (n - 1000) * L]
    offs = (np.arange(n + 1) * L).astype(np.uint64)
    words = synth.pack_2bit(codes)
    for _ in range(100):
        with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=MODES[-1]) as g:
            g.push_reads(words, offs)
            assert g.finish_count() == (n * (L - K + 1), 7)


@pytest.mark.parametrize("mode", MODES)
def test_growth_when_later_data_is_all_new(pkg, synth, mode):
    """the pipeline sizes a count launch by the rate of new nodes seen so far; here the history lies: 40 000 copies of one
    read first (one new node per 40 000 occurrences), then random reads (every k-mer a new node) into a table that starts
    far too small -- the table must grow in time, nothing may be lost"""
    K, L = 31, 100
    rng = np.random.default_rng(9)
    one = rng.integers(0, 4, size=L, dtype=np.uint8)
    first = np.tile(one, 40_000)
    second = rng.integers(0, 4, size=60_000 * L, dtype=np.uint8)
    o = ob.Oracle(K, nsets=4)
    with pkg.PregraphGPU(K, est_distinct=1 << 12, flags=mode) as g:
        for codes in (first, second):
            offs = (np.arange(len(codes) // L + 1, dtype=np.uint64) * L)
            o.add_reads(codes, offs)
            g.push_reads(synth.pack_2bit(codes), offs)
            g.finish_count()                        # the second push meets a table sized for the first
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
        hist, linear = g.mark_and_hist()
        ohist, olinear = o.mark()
        assert linear == olinear and (hist == ohist).all()
        assert node_dict_gpu(g) == node_dict_oracle(o)


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(pkg, synth, mode):
    """empty batch, reads shorter than K+1 (skipped, prlHashReads.c:592), a read of exactly K+1, reset"""
    K = 25
    with pkg.PregraphGPU(K, flags=mode) as g:
        g.push_reads(np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint64))       # zero reads
        assert g.finish_count() == (0, 0)
        rng = np.random.default_rng(1)
        lens = np.array([0, 1, K - 1, K, K + 1, 3, K + 1, 200, K, K + 2], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        codes = rng.integers(0, 4, size=int(offs[-1]), dtype=np.uint8)
        o = ob.Oracle(K, nsets=2)
        o.add_reads(codes, offs)
        g.push_reads(synth.pack_2bit(codes), offs)
        assert g.finish_count() == (o.kmers_in_reads(), o.node_count())
        assert o.kmers_in_reads() == 2 + 2 + (200 - K + 1) + 3
        hist, _ = g.mark_and_hist()
        assert (hist == o.mark()[0]).all()
        g.reset()
        assert g.finish_count() == (0, 0)
        hist, lin = g.mark_and_hist()
        assert hist.sum() == 0 and lin == 0


@pytest.mark.parametrize("mode", MODES)
def test_device_resident_batch_and_properties(pkg, synth, mode):
    """device entry point on a torch-generated workload: size-independent properties + oracle on a slice"""
    import torch
    dev = torch.device("cuda:0")
    K, L, n = 31, 150, 200_000
    words, offsets, nwords = synth.torch_workload(n, L, T=300, device=dev, seed=11)
    torch.cuda.synchronize()
    with pkg.PregraphGPU(K, est_distinct=1 << 22, flags=mode) as g:
        g.count_reads_device(words, nwords, offsets, n, L)
        kmers, nodes = g.finish_count()
        assert kmers == n * (L - K + 1)
        hist, linear = g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        assert len(keys) == nodes
        assert hist.sum() == nodes                                   # every node lands in exactly one bin
        assert int(cnt.astype(np.uint64).sum()) == kmers             # counts add up to the occurrences
        assert len(set(keys[:, 0].tolist())) == nodes                # keys are distinct
        # each occurrence has exactly one left and one right neighbour slot or none: link sums <= count
        ls = sum(((l >> (6 * b)) & 63).astype(np.int64) for b in range(4))
        assert (ls <= cnt).all()
        # idempotence of the scan: marking twice gives the same histogram
        hist2, linear2 = g.mark_and_hist()
        assert (hist2 == hist).all() and linear2 == linear
        # oracle on the first 3000 reads, through the same device buffers
        sub = 3000
        hw = words.cpu().numpy().view(np.uint32)
        codes = np.zeros(sub * L, dtype=np.uint8)
        idx = np.arange(sub * L)
        codes[:] = (hw[idx >> 4] >> (30 - 2 * (idx & 15)).astype(np.uint32)) & 3
        g.reset()
        g.count_reads_device(words, nwords, offsets, sub, L)
        k2, n2 = g.finish_count()
        o = ob.Oracle(K, nsets=8)
        o.add_reads(codes, (np.arange(sub + 1) * L).astype(np.uint64))
        assert (k2, n2) == (o.kmers_in_reads(), o.node_count())
        assert (g.mark_and_hist()[0] == o.mark()[0]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,stride,base", [(21, 1, 0), (35, 2, 1), (71, 2, 0), (33, 1, 0), (65, 2, 1), (97, 2, 0)])
def test_first_occurrence_ordinals(pkg, synth, K, stride, base, mode):
    """SDT_FLAG_TRACK_FIRST: per node, the smallest (read ordinal << 16 | position) over its occurrences --
    the order the reference's table layout is a function of"""
    tx = synth.make_transcriptome(10, seed=2)
    codes, offs = synth.sample_reads(*tx, n_reads=1500, read_len=80, seed=3, ragged=True)
    want = {}
    for r in range(len(offs) - 1):
        keys, _, _, _ = ob.chop_read(codes[int(offs[r]):int(offs[r + 1])], K)
        for j, kw in enumerate(keys_to_int(keys)):
            o = ((base + r * stride) << 16) | j
            if kw not in want or o < want[kw]:
                want[kw] = o
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_TRACK_FIRST | mode) as g:      # small table: growth keeps them
        g.set_read_ordinal(base, stride)
        half = 700
        g.push_reads(synth.pack_2bit(codes[: int(offs[half])]), offs[: half + 1])
        g.push_reads(synth.pack_2bit(codes[int(offs[half]):]), offs[half:] - offs[half])      # ordinals continue
        g.finish_count()
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        got = dict(zip(keys_to_int(keys), (int(x) for x in first)))
        assert got == want
    with pkg.PregraphGPU(K) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        with pytest.raises(pkg.SdtError):
            g.export_nodes(with_first=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,L", [(31, 100), (63, 160)])
def test_async_and_fixed_length_pushes_equal_one_push(pkg, synth, K, L, mode):
    """sdt_gpu_push_reads_async / _fixed_async: many small batches that are copied at once and launched from a queue (with
    read ordinals set once, stride 2) must leave exactly the table of one synchronous push -- keys, links, counts, flags and
    first-occurrence ordinals -- whether the offsets cross PCIe or are made on the device"""
    tx = synth.make_transcriptome(30, seed=11)
    codes, offs = synth.sample_reads(*tx, n_reads=6400, read_len=L, seed=12)          # fixed length
    assert (np.diff(offs.astype(np.int64)) == L).all()

    def table(g):
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        order = np.lexsort(keys.T[::-1])
        return keys[order].tolist(), l[order].tolist(), rf[order].tolist(), cnt[order].tolist(), first[order].tolist()

    flags = pkg.SDT_FLAG_TRACK_FIRST | mode
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=flags) as g:
        g.set_read_ordinal(1, 2)
        g.push_reads(synth.pack_2bit(codes), offs)
        want_counts = g.finish_count()
        want = table(g)
    per = 640                                            # 10 batches; 640 * L bases is a multiple of 16: batches start on a word
    assert (per * L) % 16 == 0
    batches = [(np.ascontiguousarray(synth.pack_2bit(codes[r0 * L: (r0 + per) * L])), np.ascontiguousarray((np.arange(per + 1) * L).astype(np.uint64)))
               for r0 in range(0, 6400, per)]
    for fixed in (False, True):
        with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=flags) as g:
            g.set_read_ordinal(1, 2)
            g.hint_total_kmers(6400 * (L - K + 1))
            tickets = [g.push_reads_fixed_async(w, per, L) if fixed else g.push_reads_async(w, o) for w, o in batches]
            assert tickets == list(range(1, len(batches) + 1))
            g.push_wait(tickets[-1])
            assert g.finish_count() == want_counts
            assert table(g) == want, f"fixed={fixed}"


@pytest.mark.parametrize("K", [63, 97, 127])
def test_wide_key_publication_stress(pkg, synth, K):
    """multi-word keys are claimed with a CAS on the first word and published without a release fence
    (csrc/sdt_table.cuh): a lost or duplicated node would change the node count / histogram.  ~100 M occurrences,
    ~10 M new keys, every lane of the chip inserting at once."""
    import torch
    dev = torch.device("cuda:0")
    L, n = 250, 500_000
    words, offsets, nwords = synth.torch_workload(n, L, T=200, device=dev, seed=5)
    torch.cuda.synchronize()
    hw = words.cpu().numpy().view(np.uint32)
    idx = np.arange(n * L, dtype=np.int64)
    codes = ((hw[idx >> 4] >> (30 - 2 * (idx & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    o = ob.Oracle(K, nsets=8)
    o.add_reads(codes, (np.arange(n + 1, dtype=np.uint64) * L))
    ohist, olinear = o.mark()
    for rep in range(3):
        with pkg.PregraphGPU(K, est_distinct=1 << 20) as g:       # small table: growth under load too
            g.count_reads_device(words, nwords, offsets, n, L)
            kmers, nodes = g.finish_count()
            assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
            hist, linear = g.mark_and_hist()
            assert linear == olinear and (hist == ohist).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [95, 97, 127])
def test_wide_key_poly_g_tails(pkg, synth, K, mode):
    """4-word keys whose LOW words are all ones (64+ trailing G's, the NextSeq poly-G tail) equal the cleared-slot
    sentinel in key[2..3]: the plain-load fast path must not take a half-published entry for them (csrc/sdt_table.cuh).
    Reads = transcript prefixes of varying length followed by a G run, so thousands of distinct keys share ~0 low words
    with many different high words and are inserted from every CU at once."""
    rng = np.random.default_rng(K)
    tx = synth.make_transcriptome(40, seed=K + 3)
    codes0, starts0 = tx[0], tx[1]
    n, L = 60000, 250
    reads = np.full((n, L), 3, dtype=np.uint8)                   # G = 3
    t = rng.integers(0, len(starts0) - 1, size=n)
    pre = rng.integers(K - 70 if K > 70 else 5, L - 70, size=n)  # prefix length: the G tail is at least 70 bases
    pos = starts0[t] + rng.integers(0, 200, size=n)
    for i in range(n):
        reads[i, : pre[i]] = codes0[pos[i]: pos[i] + pre[i]]
    flip = rng.random(n) < 0.5                                   # the other strand: poly-C heads, canonical form decides
    reads[flip] = (reads[flip][:, ::-1] ^ 2)
    codes = reads.reshape(-1)
    offs = (np.arange(n + 1, dtype=np.uint64) * L)
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    ohist, olinear = o.mark()
    words = synth.pack_2bit(codes)
    for rep in range(2):
        with pkg.PregraphGPU(K, est_distinct=1 << 18, flags=mode) as g:
            g.push_reads(words, offs)
            kmers, nodes = g.finish_count()
            assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
            hist, linear = g.mark_and_hist()
            assert linear == olinear and (hist == ohist).all()
            if rep == 0:
                assert node_dict_gpu(g) == node_dict_oracle(o)


def _rc_int(v, K):
    out = 0
    for _ in range(K):
        out = (out << 2) | ((v & 3) ^ 2)
        v >>= 2
    return out


def _first_link(links24):
    for b in range(4):
        if (links24 >> (6 * b)) & 63:
            return b
    return 4


def _deg(links24):
    return sum(1 for b in range(4) if (links24 >> (6 * b)) & 63)


def py_tip_walks(keys_int, l, rf, cnt, K, thin, cut_len):
    """the walk of clipTipFromNode (cutTipPreGraph.c:43-281), restated on Python ints: for every node, the index
    of the node the walk stops at (or None), ch, sm, thin_stop"""
    idx = {k: i for i, k in enumerate(keys_int)}
    mask = (1 << (2 * K)) - 1
    lin = [(int(x) >> 24) & 1 for x in rf]
    dele = [(int(x) >> 25) & 1 for x in rf]
    single = [int(c) == 1 for c in cnt]
    out = []
    for i, k in enumerate(keys_int):
        if lin[i] or dele[i] or (thin and not single[i]):
            out.append(None)
            continue
        ll, rl = int(l[i]) & 0xFFFFFF, int(rf[i]) & 0xFFFFFF
        if _deg(ll) == 0 and _deg(rl) == 1:
            at, b = k, _first_link(rl)
        elif _deg(ll) == 1 and _deg(rl) == 0:
            at, b = _rc_int(k, K), _first_link(ll) ^ 2
        else:
            out.append(None)
            continue
        steps, thin_stop, dead = 1, 0, False
        while True:
            step = ((at << 2) | b) & mask
            bal = _rc_int(step, K)
            sm = 0 if step > bal else 1
            o = idx[step if sm else bal]
            if not lin[o]:
                break
            steps += 1
            if thin and not single[o]:
                thin_stop = 1
                break
            if steps > cut_len:
                dead = True
                break
            at = step
            b = _first_link(int(rf[o]) & 0xFFFFFF) if sm else (_first_link(int(l[o]) & 0xFFFFFF) ^ 2)
        out.append(None if dead else (o, (at >> (2 * (K - 1))) & 3, sm, thin_stop))
    return out


@pytest.mark.parametrize("K,L", [(21, 100), (31, 100), (41, 150), (63, 150), (75, 200), (127, 250), (33, 120), (65, 200), (97, 250)])
def test_tip_walks_equal_reference_walk(pkg, synth, K, L):
    """the device dry run of removeSingleTips / removeMinorTips: every node's walk == the restated walk, on the
    table as counted and again after the host 'writes' nodes (update_nodes: deletions, cleared linear flags,
    dropped links on junctions) -- results indexed by an arbitrary host order"""
    tx = synth.make_transcriptome(20, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=3000, read_len=L, seed=K + 3, err=0.004, ragged=True)
    rng = np.random.default_rng(K)
    # the pinned C oracle holds the same graph (its tip_walk IS the first half of its clipTipFromNode, which the
    # reference's *.vertex goldens pin): the Python restatement below is a second opinion
    orc = ob.Oracle(K, nsets=3)
    orc.add_reads(codes, offs)
    orc.mark()
    with pkg.PregraphGPU(K, est_distinct=1 << 15) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        perm = rng.permutation(len(keys))
        keys, l, rf, cnt = keys[perm], l[perm].copy(), rf[perm].copy(), cnt[perm]
        ki = keys_to_int(keys)
        index_of = {k: i for i, k in enumerate(ki)}
        g.set_node_index(keys)
        for round_ in range(2):
            for thin in (0, 1):
                end, info = g.tip_walks(bool(thin), 2 * K)
                want = py_tip_walks(ki, l, rf, cnt, K, thin, 2 * K)
                for i in range(len(keys)):
                    w = orc.tip_walk(keys[i], 2 * K, thin)
                    if w is None:
                        assert end[i] == np.uint64(0xFFFFFFFFFFFFFFFF), (i, thin, "oracle: no walk")
                    else:
                        assert (int(end[i]), int(info[i])) == (index_of[w[0]], w[1]), (i, thin, "oracle walk")
                n_walks = 0
                for i, w in enumerate(want):
                    if w is None:
                        assert end[i] == np.uint64(0xFFFFFFFFFFFFFFFF), (i, thin)
                    else:
                        n_walks += 1
                        assert (int(end[i]), int(info[i])) == (w[0], w[1] | (w[2] << 2) | (w[3] << 3)), (i, thin, w)
                assert n_walks > 0 or thin
                # the compact form: the same walks, only for the nodes that have one
                rec = g.tip_walks_compact(bool(thin), 2 * K)
                got = {int(a) & ((1 << 56) - 1): (int(b), int(a) >> 56) for a, b in rec}
                assert got == {i: (w[0], w[1] | (w[2] << 2) | (w[3] << 3)) for i, w in enumerate(want) if w is not None}
            # short chains are cut off by cut_len
            end_short, _ = g.tip_walks(False, 3)
            want = py_tip_walks(ki, l, rf, cnt, K, 0, 3)
            assert [None if e == np.uint64(0xFFFFFFFFFFFFFFFF) else int(e) for e in end_short] == [None if w is None else w[0] for w in want]
            if round_ == 0:
                # the host writes: delete some nodes, un-linear some chain nodes, drop one link of some junctions
                pick = rng.choice(len(keys), size=len(keys) // 20, replace=False)
                rf[pick[: len(pick) // 3]] |= np.uint32(1 << 25)
                mid = pick[len(pick) // 3: 2 * len(pick) // 3]
                rf[mid] &= np.uint32(~(1 << 24) & 0xFFFFFFFF)
                for j in pick[2 * len(pick) // 3:]:
                    if not (int(rf[j]) >> 24) & 1:
                        b = _first_link(int(l[j]) & 0xFFFFFF)
                        if b < 4:
                            l[j] &= np.uint32(~(63 << (6 * b)) & 0xFFFFFFFF)
                g.update_nodes(keys[pick], l[pick], rf[pick])
                for j in pick:
                    orc.node_set(keys[j], int(l[j]) & 0xFFFFFF, int(rf[j]) & 0xFFFFFF, (int(rf[j]) >> 24) & 1, (int(rf[j]) >> 25) & 1)
        # the mirror now equals what we sent: export agrees (flags and links), counts untouched
        k2, l2, rf2, c2 = g.export_nodes()
        got = {k: (int(a), int(b) & 0x3FFFFFF, int(c)) for k, a, b, c in zip(keys_to_int(k2), l2, rf2, c2)}
        assert got == {k: (int(a), int(b) & 0x3FFFFFF, int(c)) for k, a, b, c in zip(ki, l, rf, cnt)}


def test_tip_walks_need_an_index(pkg, synth):
    tx = synth.make_transcriptome(3, seed=1)
    codes, offs = synth.sample_reads(*tx, n_reads=200, read_len=80, seed=2)
    with pkg.PregraphGPU(25, est_distinct=1 << 12) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g._nidx = 5
        with pytest.raises(pkg.SdtError):
            g.tip_walks(False, 50)
        keys, l, rf, cnt = g.export_nodes()
        bogus = keys.copy()
        bogus[0, -1] ^= np.uint64(1)                     # almost surely not a node
        if keys_to_int(bogus[:1])[0] not in set(keys_to_int(keys)):
            with pytest.raises(pkg.SdtError):
                g.set_node_index(bogus)


# ---- map stage: sdt_gpu_index_contigs / set_contig_table / align_reads vs oracle/sdt_oracle_map.c --------------
import map_util as mu  # noqa: E402


def _contig_table(num_all, lens, bals):
    """contig_array of basicContigInfo (prlRead2Ctg.c:610-648) -> (length[0..num], twin[0..num])"""
    length = np.zeros(num_all + 1, dtype=np.uint32)
    twin = np.zeros(num_all + 1, dtype=np.uint32)
    k = 0
    for ln, b in zip(lens, bals):
        k += 1
        length[k], twin[k] = ln, k + (int(b) + 1) - 1
        if b == 0:
            continue
        k += 1
        length[k], twin[k] = ln, k + (-int(b) + 1) - 1
    return length, twin


def _index_case(pkg, synth, info, g):
    K, ctgs, num_all, lens, bals = mu.case_contigs(info)
    offs = np.zeros(len(ctgs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c) for _, c in ctgs])
    codes = np.concatenate([c for _, c in ctgs])
    half = len(ctgs) // 2                                   # two calls: the contig ordinal carries over
    cut = int(offs[half])
    g.index_contigs(synth.pack_2bit(codes[:cut]), offs[: half + 1], [i for i, _ in ctgs[:half]])
    g.index_contigs(synth.pack_2bit(codes[cut:]), offs[half:] - offs[half], [i for i, _ in ctgs[half:]])
    g.set_contig_table(*_contig_table(num_all, lens, bals))
    return K


@pytest.mark.parametrize("name", mu.case_names())
def test_map_stage_equals_oracle(pkg, synth, name):
    """contig index counters and, for every read of the case, parse1read's result: hits in order (contig, offset,
    read offset, k-mers, strand), the best hit, the footprint flag -- for ALIGNLEN as the case's libraries set it and
    for a short one (more, smaller hits)"""
    info = mu.load_case(name)
    o = mu.build_oracle(info)
    K = o.K
    codes, offs, lib_of, libs, max_rd_len = mu.case_reads(info)
    with pkg.PregraphGPU(K, est_distinct=1 << 12, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:     # small table: grows while indexing
        assert _index_case(pkg, synth, info, g) == K
        kmers, nodes = g.finish_count()
        assert (nodes, kmers) == o.counts() == (info["nodes_allocated"], info["kmer_in_contigs"])
        words = synth.pack_2bit(codes)
        rng = np.random.default_rng(3)
        per_read = rng.integers(K, 80, size=len(offs) - 1).astype(np.int32)
        for mode in ("all", "per_read"):
            if mode == "all":
                info_w, hits = g.align_reads(words, offs, align_len_all=32)
                al = np.full(len(offs) - 1, 32, dtype=np.int32)
            else:
                info_w, hits = g.align_reads(words, offs, align_len=per_read)
                al = per_read
            mapped = 0
            for r in range(len(offs) - 1):
                n, want, best, foot = o.map_read(codes[int(offs[r]):int(offs[r + 1])], int(al[r]))
                w = int(info_w[r])
                start, nh, b, f, ov = w & ((1 << 40) - 1), (w >> 40) & 255, (w >> 48) & 255, (w >> 56) & 1, (w >> 57) & 1
                assert ov == 0 and n >= 0
                assert nh == n, (r, mode)
                if n == 0:
                    assert w == 0
                    continue
                mapped += 1
                got = [(int(h[0]), int(np.int32(h[1])), int(h[2]), int(h[3]) & 0x7FFFFFFF, "-" if int(h[3]) >> 31 else "+")
                       for h in [hits[r]] + list(hits[start:start + nh - 1])]       # hit 0 sits at hits[read], the rest in the tail
                assert got == want, (r, mode)
                assert (b, f) == (best, foot), (r, mode)
            assert mapped > 0


def test_map_stage_edge_cases(pkg, synth):
    """repeated k-mers across contigs are 'deleted' (never hit), reads shorter than K+1, more than 20 candidate
    contigs (undefined upstream: flagged), hit array too small -> SDT_EFULL with the needed size"""
    K = 21
    rng = np.random.default_rng(5)
    unit = rng.integers(0, 4, size=40).astype(np.uint8)
    ctgs = [rng.integers(0, 4, size=300).astype(np.uint8) for _ in range(30)]
    ctgs[3][100:140] = unit                       # the same 40 bases in two contigs: their 20 k-mers are deleted
    ctgs[7][10:50] = unit
    ids = np.arange(1, 31, dtype=np.uint32)
    o = mu.MapOracle(K, 4, 1)
    lens = np.full(30, 300, dtype=np.uint32)
    bals = np.zeros(30, dtype=np.int32)           # palindromic flag: every contig is its own twin
    o.set_contig_index(lens, bals, 30)
    for i, c in zip(ids, ctgs):
        o.add_contig(c, int(i))
    offs = np.arange(0, 31 * 300, 300, dtype=np.uint64)
    with pkg.PregraphGPU(K, est_distinct=1 << 14, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        g.index_contigs(synth.pack_2bit(np.concatenate(ctgs)), offs, ids)
        length = np.concatenate([[0], lens]).astype(np.uint32)
        g.set_contig_table(length, np.arange(31, dtype=np.uint32))
        kmers, nodes = g.finish_count()
        assert (nodes, kmers) == o.counts()
        reads = [unit.copy(),                                         # only deleted k-mers -> unmapped
                 ctgs[3][90:150].copy(),                              # flanks map, the repeat does not count
                 ctgs[5][:K].copy(),                                  # shorter than K+1
                 np.concatenate([c[50:50 + K + 4] for c in ctgs[8:30]]),   # 22 contigs x 5 k-mers: > 20 candidates
                 (ctgs[9][200:280][::-1] ^ 2).astype(np.uint8)]       # reverse strand
        roffs = np.zeros(len(reads) + 1, dtype=np.uint64)
        roffs[1:] = np.cumsum([len(r) for r in reads])
        rcodes = np.concatenate(reads)
        info_w, hits = g.align_reads(synth.pack_2bit(rcodes), roffs, align_len_all=K + 4)
        want = [o.map_read(r, K + 4) for r in reads]
        assert [w[0] for w in want] == [0, 1, 0, -1, 1]
        assert int(info_w[0]) == 0 and int(info_w[2]) == 0
        assert (int(info_w[3]) >> 57) & 1 == 1 and (int(info_w[3]) >> 40) & 255 == 0
        for r in (1, 4):
            w = int(info_w[r])
            assert (w >> 40) & 255 == 1
            h = hits[r]
            assert [(int(h[0]), int(np.int32(h[1])), int(h[2]), int(h[3]) & 0x7FFFFFFF, "-" if int(h[3]) >> 31 else "+")] == want[r][1]
        assert want[4][1][0][4] == "-"
        with pytest.raises(pkg.SdtError) as ei:
            g.align_reads(synth.pack_2bit(rcodes), roffs, align_len_all=K + 4, max_hits=1)
        assert ei.value.code == pkg.SDT_EINVAL            # fewer entries than reads
        two = np.concatenate([ctgs[1][:100], ctgs[2][:100]])                       # one read, two contigs -> needs a tail entry
        with pytest.raises(pkg.SdtError) as ei:
            g.align_reads(synth.pack_2bit(two), np.array([0, 200], dtype=np.uint64), align_len_all=K + 4, max_hits=1)
        assert ei.value.code == pkg.SDT_EFULL
        info2, hits2 = g.align_reads(synth.pack_2bit(two), np.array([0, 200], dtype=np.uint64), align_len_all=K + 4)
        assert (int(info2[0]) >> 40) & 255 == 2 and len(hits2) == 2 and [int(hits2[0][0]), int(hits2[1][0])] == [2, 3]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g2:             # not a contig-index context
        with pytest.raises(pkg.SdtError):
            g2.index_contigs(synth.pack_2bit(ctgs[0]), np.array([0, 300], dtype=np.uint64), ids[:1])


def test_bench_two_ranks_on_one_device_equal_one_rank(pkg, tmp_path):
    """the N>1 path of bench.py (C-level bucket sharding: sdt_gpu_count_reads_sharded, all-reduced kmerFreq / counters)
    run for real on the GPU: two ranks sharing cuda:0 (SDT_BENCH_SHARE_DEVICE=1: shared-memory transport, validation
    only) on slices of the single-rank workload must report the same node and linear-node counts as one rank"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--reads", "1000000", "--steps", "1", "--warmup", "1", "--cpu-sample", "0", "--T", "2000", "--extras", "0", "--slice-of-whole"]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    a = json.loads(one.stdout.strip().splitlines()[-1])
    env = dict(os.environ, SDT_BENCH_SHARE_DEVICE="1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29611", os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    b = json.loads(two.stdout.strip().splitlines()[-1])
    assert b["n_gpus"] == 2 and "sharded by minimizer bucket" in b["config"]["parallelism"]
    assert b["exchange"]["bytes_sent_all_ranks"] > 0 and b["exchange"]["exchanges_rank0"] >= 2
    assert b["roofline"] and b["roofline"]["rank"] == 0 and 0 < b["roofline"]["frac"] < 1     # rank 0's kernel, its own k-mers
    for k in ("kmers", "distinct_nodes", "linear_nodes"):
        assert a["config"][k] == b["config"][k], k


def test_bench_dump_outputs_hold_the_last_step(pkg, tmp_path):
    """bench.py --dump-outputs DIR: kmerfreq.npy holds the 257 bins the result line's kmerfreq_sha1 hashes, counts.npy its k-mer, node
    and linear-node counts (float64); a second run with the same arguments writes the same arrays; a plain run (no --full) leaves the
    legs that take runs of their own null"""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--reads", "1000000", "--T", "2000", "--steps", "2", "--warmup", "1"]
    got = []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common + ["--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads(r.stdout.strip().splitlines()[-1])
        hist, counts = np.load(d / "kmerfreq.npy"), np.load(d / "counts.npy")
        assert hist.dtype == np.float64 and hist.shape == (257,) and counts.dtype == np.float64
        assert hashlib.sha1(hist.astype(np.int64).tobytes()).hexdigest() == j["config"]["kmerfreq_sha1"]
        assert counts.tolist() == [j["config"]["kmers"], j["config"]["distinct_nodes"], j["config"]["linear_nodes"]]
        assert j["steps"] == 2 and j["ms_per_step"] > 0
        assert all(j[k] is None for k in ("track_first", "pcie_inclusive", "cpu_baseline", "e2e"))
        got.append((hist, counts))
    assert (got[0][0] == got[1][0]).all() and (got[0][1] == got[1][1]).all()


def py_minor_out_dry(keys_int, l, rf, cnt, K, threshold):
    """removeMinorOut's junction test (cutTipPreGraph.c:591-1010, 1012-1076) restated on Python ints:
    {junction index: [8 neighbour entries]} for the junctions that would cut, and the set of neighbours to cut"""
    idx = {k: i for i, k in enumerate(keys_int)}
    mask = (1 << (2 * K)) - 1
    NONE = (1 << 64) - 1

    def nbrs(i):
        k, out = keys_int[i], []
        for side in range(2):
            links = int(l[i]) & 0xFFFFFF if side == 0 else int(rf[i]) & 0xFFFFFF
            for b in range(4):
                if not (links >> (6 * b)) & 63:
                    out.append(NONE)
                    continue
                word = ((k >> 2) | (b << (2 * (K - 1)))) if side == 0 else (((k << 2) | b) & mask)
                bal = _rc_int(word, K)
                sm = 0 if word > bal else 1
                out.append((idx[word if sm else bal] << 1) | sm)
        return out

    junc, need = {}, set()
    for i in range(len(keys_int)):
        if (int(rf[i]) >> 24) & 3:                       # linear or deleted
            continue
        deg = [_deg(int(l[i]) & 0xFFFFFF), _deg(int(rf[i]) & 0xFFFFFF)]
        if deg[0] <= 1 and deg[1] <= 1:
            continue
        e = nbrs(i)
        hit = False
        for side in range(2):
            if deg[side] <= 1:
                continue
            cs = [int(cnt[v >> 1]) if v != NONE else None for v in e[side * 4: side * 4 + 4]]
            best = max([c for c in cs if c is not None] + [0])
            if not best:
                continue
            for v, c in zip(e[side * 4: side * 4 + 4], cs):
                if c and c / best < threshold:
                    need.add(v >> 1)
                    hit = True
        if hit:
            junc[i] = e
    return junc, need, nbrs


@pytest.mark.parametrize("K,L", [(21, 100), (31, 150), (47, 150), (75, 200), (33, 120), (65, 200), (97, 250)])
def test_minor_out_dry_run_equals_reference_rule(pkg, synth, K, L):
    """the device dry run of removeMinorOut: the set of junctions that would cut, the neighbours to cut, and the
    neighbour tables of both == the restated rule, on an arbitrary host order"""
    tx = synth.make_transcriptome(15, seed=K + 1)
    codes, offs = synth.sample_reads(*tx, n_reads=4000, read_len=L, seed=K + 5, err=0.006)
    rng = np.random.default_rng(K)
    orc = ob.Oracle(K, nsets=3)                       # the pinned C oracle on the same graph (clipKmerFromNode's own tests)
    orc.add_reads(codes, offs)
    orc.mark()
    NONE = (1 << 64) - 1
    with pkg.PregraphGPU(K, est_distinct=1 << 15) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        perm = rng.permutation(len(keys))
        keys, l, rf, cnt = keys[perm], l[perm], rf[perm], cnt[perm]
        ki = keys_to_int(keys)
        index_of = {k: i for i, k in enumerate(ki)}
        g.set_node_index(keys)
        for thr in (0.05, 0.3):
            rec, nj = g.minor_out_dry(thr)
            junc, need, nbrs = py_minor_out_dry(ki, l, rf, cnt, K, thr)
            got_j = {int(r[0]): [int(x) for x in r[1:]] for r in rec[:nj]}
            # C oracle: which nodes cut at all, whom, and every reported neighbour table
            o_junc, o_need = set(), set()
            for i in range(len(keys)):
                ncut, cut = orc.minor_out_probe(keys[i], thr)
                if ncut:
                    o_junc.add(i)
                    nb = orc.neighbours(keys[i])
                    o_need |= {index_of[nb[t][0]] for t in range(8) if cut[t]}
            assert set(got_j) == o_junc
            assert {int(r[0]) for r in rec[nj:]} == o_need - o_junc
            for r in rec:
                nb = orc.neighbours(keys[int(r[0])])
                assert [int(x) for x in r[1:]] == [NONE if e is None else (index_of[e[0]] << 1) | e[1] for e in nb]
            assert got_j == junc and len(junc) > 0
            got_c = {int(r[0]): [int(x) for x in r[1:]] for r in rec[nj:]}
            assert set(got_c) == need - set(junc)
            for i, e in got_c.items():
                assert e == nbrs(i)


def py_edge_ports(keys_int, l, rf, K):
    """stringBeads + check_iden_kmerList (node2edge.c:58-191, 563-588) restated: {node: [(far, far_port, length, bal) or None] * 8}"""
    idx = {k: i for i, k in enumerate(keys_int)}
    mask = (1 << (2 * K)) - 1
    lin = [(int(x) >> 24) & 1 for x in rf]
    dele = [(int(x) >> 25) & 1 for x in rf]
    out = {}
    for i, k in enumerate(keys_int):
        if lin[i] or dele[i]:
            continue
        ports = []
        for p in range(8):
            links = int(rf[i]) & 0xFFFFFF if p < 4 else int(l[i]) & 0xFFFFFF
            if not (links >> (6 * (p & 3))) & 63:
                ports.append(None)
                continue
            word = k if p < 4 else _rc_int(k, K)
            b = p if p < 4 else (p - 4) ^ 2
            chain = [word]
            while True:
                word = ((word << 2) | b) & mask
                bal = _rc_int(word, K)
                sm = 0 if word > bal else 1
                o = idx[word if sm else bal]
                chain.append(word)
                if not lin[o]:
                    break
                b = _first_link(int(rf[o]) & 0xFFFFFF) if sm else (_first_link(int(l[o]) & 0xFFFFFF) ^ 2)
            fc = (chain[-2] >> (2 * (K - 1))) & 3
            palin = all(chain[len(chain) - 1 - j] == _rc_int(chain[j], K) for j in range(len(chain)))
            ports.append((o, 4 + fc if sm else fc ^ 2, len(chain) - 1, 0 if palin else 1))
        out[i] = ports
    return out


@pytest.mark.parametrize("K,L", [(21, 100), (31, 120), (47, 150), (75, 200), (33, 120), (65, 200), (97, 250)])
def test_edge_port_walks_equal_reference_rule(pkg, synth, K, L):
    """the device dry run of kmer2edges: every port of every non-linear node -- far node, arrival port, length and
    the palindrome flag (decided from 4 k-mers on the device, from the whole list here); reads that spell X + rc(X)
    put self-complementary chains into the graph"""
    tx = synth.make_transcriptome(12, seed=K + 2)
    codes, offs = synth.sample_reads(*tx, n_reads=2500, read_len=L, seed=K + 7, err=0.004)
    rng = np.random.default_rng(K)
    extra = []
    for j in range(6):                                    # hairpins: X + rc(X), several copies each
        x = tx[0][200 * j + 17: 200 * j + 17 + L // 2]
        hp = np.concatenate([x, (x[::-1] ^ 2)]).astype(np.uint8)
        extra += [hp] * 5
    codes = np.concatenate([codes] + extra)
    offs = np.concatenate([offs, offs[-1] + np.cumsum([len(e) for e in extra]).astype(np.uint64)])
    # the C oracle holds the same graph (its walk restates startEdgeFromNode / stringBeads / check_iden_kmerList from the
    # reference's sources); the Python restatement above is a second opinion
    orc = ob.Oracle(K, nsets=3)
    orc.add_reads(codes, offs)
    orc.mark()
    with pkg.PregraphGPU(K, est_distinct=1 << 15) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        perm = rng.permutation(len(keys))
        keys, l, rf = keys[perm], l[perm], rf[perm]
        ki = keys_to_int(keys)
        g.set_node_index(keys)
        rec = g.edge_ports()
        want = py_edge_ports(ki, l, rf, K)
        assert len(rec) == len(want) > 0
        for i, ports in want.items():                         # restatement in C == restatement in Python
            for p in range(8):
                c = orc.edge_port(keys[i], p)
                assert c != -1
                assert c == (None if ports[p] is None else (ki[ports[p][0]],) + tuple(ports[p][1:])), (i, p)
        for i in range(len(keys)):                            # linear / deleted nodes start no edge
            if i not in want:
                assert orc.edge_port(keys[i], 0) == -1
        NONE = (1 << 64) - 1
        palins = 0
        for r in rec:
            i = int(r[0])
            got = []
            for p in range(8):
                far, meta = int(r[1 + 2 * p]), int(r[2 + 2 * p])
                got.append(None if far == NONE else (far, (meta >> 32) & 255, meta & 0xFFFFFFFF, (meta >> 40) & 1))
            assert got == want[i], i
            palins += sum(1 for x in got if x is not None and x[3] == 0)
        assert palins > 0


@pytest.mark.parametrize("K,L", [(21, 90), (45, 160), (81, 300), (33, 120), (65, 200), (97, 250)])
def test_map_stage_randomised_vs_oracle(pkg, synth, K, L):
    """random contigs that share stretches (repeated k-mers = 'deleted'), reads that hop between contigs and
    strands, reads shorter than K+1, lengths that need several 64-k-mer rounds per wavefront; 1-, 2- and 4-word keys"""
    rng = np.random.default_rng(K * 7 + L)
    nctg = 40
    ctgs = [rng.integers(0, 4, size=int(rng.integers(K + 2, 900))).astype(np.uint8) for _ in range(nctg)]
    for _ in range(12):                                   # shared stretches between random contig pairs
        a, b = rng.integers(0, nctg, size=2)
        n = int(rng.integers(K, 2 * K))
        if len(ctgs[a]) > n + 2 and len(ctgs[b]) > n + 2:
            pa, pb = int(rng.integers(0, len(ctgs[a]) - n)), int(rng.integers(0, len(ctgs[b]) - n))
            ctgs[b][pb:pb + n] = ctgs[a][pa:pa + n]
    ids = np.arange(1, 2 * nctg, 2, dtype=np.uint32)      # odd ids, twin = id + 1
    lens = np.array([len(c) for c in ctgs], dtype=np.uint32)
    o = mu.MapOracle(K, 5, 1 if K <= 31 else (2 if K <= 63 else 4))
    o.set_contig_index(lens, np.ones(nctg, dtype=np.int32), 2 * nctg)
    for i, c in zip(ids, ctgs):
        o.add_contig(c, int(i))
    length = np.zeros(2 * nctg + 1, dtype=np.uint32)
    twin = np.zeros(2 * nctg + 1, dtype=np.uint32)
    length[1::2], length[2::2] = lens, lens
    twin[1::2], twin[2::2] = ids + 1, ids
    reads = []
    for _ in range(600):
        parts, want = [], int(rng.integers(10, L + 1))
        while sum(len(p) for p in parts) < want:           # 1..3 pieces from random contigs / strands
            c = ctgs[int(rng.integers(0, nctg))]
            n = int(rng.integers(5, min(len(c), want) + 1))
            p0 = int(rng.integers(0, len(c) - n + 1))
            piece = c[p0:p0 + n]
            if rng.random() < 0.5:
                piece = (piece[::-1] ^ 2).astype(np.uint8)
            parts.append(piece)
        r = np.concatenate(parts)[:want].copy()
        flips = rng.random(len(r)) < 0.01
        r[flips] = (r[flips] + 1) & 3
        reads.append(r)
    # reads across a junction: the end of one contig, then the start of another on either strand, L / 2 bases (more than K) of each.
    # The pieces above are too short to give a read two hits once K nears L / 2 (none of the 600 has two at K = 97, L = 250).  A
    # generator of their own, so that the 600 reads above and their align_len are what they were before these were added
    rng2 = np.random.default_rng(K * 11 + L)
    for _ in range(40):
        a, b = rng2.choice(nctg, size=2, replace=False)
        tail, head = ctgs[a][-(L // 2):], ctgs[b][:L - L // 2]
        if rng2.random() < 0.5:
            head = (head[::-1] ^ 2).astype(np.uint8)
        reads.append(np.concatenate([tail, head]))
    roffs = np.zeros(len(reads) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in reads])
    rcodes = np.concatenate(reads)
    offs = np.zeros(nctg + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    with pkg.PregraphGPU(K, est_distinct=1 << 13, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        g.index_contigs(synth.pack_2bit(np.concatenate(ctgs)), offs, ids)
        g.set_contig_table(length, twin)
        kmers, nodes = g.finish_count()
        assert (nodes, kmers) == o.counts()
        al = np.concatenate([rng.integers(K, K + 40, size=600), rng2.integers(K, K + 40, size=40)]).astype(np.int32)
        info_w, hits = g.align_reads(synth.pack_2bit(rcodes), roffs, align_len=al)
        multi = 0
        for r in range(len(reads)):
            n, want, best, foot = o.map_read(reads[r], int(al[r]))
            w = int(info_w[r])
            start, nh, b, f = w & ((1 << 40) - 1), (w >> 40) & 255, (w >> 48) & 255, (w >> 56) & 1
            assert n >= 0 and nh == n, r
            if not n:
                assert w == 0
                continue
            got = [(int(h[0]), int(np.int32(h[1])), int(h[2]), int(h[3]) & 0x7FFFFFFF, "-" if int(h[3]) >> 31 else "+")
                   for h in [hits[r]] + list(hits[start:start + nh - 1])]
            assert got == want and (b, f) == (best, foot), r
            multi += n > 1
        assert multi > 0


def test_kernel_rate_floors(pkg, synth):
    """not a benchmark -- a guard against order-of-magnitude regressions (a shared atomic cursor once cost the look-up
    kernel 5x without changing any result): pass-1 counting >= 8 G k-mers/s (measured 19.6 direct, ~40 through the
    locality pipeline at this size), contig look-ups >= 15 G k-mers/s (measured 50), on a workload generated in HBM.
    On a shared or down-clocked GPU a rate can dip: a miss is a WARNING unless SDT_STRICT_RATES=1 (the results above
    are still asserted)."""
    import ctypes
    import os
    import warnings

    def floor(rate, limit, what):
        if rate > limit:
            return
        msg = f"{what}: {rate / 1e9:.1f} G k-mers/s is below the floor of {limit / 1e9:.0f}"
        if os.environ.get("SDT_STRICT_RATES") == "1":
            raise AssertionError(msg)
        warnings.warn(msg)

    import torch
    dev = torch.device("cuda:0")
    K, L, n, T = 31, 150, 4_000_000, 2000
    words, offsets, nwords = synth.torch_workload(n, L, T, dev)
    torch.cuda.synchronize()
    kmers = n * (L - K + 1)
    with pkg.PregraphGPU(K, est_distinct=1 << 26) as g:
        for _ in range(2):
            g.reset()
            g.kernel_time(reset=True)
            g.count_reads_device(words, nwords, offsets, n, L)
            got, _ = g.finish_count()
            ms, _, _ = g.kernel_time(reset=True)
        assert got == kmers
        floor(kmers / (ms * 1e-3), 8e9, "pass 1")
    codes, starts, _ = synth.make_transcriptome(T, seed=42)
    ids = np.arange(1, 2 * T, 2, dtype=np.uint32)
    lens = (starts[1:] - starts[:-1]).astype(np.uint32)
    length = np.zeros(2 * T + 1, dtype=np.uint32)
    twin = np.zeros(2 * T + 1, dtype=np.uint32)
    length[1::2], length[2::2] = lens, lens
    twin[1::2], twin[2::2] = ids + 1, ids
    with pkg.PregraphGPU(K, est_distinct=int(starts[-1]) + 1024, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        g.index_contigs(synth.pack_2bit(codes), starts.astype(np.uint64), ids)
        g.finish_count()
        g.set_contig_table(length, twin)
        info = torch.zeros(n, dtype=torch.int64, device=dev)
        cap = n + n // 4
        hits = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        nh = ctypes.c_uint64()
        for _ in range(2):
            g.kernel_time(reset=True)
            rc = g.lib.sdt_gpu_align_reads_device(g._ctx, words.data_ptr(), offsets.data_ptr(), n, L, None, 32, info.data_ptr(),
                                                  hits.data_ptr(), cap, ctypes.byref(nh))
            assert rc == 0, g.lib.sdt_gpu_last_error().decode()
            ms, _, _ = g.kernel_time(reset=True)
        mapped = int((((info >> 40) & 255) > 0).sum().item())
        assert mapped > 0.99 * n
        floor(kmers / (ms * 1e-3), 15e9, "k_align_reads")


# ---- round 4: the visiting order on the device, labelled dry runs ----------------------------------------------------
def _uf_labels(n, edges):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


@pytest.mark.parametrize("K,L,variant,p", [(23, 100, 1, 8), (31, 150, 1, 3), (31, 150, 2, 16), (47, 150, 2, 5), (75, 200, 4, 8), (25, 100, 4, 1),
                                           (33, 120, 2, 4), (65, 200, 4, 3), (97, 250, 4, 5)])
def test_layout_on_device_sorts_by_set_and_first_occurrence(pkg, synth, K, L, variant, p):
    """sdt_gpu_layout_sorted_keys: the nodes grouped by hash_kmer % p (the oracle's pinned restatement of hashFunction.c:83-122,
    over the bytes of the emulated variant's Kmer) and ordered by first occurrence inside a set; layout_apply + export_ordered:
    the nodes come back in whatever order the host asks for, and the dry runs are indexed by it"""
    tx = synth.make_transcriptome(10, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=2500, read_len=L, seed=K + 1, err=0.004, ragged=True)
    rng = np.random.default_rng(K + p)
    with pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt, first = g.export_nodes(with_first=True)
        nwk = keys.shape[1]
        wide = np.zeros((len(keys), 4), dtype=np.uint64)
        wide[:, 4 - nwk:] = keys
        OL = ob.lib()
        sets = np.array([OL.sdto_hash_kmer(ob.Kmer.of(wide[i]), variant) % p for i in range(len(keys))])
        want = np.lexsort((first, sets))
        skeys, ss = g.layout_sorted_keys(p, variant)
        assert (skeys == keys[want]).all()
        assert [int(x) for x in ss] == [int((sets < s).sum()) for s in range(p + 1)]
        order = rng.permutation(len(keys)).astype(np.uint64)
        g.layout_apply(order)
        k2, l2, r2, c2 = g.export_ordered()
        src = want[order]
        assert (k2 == keys[src]).all() and (l2 == l[src]).all() and (c2 == cnt[src]).all()
        assert ((r2 & 0x3FFFFFF) == (rf[src] & 0x3FFFFFF)).all()
        # the node numbering is what every dry run speaks: same walks as with set_node_index on the same order
        end_a, info_a = g.tip_walks(False, 2 * K)
        g.set_node_index(k2)
        end_b, info_b = g.tip_walks(False, 2 * K)
        assert (end_a == end_b).all() and (info_a == info_b).all()
        # writes by node index reach the same nodes as writes by key
        g.layout_sorted_keys(p, variant)
        g.layout_apply(order)
        pick = rng.choice(len(keys), size=max(1, len(keys) // 10), replace=False)
        l3, r3 = l2.copy(), r2.copy()
        r3[pick] |= np.uint32(1 << 25)
        l3[pick] &= np.uint32(0xFFFFC0)
        g.update_nodes_by_index(pick.astype(np.uint64), l3[pick], r3[pick])
        k4, l4, r4, c4 = g.export_ordered()
        assert (k4 == k2).all() and (l4 == l3).all() and ((r4 & 0x3FFFFFF) == (r3 & 0x3FFFFFF)).all() and (c4 == c2).all()


@pytest.mark.parametrize("K,L", [(21, 100), (31, 150), (63, 150), (75, 200), (33, 120), (65, 200), (97, 250)])
def test_labelled_walks_and_their_components(pkg, synth, K, L):
    """sdt_gpu_tip_walks_labelled: the walks of tip_walks_compact, each with the component of its node -- removeSingleTips: the
    connected components of (tip, end node); removeMinorTips: of the non-linear nodes joined by chains of <= cut_len linear
    nodes (taken here from the port walks of py_edge_ports) -- and sorted by (label, node)"""
    tx = synth.make_transcriptome(6, seed=K + 11)
    codes, offs = synth.sample_reads(*tx, n_reads=4000, read_len=L, seed=K + 12, err=0.01)
    rng = np.random.default_rng(K)
    with pkg.PregraphGPU(K, est_distinct=1 << 15) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        perm = rng.permutation(len(keys))
        keys, l, rf, cnt = keys[perm], l[perm], rf[perm], cnt[perm]
        ki = keys_to_int(keys)
        g.set_node_index(keys)
        M56 = (1 << 56) - 1
        for thin, cut_len in ((1, 2 * K), (0, 2 * K), (0, 5)):
            plain = g.tip_walks_compact(bool(thin), cut_len)
            rec = g.tip_walks_labelled(bool(thin), cut_len)
            assert sorted((int(a), int(b)) for a, b in plain) == sorted((int(a), int(b)) for a, b, _ in rec)
            assert len(rec) > 0
            nodes = [int(a) & M56 for a, _, _ in rec]
            labs = [int(c) for _, _, c in rec]
            assert list(zip(labs, nodes)) == sorted(zip(labs, nodes)), "sorted by (label, node)"
            if thin:
                edges = [(int(a) & M56, int(b)) for a, b, _ in rec]
            else:
                ports = py_edge_ports(ki, l, rf, K)
                edges = [(i, pt[0]) for i, pp in ports.items() for pt in pp if pt is not None and pt[2] - 1 <= cut_len]
            want = _uf_labels(len(keys), edges)
            assert labs == [want[i] for i in nodes]
            if not thin and cut_len > 5:
                assert len(set(labs)) < len(labs), "some component holds more than one walk"


@pytest.mark.parametrize("K,L", [(21, 100), (31, 150), (47, 150), (33, 120), (65, 200), (97, 250)])
def test_labelled_junction_records_and_their_components(pkg, synth, K, L):
    """sdt_gpu_minor_out_labelled: the records of minor_out_dry with the component of their node (every record's node united
    with its eight neighbours), the junction records sorted by (label, node)"""
    tx = synth.make_transcriptome(8, seed=K + 21)
    codes, offs = synth.sample_reads(*tx, n_reads=4000, read_len=L, seed=K + 22, err=0.008)
    rng = np.random.default_rng(K)
    NONE = (1 << 64) - 1
    with pkg.PregraphGPU(K, est_distinct=1 << 15) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        keys, l, rf, cnt = g.export_nodes()
        perm = rng.permutation(len(keys))
        keys, cnt = keys[perm], cnt[perm]
        g.set_node_index(keys)
        for thr in (0.05, 0.3):
            plain, nj0 = g.minor_out_dry(thr)
            rec, nj = g.minor_out_labelled(thr)
            assert nj == nj0 > 0 and len(rec) == len(plain)
            assert sorted(tuple(int(x) for x in r) for r in plain[:nj0]) == sorted(tuple(int(x) for x in r[:9]) for r in rec[:nj])
            assert sorted(tuple(int(x) for x in r) for r in plain[nj0:]) == sorted(tuple(int(x) for x in r[:9]) for r in rec[nj:])
            for r in rec:                                     # the counts of the neighbours ride along
                for q in range(8):
                    c = (int(r[9 + q // 2]) >> (32 * (q & 1))) & 0xFFFFFFFF
                    assert c == (0 if int(r[1 + q]) == NONE else int(cnt[int(r[1 + q]) >> 1]))
            edges = [(int(r[0]), int(x) >> 1) for r in rec for x in r[1:9] if int(x) != NONE]
            want = _uf_labels(len(keys), edges)
            labs = [int(r[13]) for r in rec[:nj]]
            nodes = [int(r[0]) for r in rec[:nj]]
            assert labs == [want[i] for i in nodes]
            assert list(zip(labs, nodes)) == sorted(zip(labs, nodes))


def py_minor_out_commit(rec, nj, keys_int, l, rf, K, thr):
    """removeMinorOut's commit (cutTipPreGraph.c:591-1010; csrc/host/graph/cuttip.c: visit_minor_out / prune_side / isolate) over
    the junction records in node order -- the reference's sweep -- plus the re-marking of the nodes it wrote:
    (l, r, linear, deleted, kmers off, newly linear, written nodes)"""
    ll = [int(x) & 0xFFFFFF for x in l]
    rr = [int(x) & 0xFFFFFF for x in rf]
    lin = [(int(x) >> 24) & 1 for x in rf]
    dele = [(int(x) >> 25) & 1 for x in rf]
    recof = {int(R[0]): R for R in rec}
    deg = lambda v: sum(1 for b in range(4) if (v >> (6 * b)) & 63)
    cnt_of = lambda R, q: (int(R[9 + q // 2]) >> (32 * (q & 1))) & 0xFFFFFFFF
    touched, off = set(), 0

    def isolate(q):
        dele[q] = 1
        touched.add(q)
        Q, kq = recof[q], keys_int[q]
        ch_last, ch_first = kq & 3, (kq >> (2 * (K - 1))) & 3
        for side in (0, 1):
            for b in range(4):
                if not ((ll[q] if side == 0 else rr[q]) >> (6 * b)) & 63:
                    continue
                nb = int(Q[1 + side * 4 + b])
                x, sm = nb >> 1, nb & 1
                if side == 0:                                 # unlink_next(x, last base of q, sm)
                    right, base = (1, ch_last) if sm else (0, ch_last ^ 2)
                else:                                         # unlink_prev(y, first base of q, sm)
                    right, base = (0, ch_first) if sm else (1, ch_first ^ 2)
                if right:
                    rr[x] &= ~(63 << (6 * base))
                else:
                    ll[x] &= ~(63 << (6 * base))
                lin[x] = 1 if deg(ll[x]) == 1 and deg(rr[x]) == 1 else 0
                touched.add(x)

    for R in sorted(rec[:nj], key=lambda R: int(R[0])):
        n = int(R[0])
        if lin[n] or dele[n]:
            continue
        i, o = deg(ll[n]), deg(rr[n])
        if i <= 1 and o <= 1:
            continue
        for side, d in ((0, i), (1, o)):
            if d <= 1:
                continue
            links = ll[n] if side == 0 else rr[n]
            best = max([cnt_of(R, side * 4 + b) for b in range(4) if (links >> (6 * b)) & 63] + [0])
            if not best:
                continue
            for b in range(4):
                if not ((ll[n] if side == 0 else rr[n]) >> (6 * b)) & 63:
                    continue
                c = cnt_of(R, side * 4 + b)
                if c and c / best < thr:
                    off += 1
                    isolate(int(R[1 + side * 4 + b]) >> 1)
    marked = 0
    for i in touched:
        if not dele[i] and not lin[i] and deg(ll[i]) == 1 and deg(rr[i]) == 1:
            lin[i] = 1
            marked += 1
    return ll, rr, lin, dele, off, marked, touched


@pytest.mark.parametrize("K,L,thr", [(21, 100, 0.05), (31, 150, 0.3), (31, 150, 0.05), (47, 150, 0.3), (75, 200, 0.2),
                                     (33, 120, 0.3), (65, 200, 0.2), (97, 250, 0.2)])
def test_minor_out_commit_on_the_device_equals_the_sequential_commit(pkg, synth, K, L, thr):
    """sdt_gpu_minor_out_commit (one lane per component, the visits of a component in record order) against the sequential sweep over
    the junctions in node order: kmers off, newly linear nodes, the set of written nodes, and every node's links and flags afterwards"""
    tx = synth.make_transcriptome(8, seed=K + 31)
    codes, offs = synth.sample_reads(*tx, n_reads=5000, read_len=L, seed=K + 32, err=0.01)
    variant = 1 if K <= 31 else (2 if K <= 63 else 4)
    with pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        g.layout_on_device(4, variant)
        keys, l, rf, cnt = g.export_ordered()
        ki = keys_to_int(keys)
        # a component limit of zero: every component is left to the caller -- nothing written, all junction records handed over in order
        small = g.minor_out_commit(thr, max_component=0)
        assert small["largest"] >= 1 and small["off"] == 0 and len(small["node"]) == 0
        assert (small["skipped"] == small["records"][:small["n_junctions"]]).all()
        assert (small["skipped_neighbours"] == small["records"][small["n_junctions"]:]).all()
        k1, l1, r1, c1 = g.export_ordered()
        assert (l1 == l).all() and (r1 == rf).all()
        res = g.minor_out_commit(thr)
        rec, nj = res["records"], res["n_junctions"]
        assert nj > 0 and res["largest"] == small["largest"] and len(res["skipped"]) == 0
        ll, rr, lin, dele, off, marked, touched = py_minor_out_commit(rec, nj, ki, l, rf, K, thr)
        assert off > 0 and res["off"] == off and res["linear"] == marked
        assert sorted(int(x) for x in res["node"]) == sorted(touched)
        for i, a, b in zip(res["node"], res["l_links"], res["r_flags"]):
            i = int(i)
            assert int(a) == ll[i] and int(b) & 0xFFFFFF == rr[i] and (int(b) >> 24) & 1 == lin[i] and (int(b) >> 25) & 1 == dele[i]
        k2, l2, r2, c2 = g.export_ordered()
        assert (k2 == keys).all() and (c2 == cnt).all()
        assert [int(x) & 0xFFFFFF for x in l2] == ll and [int(x) & 0xFFFFFF for x in r2] == rr
        assert [(int(x) >> 24) & 1 for x in r2] == lin and [(int(x) >> 25) & 1 for x in r2] == dele


@pytest.mark.parametrize("K,L,thr", [(31, 150, 0.3), (47, 150, 0.2)])
def test_minor_out_commit_split_between_the_device_and_the_caller(pkg, synth, K, L, thr):
    """components above the limit are left alone and their records handed over: the device's half + the sequential commit of the
    handed-over records (they touch no node the device wrote) = the whole sequential commit"""
    tx = synth.make_transcriptome(8, seed=K + 41)
    codes, offs = synth.sample_reads(*tx, n_reads=5000, read_len=L, seed=K + 42, err=0.012)
    variant = 1 if K <= 31 else 2
    with pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        g.layout_on_device(4, variant)
        keys, l, rf, cnt = g.export_ordered()
        ki = keys_to_int(keys)
        res = g.minor_out_commit(thr, max_component=2)
        rec, nj, sk = res["records"], res["n_junctions"], res["skipped"]
        assert res["largest"] > 2 and 0 < len(sk) < nj, "the input must have components on both sides of the limit"
        labs = [int(R[13]) for R in rec[:nj]]
        big = {lab for lab in set(labs) if labs.count(lab) > 2}
        assert [tuple(int(x) for x in R) for R in sk] == [tuple(int(x) for x in R) for R in rec[:nj] if int(R[13]) in big]
        assert [tuple(int(x) for x in R) for R in res["skipped_neighbours"]] == [tuple(int(x) for x in R) for R in rec[nj:] if int(R[13]) in big]
        # the whole commit, sequentially
        ll, rr, lin, dele, off, marked, touched = py_minor_out_commit(rec, nj, ki, l, rf, K, thr)
        # the device's half ...
        small_rec = np.array([R for R in rec[:nj] if int(R[13]) not in big] + [R for R in rec[nj:]], dtype=np.uint64).reshape(-1, 14)
        n_small = sum(1 for R in rec[:nj] if int(R[13]) not in big)
        l_a, r_a, lin_a, del_a, off_a, marked_a, touched_a = py_minor_out_commit(small_rec, n_small, ki, l, rf, K, thr)
        assert res["off"] == off_a and res["linear"] == marked_a and sorted(int(x) for x in res["node"]) == sorted(touched_a)
        # ... and the caller's on top of it give the whole
        rf_mid = np.array([r_a[i] | (lin_a[i] << 24) | (del_a[i] << 25) for i in range(len(ki))], dtype=np.uint32)
        big_rec = np.array([R for R in sk] + [R for R in rec[nj:]], dtype=np.uint64).reshape(-1, 14)
        l_b, r_b, lin_b, del_b, off_b, marked_b, touched_b = py_minor_out_commit(big_rec, len(sk), ki, np.array(l_a, dtype=np.uint32), rf_mid, K, thr)
        assert not (touched_a & touched_b)
        assert off_a + off_b == off and marked_a + marked_b == marked
        assert l_b == ll and r_b == rr and lin_b == lin and del_b == dele


def py_build_edges(keys_int, l, rf, cnt, K):
    """kmer2edges (node2edge.c:46-561) restated sequentially over the nodes in index order: [(length, bal_edge, cvg, id, from, to,
    bases)], num_ed, {node: path word} -- interior nodes are stamped last to first and the coverage sum reads what is there"""
    idx = {k: i for i, k in enumerate(keys_int)}
    mask = (1 << (2 * K)) - 1
    lin = [(int(x) >> 24) & 1 for x in rf]
    dele = [(int(x) >> 25) & 1 for x in rf]
    ll = [int(x) & 0xFFFFFF for x in l]                  # l_links as the stamping leaves them
    zeroed = [0] * len(keys_int)
    edges, num_ed, stamp = [], 0, {}
    for i, k in enumerate(keys_int):
        if lin[i] or dele[i]:
            continue
        for p in range(8):
            links = int(rf[i]) & 0xFFFFFF if p < 4 else int(l[i]) & 0xFFFFFF
            if not (links >> (6 * (p & 3))) & 63 or (zeroed[i] >> p) & 1:
                continue
            word = k if p < 4 else _rc_int(k, K)
            b = p if p < 4 else (p - 4) ^ 2
            chain, nodes, sms = [word], [i], [1 if p < 4 else 0]
            while True:
                word = ((word << 2) | b) & mask
                bal = _rc_int(word, K)
                sm = 0 if word > bal else 1
                o = idx[word if sm else bal]
                chain.append(word); nodes.append(o); sms.append(sm)
                if not lin[o]:
                    break
                b = _first_link(int(rf[o]) & 0xFFFFFF) if sm else (_first_link(int(l[o]) & 0xFFFFFF) ^ 2)
            n = len(chain)
            fc = (chain[-2] >> (2 * (K - 1))) & 3
            far_port = 4 + fc if sms[-1] else fc ^ 2
            bal_edge = 0 if all(chain[n - 1 - j] == _rc_int(chain[j], K) for j in range(n)) else 1
            zeroed[i] |= 1 << p
            zeroed[nodes[-1]] |= 1 << far_port
            num_ed += 1
            eid = num_ed
            num_ed += bal_edge
            length = n - 1
            symbol = int(cnt[i]) if length == 1 else 0
            for j in range(n - 2, 0, -1):
                o = nodes[j]
                v = ll[o]
                symbol += (v & 63) + ((v >> 6) & 63) + ((v >> 12) & 63) + ((v >> 18) & 63)
                ll[o] = (eid if sms[j] else eid + bal_edge) & 0xFFFFFFFF
                stamp[o] = 2 | ((bal_edge + 1 if sms[j] else 1 - bal_edge) << 2) | ((eid if sms[j] else eid + bal_edge) << 32)
            cvg = (symbol // (length - 1) * 10) if length > 1 else (symbol // length * 10)
            edges.append((length, bal_edge, min(cvg, 16000), eid, chain[0], chain[-1], "".join("ACTG"[w & 3] for w in chain[1:])))
    return edges, num_ed, stamp


@pytest.mark.parametrize("K,L,p", [(21, 100, 8), (31, 120, 3), (47, 150, 16), (75, 200, 5), (33, 120, 4), (65, 200, 3), (97, 250, 5)])
def test_edges_built_on_the_device_equal_the_sequential_rule(pkg, synth, K, L, p):
    """sdt_gpu_build_edges: edge records in id order (length, bal_edge, cvg with the palindrome quirk, id, end k-mers), the bases
    of every edge and the number of ids == kmer2edges restated sequentially over the nodes in the order the host asked for;
    hairpin reads (X + rc(X)) put self-complementary chains into the graph"""
    tx = synth.make_transcriptome(12, seed=K + 2)
    codes, offs = synth.sample_reads(*tx, n_reads=2500, read_len=L, seed=K + 7, err=0.004)
    rng = np.random.default_rng(K)
    extra = []
    for j in range(6):
        x = tx[0][200 * j + 17: 200 * j + 17 + L // 2]
        hp = np.concatenate([x, (x[::-1] ^ 2)]).astype(np.uint8)
        extra += [hp] * 5
    codes = np.concatenate([codes] + extra)
    offs = np.concatenate([offs, offs[-1] + np.cumsum([len(e) for e in extra]).astype(np.uint64)])
    with pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        skeys, _ = g.layout_sorted_keys(p, 4 if K > 63 else (2 if K > 31 else 1))
        g.layout_apply(rng.permutation(len(skeys)).astype(np.uint64))
        keys, l, rf, cnt = g.export_ordered()
        ki = keys_to_int(keys)
        want, want_ids, _ = py_build_edges(ki, l, rf, cnt, K)
        rec, bases, num_ed = g.build_edges()
        nw = keys.shape[1]
        assert num_ed == want_ids and len(rec) == len(want) > 0
        palins = 0
        for r, w in zip(rec, want):
            length, bal = int(r[0]) & 0xFFFFFFFF, (int(r[0]) >> 32) & 1
            frm = keys_to_int(r[4:4 + nw].reshape(1, nw))[0]
            to = keys_to_int(r[4 + nw:4 + 2 * nw].reshape(1, nw))[0]
            got = (length, bal, int(r[1]), int(r[2]), frm, to, bases[int(r[3]):int(r[3]) + length].decode())
            assert got == w
            palins += bal == 0
        assert palins > 0, "the hairpin reads made no self-complementary chain"


@pytest.mark.parametrize("mode", MODES)
def test_read_ordinals_continue_from_device_batches_into_pushed_ones(pkg, synth, mode):
    """a batch counted from device memory followed by a pushed batch with no finish_count in between: the pushed reads continue
    the ordinals of the stream (first-occurrence order == one stream through the oracle)"""
    import torch
    K, L, n = 31, 100, 6000
    tx = synth.make_transcriptome(20, seed=5)
    codes, offs = synth.sample_reads(*tx, n_reads=n, read_len=L, seed=6, err=0.004)
    words = synth.pack_2bit(codes)
    half = n // 2
    w1 = np.ascontiguousarray(words[: half * L // 16 + 8])
    o = ob.Oracle(K, nsets=4)
    o.add_reads(codes, offs)
    d_w = torch.from_numpy(w1.view(np.int32).copy()).cuda()
    d_o = torch.from_numpy(offs[: half + 1].astype(np.int64)).cuda()
    codes2 = codes[half * L:]
    offs2 = (offs[half:] - offs[half]).astype(np.uint64)
    with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=mode | pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.count_reads_device(d_w, w1.size, d_o, half, L)
        g.push_reads(synth.pack_2bit(codes2), offs2)               # no finish_count in between
        kmers, nodes = g.finish_count()
        assert (kmers, nodes) == (o.kmers_in_reads(), o.node_count())
        _, _, _, _, first = g.export_nodes(with_first=True)
        assert sorted(first.tolist()) == sorted(o.export_first().tolist())


@pytest.mark.parametrize("K,L,variant,p,small,n_reads", [(23, 100, 1, 8, False, 6000), (31, 150, 1, 1, False, 20000), (31, 150, 2, 3, True, 8000),
                                                         (47, 150, 2, 5, False, 6000), (75, 200, 4, 2, True, 5000), (31, 100, 4, 16, False, 30000),
                                                         (33, 120, 2, 4, True, 6000), (65, 200, 4, 3, False, 5000), (97, 250, 4, 5, True, 5000)])
def test_layout_replay_on_the_device_equals_the_reference_table(pkg, synth, K, L, variant, p, small, n_reads):
    """sdt_gpu_layout_on_device: the visiting order it numbers the nodes in == the slot order of the oracle's KmerSet (pinned to
    the reference's newhash.c by the unit vectors: growth sizes and final slots) after the set's distinct keys went in in
    first-occurrence order -- several growths per set, sets that start at 3 slots (-a), 1- / 2- / 4-word variants"""
    tx = synth.make_transcriptome(10, seed=K + variant)
    codes, offs = synth.sample_reads(*tx, n_reads=n_reads, read_len=L, seed=K + 1, err=0.01, ragged=True)
    OL = ob.lib()
    with pkg.PregraphGPU(K, est_distinct=1 << 15, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.push_reads(synth.pack_2bit(codes), offs)
        g.finish_count()
        g.mark_and_hist()
        skeys, ss = g.layout_sorted_keys(p, variant)
        nwk = skeys.shape[1]
        want = []
        for s in range(p):
            a, b = int(ss[s]), int(ss[s + 1])
            st = OL.sdto_set_new(3 if (small and variant != 1) else 1024, 0.77)
            for i in range(a, b):
                w4 = [0] * (4 - nwk) + [int(x) for x in skeys[i]]
                OL.sdto_set_put(st, ob.Kmer.of(w4), 4, 4, variant, None)
            slot = ob.C.c_uint64()
            where = []
            for i in range(a, b):
                w4 = [0] * (4 - nwk) + [int(x) for x in skeys[i]]
                assert OL.sdto_set_search(st, ob.Kmer.of(w4), variant, ob.C.byref(slot)) == 1
                where.append((slot.value, i))
            OL.sdto_set_free(st)
            want += [i for _, i in sorted(where)]
        ss2 = g.layout_on_device(p, variant, small)
        assert (ss2 == ss).all()
        k2, _, _, _ = g.export_ordered()
        assert (k2 == skeys[np.array(want, dtype=np.int64)]).all()
