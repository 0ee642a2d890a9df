"""GPU (-m gpu): sdt_gpu_screen_load / lookup / reads and their siblings against the Python restatement of the rule (read_screen_util.py).
Expectations never come from the library under test: the set is a dict from canonical k-mer to the smallest reference, the counts of
the compacted stream are the oracle's, and every output is compared for exact equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_screen_util as su
from test_kmer_search import keys_to_int, node_dict_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31                                                   # of the counting contexts; the screen has a k of its own


def load_case(g, synth, k, order=1):
    c = su.set_case(k)
    codes, offs = su.concat(c["seqs"][::order])
    return g.screen_load(synth.pack_2bit(codes), offs, c["refs"][::order], su.N_REFS, k)


def lookup_queries(k):
    d = su.set_dict(k)
    stored = sorted(d)
    absent = su.absent_kmers(k, d, 1000, seed=k)
    queries = stored + [su.revcomp_int(x, k) for x in stored] + absent
    want = [d[x] for x in stored] * 2 + [su.NO_REF] * len(absent)
    return np.array(queries, dtype=np.uint64), np.array(want, dtype=np.uint32)


def assert_screen(pkg, got, want, what):
    rec, keep, kept = got
    wrec, wkeep, wkept = want
    assert rec.dtype == pkg.READ_SCREEN_DTYPE
    su.assert_records_equal(rec, wrec, what)
    assert keep.dtype == np.uint8 and keep.tolist() == wkeep.tolist(), f"{what}: keep differs"
    assert kept == wkept == int(keep.sum()), f"{what}: {kept} reads kept, {wkept} expected"


# ---- 1. the set -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", su.KS)
def test_screen_set_equals_the_dict(pkg, synth, k):
    c = su.set_case(k)
    d = su.set_dict(k)
    offs = su.concat(c["seqs"])[1]
    assert set((offs[:-1] % 16).tolist()) == set(range(16))                   # a sequence starts at every base of a word
    shared = su.kmer_int(c["shared"])
    assert d[min(shared, su.revcomp_int(shared, k))] == 1 and d[0] == 3       # references 4, 1 and (reversed) 2; poly-A in 5, poly-T in 3
    if k == 16:
        pal = su.kmer_int(c["pal"])
        assert su.revcomp_int(pal, 16) == pal and pal in d
    queries, want = lookup_queries(k)
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        assert g.screen_info() == (0, 0, 0, 0)
        for order in (1, -1):                                                  # the sequences in reversed order give the same answers
            assert load_case(g, synth, k, order) == len(d)
            info = g.screen_info()
            assert info[:3] == (k, su.N_REFS, len(d)) and info[3] == 65536    # the power of two >= 2 x 31 500 positions
            got = g.screen_lookup(queries)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, f"k={k} order={order}: {len(bad)} look-ups differ, first {bad[:5].tolist()}"
        assert len(g.screen_lookup(np.zeros(0, dtype=np.uint64))) == 0
        # a key of more than 2 k bits is absent
        assert g.screen_lookup(np.array([(1 << 2 * k) | sorted(d)[0]], dtype=np.uint64)).tolist() == [su.NO_REF]


CHILD_SET = """
import os
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import read_screen_util as su
from test_read_screen import load_case, lookup_queries
k = {k}
rc = su.read_case(k)
refused = []
with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
    n = load_case(g, synth, k)
    info = g.screen_info()
    refs = g.screen_lookup(lookup_queries(k)[0][::{qstep}])
    rec, keep, kept = g.screen_reads(synth.pack_2bit(rc["codes"]), rc["offs"][:{nreads} + 1], paired={paired}, params=su.params())
    for v in {bad_slots!r}:                                # (the hook is read at every load)
        os.environ["SDT_SCREEN_SLOTS"] = v
        try:
            load_case(g, synth, k)
            refused.append("loaded")
        except pkg.SdtError as e:
            refused.append(str(e.code) + " " + str(e))
    still = g.screen_info()
np.savez({path!r}, n=np.uint64(n), info=np.array(info, dtype=np.uint64), refs=refs, rec=rec, keep=keep, kept=np.uint64(kept),
         refused=np.array(refused, dtype=str), still=np.array(still, dtype=np.uint64))
"""


def run_child(tmp_path, k, paired, nreads, bad_slots=(), qstep=1, **env):
    path = str(tmp_path / f"child{k}.npz")
    r = subprocess.run([sys.executable, "-c", CHILD_SET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path, k=k, paired=paired,
                                                               nreads=nreads, bad_slots=tuple(bad_slots), qstep=qstep)],
                       env=dict(os.environ, SDT_TEST_HOOKS="1", **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


def test_screen_set_in_a_full_table(pkg, synth, tmp_path):
    """SDT_SCREEN_SLOTS = 32 768 for 31 500 positions: the table is more than 90 % full, chains run into each other and across the table's
    end, and an absent key still ends at one of the few empty slots"""
    k = 21
    d, rc = su.set_dict(k), su.read_case(k)
    assert len(d) > 0.9 * 32768
    got = run_child(tmp_path, k, False, len(rc["offs"]) - 1, bad_slots=("30000", "16384", "31500"), SDT_SCREEN_SLOTS="32768")
    assert int(got["n"]) == len(d) and got["info"].tolist() == [k, su.N_REFS, len(d), 32768]
    assert (got["refs"] == lookup_queries(k)[1]).all()
    assert_screen(pkg, (got["rec"], got["keep"], int(got["kept"])), su.expect_screen(rc["codes"], rc["offs"], k, d, su.params(), facts=rc["facts"]),
                  "a full table")
    # a slot count that is no power of two, or leaves no empty slot: refused, and the set stays
    assert len(got["refused"]) == 3 and all(m.startswith(f"{pkg.SDT_EINVAL} ") and "SDT_SCREEN_SLOTS" in m for m in got["refused"].tolist()), got["refused"]
    assert got["still"].tolist() == got["info"].tolist()


# ---- 2. the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", su.KS)
def test_screen_equals_the_rule(pkg, synth, k):
    rc = su.read_case(k)
    d = su.set_dict(k)
    codes, offs, facts = rc["codes"], rc["offs"], rc["facts"]
    words = synth.pack_2bit(codes)
    n = len(offs) - 1
    lens = np.diff(offs.astype(np.int64))
    assert {0, k - 1, k, k + 1, k + 63, k + 64, 200, 5000} <= set(lens.tolist())
    # a read and its reverse complement get the same kmers, hits and ref: already in the restatement
    half = (n - 1) // 2
    assert all(facts[i] == facts[half + i] for i in range(half))
    ekm, ehits, _ = facts[rc["exact"]]
    assert ekm == 100 and 37 <= ehits < 100
    hits_seen = sorted(set(h for _, h, _ in facts if h > 1))
    h = hits_seen[len(hits_seen) // 2]                                        # a hit count that some read has exactly
    runs = [su.params(), su.params(min_hits=0), su.params(min_hits=h), su.params(min_hits=h + 1), su.params(min_hit_pct=ehits),
            su.params(min_hit_pct=ehits + 1), su.params(min_hit_pct=100), su.params(min_hits=h, min_hit_pct=50, flags=su.KEEP_MATCHED),
            su.params(flags=su.KEEP_MATCHED)]
    want = [su.expect_screen(codes, offs, k, d, p, facts=facts) for p in runs]
    # what the boundaries are about, in the expectation itself
    at = [i for i, f in enumerate(facts) if f[1] == h][0]
    assert want[2][0]["verdict"][at] == su.DROPPED and want[3][0]["verdict"][at] == su.KEPT          # hits = min_hits; hits = min_hits - 1
    assert want[4][0]["verdict"][rc["exact"]] == su.DROPPED and want[5][0]["verdict"][rc["exact"]] == su.KEPT      # 100 hits = pct kmers; one short
    assert want[0][1].tolist() == want[1][1].tolist()                                                  # min_hits 0 behaves as 1
    assert 0 < want[6][2] < n and {su.KEPT, su.DROPPED} <= set(want[6][0]["verdict"].tolist())         # pct 100: only reads that are all hits
    assert set(r for _, _, r in facts) >= {0, 1, 3, su.NO_REF}
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        load_case(g, synth, k)
        for i, (p, w) in enumerate(zip(runs, want)):
            assert_screen(pkg, g.screen_reads(words, offs, params=p), w, f"k={k} run {i}")
        rec, keep, kept = g.screen_reads(words, offs[:1])
        assert len(rec) == 0 and len(keep) == 0 and kept == 0


# ---- 3. pairs ---------------------------------------------------------------------------------------------------------------------
def test_screen_pairs(pkg, synth):
    k = 21
    c, d = su.set_case(k), su.set_dict(k)
    rng = np.random.default_rng(5)
    hit = lambda: c["seqs"][0][1000:1100].copy()
    miss = lambda: rng.integers(0, 4, size=int(rng.integers(60, 130)), dtype=np.uint8)
    reads = [hit(), miss(), miss(), hit(), hit(), hit(), miss(), miss()]
    codes, offs = su.concat(reads)
    words = synth.pack_2bit(codes)
    facts = su.all_facts(codes, offs, k, d)
    assert [f[1] > 0 for f in facts] == [True, False, False, True, True, True, False, False]
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        load_case(g, synth, k)
        for flags, dropped in ((0, [1, 1, 1, 1, 1, 1, 0, 0]), (su.KEEP_MATCHED, [0, 0, 0, 0, 0, 0, 1, 1])):
            want = su.expect_screen(codes, offs, k, d, su.params(flags=flags), paired=True, facts=facts)
            assert want[0]["verdict"].tolist() == dropped
            assert_screen(pkg, g.screen_reads(words, offs, paired=True, params=su.params(flags=flags)), want, f"pairs, flags={flags}")
        # every read keeps its own kmers, hits and ref
        rec = g.screen_reads(words, offs, paired=True)[0]
        assert rec["hits"][1] == 0 and rec["ref"][1] == su.NO_REF and rec["hits"][0] == 80 and rec["ref"][0] == 0
        # an odd number of reads
        out = np.full(7, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_SCREEN_DTYPE)
        prm = pkg.ScreenParams()
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_screen_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, 7, 1, ctypes.addressof(prm), out.ctypes.data, None,
                                          ctypes.byref(kept))
        assert code == pkg.SDT_EINVAL and "odd" in g.lib.sdt_gpu_last_error().decode()
        assert (out.view(np.uint32) == 0xABABABAB).all() and kept.value == 0


# ---- 4. where the reads start ---------------------------------------------------------------------------------------------------------
def test_screen_is_alignment_independent(pkg, synth):
    """the same reads behind one filler read of 0 .. 15 bases, and with offsets[0] = 7: every read starts at another base of its word"""
    k = 16
    rc, d = su.read_case(k), su.set_dict(k)
    p = su.params()
    base = su.expect_screen(rc["codes"], rc["offs"], k, d, p, facts=rc["facts"])
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        load_case(g, synth, k)
        for f in range(16):
            filler = np.resize(np.array([su.C, su.G], dtype=np.uint8), f)
            codes, offs = su.concat([filler] + rc["reads"])
            first = su.expect_screen(filler, np.array([0, f], dtype=np.uint64), k, d, p)
            want = tuple(np.concatenate([a, b]) for a, b in zip(first[:2], base[:2])) + (first[2] + base[2],)
            assert_screen(pkg, g.screen_reads(synth.pack_2bit(codes), offs, params=p), want, f"{f} filler bases")
        shifted = np.concatenate([np.full(7, su.T, dtype=np.uint8), rc["codes"]])
        assert_screen(pkg, g.screen_reads(synth.pack_2bit(shifted), rc["offs"] + np.uint64(7), params=p), base, "offsets[0] = 7")


# ---- 5. what is refused ---------------------------------------------------------------------------------------------------------------
def test_screen_refusals(pkg, synth):
    k = 21
    c, d, rc = su.set_case(k), su.set_dict(k), su.read_case(k)
    scodes, soffs = su.concat(c["seqs"])
    swords = synth.pack_2bit(scodes)
    srefs = np.array(c["refs"], dtype=np.uint32)
    words, offs = synth.pack_2bit(rc["codes"]), rc["offs"]
    n = len(offs) - 1
    untouched = np.full(n, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_SCREEN_DTYPE)
    want = su.expect_screen(rc["codes"], offs, k, d, su.params(), facts=rc["facts"])
    queries, qwant = lookup_queries(k)

    def screen_raw(prm):
        kept = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_screen_reads(g._ctx, words.ctypes.data, words.size, offs.ctypes.data, n, 0, ctypes.addressof(prm) if prm else None,
                                          untouched.ctypes.data, None, ctypes.byref(kept))
        return code, g.lib.sdt_gpu_last_error().decode(), kept.value

    def refused(code_want, prm, *say):
        code, msg, kept = screen_raw(prm)
        assert code == code_want and all(s in msg for s in say), f"{say}: {code} {msg}"
        assert (untouched.view(np.uint32) == 0xABABABAB).all() and kept == 0

    def load_raw(w, o, r, n_refs, kk, nseqs=None, nwords=None):
        nk = ctypes.c_uint64(99)
        code = g.lib.sdt_gpu_screen_load(g._ctx, w.ctypes.data, len(w) if nwords is None else nwords, o.ctypes.data, len(o) - 1 if nseqs is None else nseqs,
                                         r.ctypes.data, n_refs, kk, ctypes.byref(nk))
        return code, g.lib.sdt_gpu_last_error().decode(), nk.value

    def still_works(what):
        assert g.screen_info()[:3] == (k, su.N_REFS, len(d)), what
        assert (g.screen_lookup(queries[::37]) == qwant[::37]).all(), what
        assert_screen(pkg, g.screen_reads(words, offs), want, what)

    with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
        # without a set
        refused(pkg.SDT_ESTATE, pkg.ScreenParams(), "no reference set", "sdt_gpu_screen_load")
        with pytest.raises(pkg.SdtError) as e:
            g.screen_lookup(queries[:5])
        assert e.value.code == pkg.SDT_ESTATE and "no reference set" in str(e.value)
        # no reads: SDT_OK whatever the rest says, even without a set
        rec, keep, kept = g.screen_reads(words, offs[:1], params=su.params(min_hit_pct=200, flags=6, reserved=1))
        assert len(rec) == 0 and kept == 0
        assert g.screen_load(swords, soffs, srefs, su.N_REFS, k) == len(d)
        # the parameters
        refused(pkg.SDT_EINVAL, pkg.ScreenParams(min_hit_pct=101), "min_hit_pct", "101")
        refused(pkg.SDT_EINVAL, pkg.ScreenParams(flags=2), "flags", "0x2")
        refused(pkg.SDT_EINVAL, pkg.ScreenParams(flags=0x80000000), "flags", "0x80000000")
        refused(pkg.SDT_EINVAL, pkg.ScreenParams(reserved=7), "reserved", "7")
        refused(pkg.SDT_EINVAL, None, "params", "NULL")
        # every load that is refused says why and keeps the set
        bad_refs = srefs.copy()
        bad_refs[5] = su.N_REFS
        back = soffs.copy()
        back[3] = back[2] - 1
        tiny = su.concat([s for s in c["seqs"] if len(s) < k])
        for args, say in (((swords, soffs, srefs, su.N_REFS, 10), ("k = 10",)), ((swords, soffs, srefs, su.N_REFS, 32), ("k = 32",)),
                          ((swords, soffs, srefs, 0, k), ("n_refs = 0",)), ((swords, soffs, bad_refs, su.N_REFS, k), ("ref_of_seq[5]", "6")),
                          ((swords, back, srefs, su.N_REFS, k), ("monotonic",)),
                          ((synth.pack_2bit(tiny[0]), tiny[1], srefs[:len(tiny[1]) - 1], su.N_REFS, k), ("no k-mer",))):
            code, msg, nk = load_raw(*args)
            assert code == pkg.SDT_EINVAL and all(s in msg for s in say) and nk == 99, f"{say}: {code} {msg}"
            still_works(f"after a load refused for {say}")
        code, msg, nk = load_raw(swords, soffs, srefs, su.N_REFS, k, nwords=len(swords) - 1)              # a pad word short
        assert code == pkg.SDT_EINVAL and "too short" in msg and nk == 99
        still_works("after a load with too few words")
        # reset and counting leave the set alone
        g.push_reads(*(lambda co: (synth.pack_2bit(co[0]), co[1]))(su.concat([r for r in rc["reads"] if len(r) < 1000])))
        g.finish_count()
        still_works("after a count")
        g.reset()
        still_works("after sdt_gpu_reset")
        # a second load replaces it
        c2 = su.set_case(16)
        codes2, offs2 = su.concat(c2["seqs"])
        assert g.screen_load(synth.pack_2bit(codes2), offs2, c2["refs"], su.N_REFS, 16) == len(su.set_dict(16))
        assert g.screen_info()[0] == 16
        # unloaded: as without a set; unloading twice is fine
        g.screen_unload()
        g.screen_unload()
        assert g.screen_info() == (0, 0, 0, 0)
        refused(pkg.SDT_ESTATE, pkg.ScreenParams(), "no reference set")
        with pytest.raises(pkg.SdtError) as e:
            g.screen_lookup(queries[:5])
        assert e.value.code == pkg.SDT_ESTATE


# ---- 6. a host batch in pieces --------------------------------------------------------------------------------------------------------
def test_screen_in_pieces(pkg, synth, tmp_path):
    """SDT_SEARCH_CHUNK = 7, paired: the host form stages pieces of 6 reads (whole pairs), each rebased to its first word; it equals the
    restatement and the one-piece result"""
    k = 16
    rc, d = su.read_case(k), su.set_dict(k)
    n = len(rc["offs"]) - 1
    assert n % 2 == 1
    got = run_child(tmp_path, k, True, n - 1, qstep=211, SDT_SEARCH_CHUNK="7")   # (the case has an odd number of reads: all but the last)
    assert (got["refs"] == lookup_queries(k)[1][::211]).all()                  # 300 look-ups in pieces of 7 keys
    got = (got["rec"], got["keep"], int(got["kept"]))
    want = su.expect_screen(rc["codes"], rc["offs"][:-1], k, d, su.params(), paired=True, facts=rc["facts"][:-1])
    assert_screen(pkg, got, want, "pieces of 6 reads")
    with pkg.PregraphGPU(K, est_distinct=1 << 12) as g:
        load_case(g, synth, k)
        assert_screen(pkg, got, g.screen_reads(synth.pack_2bit(rc["codes"]), rc["offs"][:-1], paired=True), "pieces against the one-piece run")


# ---- 7. screen, compact, count: nothing crosses to the host ---------------------------------------------------------------------------
def test_screen_device_form_and_compaction(pkg, synth):
    import torch
    dev = torch.device("cuda:0")
    k = 21
    c, d = su.set_case(k), su.set_dict(k)
    rng = np.random.default_rng(31)
    tx = synth.make_transcriptome(12, seed=3)
    codes, offs = synth.sample_reads(*tx, n_reads=200, read_len=120, seed=4, err=0.0, ragged=True)
    reads = [codes[int(offs[r]):int(offs[r + 1])].copy() for r in range(len(offs) - 1)]
    reads = [r for r in reads if len(r) >= K + 1][:160]
    assert len(reads) == 160
    for i in range(0, 160, 4):                            # a quarter of the reads come from the references instead
        at = int(rng.integers(0, 5800))
        reads[i] = c["seqs"][1][at:at + int(rng.integers(40, 160))].copy()
    codes, offs = su.concat(reads)
    n = len(offs) - 1
    words = synth.pack_2bit(codes)
    d_w = torch.from_numpy(words.view(np.int32)).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    facts = su.all_facts(codes, offs, k, d)
    for paired, flags in ((False, 0), (True, 0), (False, su.KEEP_MATCHED)):
        p = su.params(flags=flags)
        wrec, wkeep, wkept = su.expect_screen(codes, offs, k, d, p, paired=paired, facts=facts)
        assert 30 <= wkept <= n - 30
        kcodes, koffs = su.concat(su.cut_kept(codes, offs, wrec))
        o2 = ob.Oracle(K, nsets=5)
        o2.add_reads(kcodes, koffs)
        want = {key: (v[0], v[1] & 0xFFFFFF, v[2]) for key, v in node_dict_oracle(o2).items()}
        d_rec = torch.full((n, 6), -3, dtype=torch.int32, device=dev)
        d_keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_ow = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
        d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        d_ow2 = torch.full((len(words),), -1, dtype=torch.int32, device=dev)
        d_oo2 = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # the screen runs on a context that never counts (a contig index): it needs the stream and the set only
        with pkg.PregraphGPU(K, est_distinct=1 << 16, flags=pkg.SDT_FLAG_CONTIG_INDEX) as a, pkg.PregraphGPU(K, est_distinct=1 << 16) as b:
            load_case(a, synth, k)
            assert a.screen_reads_device(d_w, d_o, n, d_rec, d_keep, paired=paired, params=p) == wkept
            assert d_keep.cpu().numpy().tolist() == wkeep.tolist()
            assert a.screen_reads_device(d_w, d_o, n, d_rec, None, paired=paired, params=p) == wkept                # d_keep may be NULL
            assert a.screen_reads_device(d_w, d_o, 0, None) == 0
            nr, nw = a.compact_reads_device(d_w, d_o, n, d_keep, d_ow, len(words), d_oo)
            assert nr == wkept and nw == (int(koffs[-1]) + 15) // 16
            nr2, nw2 = a.compact_trimmed_device(d_w, d_o, n, d_rec, d_ow2, len(words), d_oo2)                       # the records through the cast
            assert (nr2, nw2) == (nr, nw)
            b.count_reads_device(d_ow, nw + 4, d_oo, nr, int(np.diff(koffs.astype(np.int64)).max()))
            assert b.finish_count() == (o2.kmers_in_reads(), o2.node_count())
            keys, l, rf, cnt = b.export_nodes()[:4]
            assert_screen(pkg, a.screen_reads(words, offs, paired=paired, params=p), (wrec, wkeep, wkept), "a contig index, host form")
        got_rec = d_rec.cpu().numpy().view(np.uint8).copy().view(pkg.READ_SCREEN_DTYPE).reshape(-1)
        su.assert_records_equal(got_rec, wrec, f"device form, paired={paired} flags={flags}")
        assert d_oo.cpu().numpy()[: nr + 1].tolist() == koffs.tolist() and d_oo2.cpu().numpy()[: nr + 1].tolist() == koffs.tolist()
        assert d_ow.cpu().numpy()[:nw].tolist() == d_ow2.cpu().numpy()[:nw].tolist()
        assert d_ow.cpu().numpy()[:nw].view(np.uint32).tolist() == synth.pack_2bit(kcodes)[:nw].tolist()
        got = {key: (int(x), int(y) & 0xFFFFFF, int(z)) for key, x, y, z in zip(keys_to_int(keys), l, rf, cnt)}
        assert len(got) == len(want) and got == want, (paired, flags)


# ---- 8. kept reads ----------------------------------------------------------------------------------------------------------------
def test_screen_kept_reads(pkg, synth):
    """three keep_reads batches: the read-1 file (ordinals base, base + 2, ...), the read-2 file (base + 1, base + 3, ...; one read
    short, so the last pair has one mate), and single reads behind the range; no read has ordinals 0 .. 2"""
    k = 21
    c, d = su.set_case(k), su.set_dict(k)
    rng = np.random.default_rng(83)
    def hit():
        a = int(rng.integers(0, 19000))
        return c["seqs"][0][a:a + int(rng.integers(50, 200))].copy()
    miss = lambda: rng.integers(0, 4, size=int(rng.integers(10, 200)), dtype=np.uint8)
    P, base = 12, 3
    r1 = [hit() if t % 3 == 0 else miss() for t in range(P + 1)]            # the last one's mate is missing
    r2 = [hit() if t % 4 == 1 else miss() for t in range(P)]
    singles = [hit() if t % 2 else miss() for t in range(7)]
    first, end = base, base + 2 * (P + 1)
    ords = [base + 2 * t for t in range(P + 1)] + [base + 1 + 2 * t for t in range(P)] + [end + t for t in range(7)]
    total = end + 7
    codes, offs = su.concat(r1 + r2 + singles)
    facts = su.all_facts(codes, offs, k, d)
    lens = np.diff(offs.astype(np.int64)).tolist()
    by_ord = {o: i for i, o in enumerate(ords)}
    absent = np.ones(total, dtype=bool)
    absent[ords] = False
    assert absent.sum() == 4

    def expect(p, ranges):
        units = [[by_ord[o] for o in u] for u in su.ranged_units(ords, ranges)]
        rec, keep, kept = su.verdicts(facts, lens, p, units)
        out = np.zeros(total, dtype=su.DTYPE)
        out[ords] = rec
        return out, kept

    # the case holds what it promises: pairs of which the first mate, the second, both and neither hit
    mix = set((facts[by_ord[base + 2 * t]][1] > 0, facts[by_ord[base + 2 * t + 1]][1] > 0) for t in range(P))
    assert mix == {(True, False), (False, True), (False, False), (True, True)}
    with pkg.PregraphGPU(K, est_distinct=1 << 14) as g:
        load_case(g, synth, k)
        with pytest.raises(pkg.SdtError) as e:                              # no kept reads yet
            g.screen_kept_reads(total, [(first, end)])
        assert e.value.code == pkg.SDT_ESTATE and "kept" in str(e.value)
        for batch, b, stride in ((r1, base, 2), (r2, base + 1, 2), (singles, end, 1)):
            g.set_read_ordinal(b, stride)
            bc, bo = su.concat(batch)
            g.keep_reads(synth.pack_2bit(bc), bo)
        for flags in (0, su.KEEP_MATCHED):
            for ranges in ([(first, end)], [], [(first, first + 8), (first + 8, end)]):
                p = su.params(flags=flags)
                wrec, wkept = expect(p, ranges)
                out = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_SCREEN_DTYPE)
                rec, nr, kept = g.screen_kept_reads(total, ranges, params=p, out=out)
                assert nr == len(ords) and kept == wkept
                assert (np.ascontiguousarray(rec[absent]).view(np.uint32) == 0xABABABAB).all()
                su.assert_records_equal(rec[~absent], wrec[~absent], f"kept reads, flags={flags}, ranges={ranges}")
        # the pair whose second mate is missing is a unit of its first mate
        wrec, _ = expect(su.params(), [(first, end)])
        lone = base + 2 * P
        assert wrec["verdict"][lone] == (su.DROPPED if facts[by_ord[lone]][1] else su.KEPT)
        # one record short: SDT_EFULL and nothing written
        small = np.full(total - 1, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_SCREEN_DTYPE)
        with pytest.raises(pkg.SdtError) as e:
            g.screen_kept_reads(total - 1, [(first, end)], out=small)
        assert e.value.code == pkg.SDT_EFULL and "ordinal" in str(e.value)
        assert (small.view(np.uint32) == 0xABABABAB).all()
        full = np.full(total, 0xABABABAB, dtype=np.uint32).repeat(6).view(pkg.READ_SCREEN_DTYPE)
        for bad in ([(first, end), (end - 2, end + 2)], [(first, first + 3)], [(end, first)]):
            with pytest.raises(pkg.SdtError) as e:
                g.screen_kept_reads(total, bad, out=full)
            assert e.value.code == pkg.SDT_EINVAL and "range" in str(e.value)
            assert (full.view(np.uint32) == 0xABABABAB).all()
        with pytest.raises(pkg.SdtError) as e:
            g.screen_kept_reads(total, [(first, end)], params=su.params(flags=4))
        assert e.value.code == pkg.SDT_EINVAL
        # the kept reads are as they were
        bc, bo = su.concat(r2)
        w, o, b, stride = g.fetch_kept_batch(1)
        assert (b, stride) == (base + 1, 2) and o.tolist() == bo.tolist() and w[:len(w) - 4].tolist() == synth.pack_2bit(bc)[:len(w) - 4].tolist()
