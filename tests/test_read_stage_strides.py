"""GPU (-m gpu; the conditions on the inputs also run on the CPU): the read stages when a wavefront takes read after read, and a lane
item after item.

Every read stage gives a wavefront one read (or one pair) and strides over the batch; the grid is capped at cu_count * 32 workgroups
(wave_blocks, csrc/sdt_read_plan.h), so on a device of 256 CUs only a batch of more than 32 768 reads sends a wavefront round its loop
a second time.  The batches of the other tests have 120 to 6 000 reads.  Here SDT_WAVE_BLOCKS (1 and 3 workgroups) and
SDT_SCAN_BLOCKS = 1 make the same batches go round many times: what a wavefront carries from one read to the next -- the LDS strip
of the strip kernels, the counters, the wave-uniform state -- and the stride itself are compared with the restatements the stages'
own tests use, and with the run without the hooks.

The hooks are read once per process: a child process per stage and value of SDT_WAVE_BLOCKS runs the stage (`RUNS[stage]`), saves
every output, and the parent compares.  The same function runs in the parent without the hooks.  Every test asserts about its own
input that the runs can show something: at least 8 reads (units) per wavefront, at least a quarter of the reads r >= W shorter than
read r - W (W: the wavefronts of the grid; a stale strip tail or stale state then lies behind the shorter read's end), and a read
that the stage skips (shorter than K, empty, too long) with a normal read W further on.  All comparisons are exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import read_clip_util as rcl
import read_complexity_util as cu
import read_correct_util as rc
import read_dedup_util as rd
import read_overlap_util as ru
import read_quality_util as qu
import read_screen_util as su
import read_select_util as rs
import read_trim_util as rt
import test_kmer_search as tks
import test_read_correct as trc
import test_read_select as trs
import test_read_trim as trt
from test_read_clip import assert_clip
from test_read_complexity import TRIM, assert_cx
from test_read_dedup import assert_dedup
from test_read_overlap import assert_overlap
from test_read_quality import assert_q
from test_read_screen import assert_screen, load_case, lookup_queries
from test_read_select_host import length_mix
from test_read_trim_host import range_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_BLOCKS = (1, 3)                                    # SDT_WAVE_BLOCKS of the children
KS = (31, 63)
ONE_WAVE = 16000                                        # a promise of that many bases: one wavefront per workgroup (strip_geometry)
TOO_LONG = 0xFFFFFFFF
EINVAL = -1                                             # (checked against pkg.SDT_EINVAL in the parent)


# ---- the stride conditions ------------------------------------------------------------------------------------------------------------
def strip_waves(K, promise):
    """the wavefronts per workgroup of a strip kernel over reads of up to `promise` bases (strip_geometry, csrc/sdt_read_plan.h)"""
    mk = max(promise, K) - K + 1
    assert mk <= 16384
    return 4 if mk <= 4096 else 2 if mk <= 8192 else 1


def assert_strides(what, lens, skipped, unit, waves, reached):
    """lens: the bases of every read; skipped: the reads the stage skips or drops before its work; unit: reads per wavefront's item
    (2: pairs); waves: the wavefronts per workgroup of the launch.  For the grids of both hook values.  reached[what]: the items per
    wavefront"""
    lens, skipped = np.asarray(lens, dtype=np.int64), np.asarray(skipped, dtype=bool)
    n = len(lens) // unit
    for b in WAVE_BLOCKS:
        W = waves * b
        s = W * unit                                    # read r and read r - s are taken by the same wavefront, as the same mate
        assert n >= 8 * W, f"{what}: {n} units for {W} wavefronts"
        shorter = float((lens[s:] < lens[:len(lens) - s]).mean())
        assert shorter >= 0.25, f"{what}: only {shorter:.2f} of the reads r >= {s} are shorter than read r - {s}"
        follow = int((skipped[:len(lens) - s] & ~skipped[s:]).sum())
        assert follow >= 1, f"{what}: no skipped read has a normal read {s} reads further on"
        reached[f"{what}, {W} wavefronts"] = n // W


# ---- outputs through a file -----------------------------------------------------------------------------------------------------------
def flatten(runs):
    """{run: tuple of arrays and integers} -> what np.savez takes"""
    return {f"{name}|{i}": (x if isinstance(x, np.ndarray) else np.int64(x)) for name, outs in runs.items() for i, x in enumerate(outs)}


def unflatten(npz):
    runs = {}
    for key in npz.files:
        name, i = key.rsplit("|", 1)
        x = npz[key]
        runs.setdefault(name, {})[int(i)] = int(x) if x.ndim == 0 else x
    return {name: tuple(outs[i] for i in range(len(outs))) for name, outs in runs.items()}


def dev(a):
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed)).cuda()


def filled(shape, value, dtype="int32"):
    import torch
    t = torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda:0")
    torch.cuda.synchronize()
    return t


def records(t, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8).reshape(-1).view(dtype).copy()


def promised(pkg, call):
    """a device form under a promise that some reads break: -> (what it returns or None, the error code or 0)"""
    try:
        return call(), 0
    except pkg.SdtError as e:
        assert "longer" in str(e), str(e)
        return None, e.code


# ---- search_kmers (a lane per query: SDT_SCAN_BLOCKS) -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def search_case(K):
    """the workload and the queries of test_search_equals_oracle: every node as stored, its reverse complement, k-mers that are absent,
    one query 200 times"""
    from soapdenovo_trans_amd import synth
    _, codes, offs = tks.workload(synth, K, 150 if K <= 31 else 250)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    o.mark()
    nodes = tks.node_dict_oracle(o)
    stored = sorted(nodes)
    queries = stored + [tks.revcomp_int(k, K) for k in stored] + tks.absent_kmers(K, nodes, 1000 + K) + [stored[len(stored) // 3]] * 200
    return dict(codes=codes, offs=offs, nodes=nodes, queries=queries, keys=tks.int_to_keys(queries, 1 if K <= 31 else 2),
                oracle=(o.kmers_in_reads(), o.node_count()))


def run_search(pkg, synth):
    out = {}
    for K in KS:
        c = search_case(K)
        with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
            g.push_reads(synth.pack_2bit(c["codes"]), c["offs"])
            assert g.finish_count() == c["oracle"]
            g.mark_and_hist()
            out[f"K={K}"] = g.search_kmers(c["keys"])
    return out


@functools.lru_cache(maxsize=None)
def want_search():
    return {f"K={K}": tks.expect_search(search_case(K)["queries"], K, search_case(K)["nodes"]) for K in KS}


def check_search(pkg, got, want, what):
    assert len(got) == len(want) == 4
    for name, a, b in zip(("count", "l_links", "r_flags", "status"), got, want):
        bad = np.nonzero(a != b)[0]
        assert a.shape == b.shape and bad.size == 0, f"{what}: {name} differs at {bad[:8].tolist()}: got {a[bad[:8]].tolist()} want {b[bad[:8]].tolist()}"


def strides_search(reached):
    for K in KS:                                        # one workgroup of 256 lanes takes every query
        n = len(search_case(K)["queries"])
        assert n >= 8 * 256
        reached[f"search K={K}, 256 lanes"] = n // 256


# ---- the strip stages: what a promise that some reads break leaves ------------------------------------------------------------------------
def strip_runs(lens, K):
    """(run, promise, wavefronts per workgroup, the reads the run skips) of a strip stage: the host form (the promise is the longest
    read), the device form under a promise of 16 000 bases (one wavefront per workgroup), and the device form under a promise one
    base short of the longest read, which marks that read"""
    longest = int(lens.max())
    return [("host", longest, strip_waves(K, longest), lens < K), ("one wave", ONE_WAVE, 1, lens < K),
            ("short", longest - 1, strip_waves(K, longest - 1), (lens < K) | (lens == longest))]


def strides_strip(what, lens, K, unit, reached, runs=("host", "one wave", "short")):
    for run, _, waves, skipped in strip_runs(lens, K):
        if run in runs:
            assert run != "short" or 1 <= (lens == lens.max()).sum() < len(lens) // 4
            assert_strides(f"{what} K={K} {run}", lens, skipped, unit, waves, reached)


# ---- profile_reads ------------------------------------------------------------------------------------------------------------------------
PROFILE_MIN_COUNT = 2


@functools.lru_cache(maxsize=None)
def profile_case(K):
    """the batch of test_profile_equals_numpy: ragged reads of the counted workload, hand-made reads of K - 1, K and K + 1 bases and of
    more than 256 k-mers, reads of another seed that hold k-mers the table does not have"""
    from soapdenovo_trans_amd import synth
    L = 150 if K <= 31 else 250
    tx, codes, offs = tks.workload(synth, K, L, n_reads=4000)
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    t = tx[0]
    hand = [t[100:100 + K - 1], t[200:200 + K], (t[300:300 + K + 1][::-1] ^ 2).astype(np.uint8), t[40:40 + 330], t[10:10 + 480],
            np.zeros(K + 5, dtype=np.uint8)]
    other, ooffs = synth.sample_reads(*tx, n_reads=400, read_len=L, seed=K + 99, err=0.02, ragged=True)
    lens = np.concatenate([np.diff(offs.astype(np.int64)), [len(h) for h in hand], np.diff(ooffs.astype(np.int64))])
    pcodes = np.concatenate([codes] + hand + [other])
    poffs = np.zeros(len(lens) + 1, dtype=np.uint64)
    poffs[1:] = np.cumsum(lens)
    return dict(codes=codes, offs=offs, pcodes=pcodes, poffs=poffs, lens=lens, nodes=tks.node_dict_oracle(o), oracle=(o.kmers_in_reads(), o.node_count()))


def run_profile(pkg, synth):
    out = {}
    for K in KS:
        c = profile_case(K)
        words, n = synth.pack_2bit(c["pcodes"]), len(c["lens"])
        with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
            g.push_reads(synth.pack_2bit(c["codes"]), c["offs"])
            assert g.finish_count() == c["oracle"]
            out[f"K={K} host"] = (g.profile_reads(words, c["poffs"], min_count=PROFILE_MIN_COUNT),)
            d_w, d_o = dev(words), dev(c["poffs"])
            for run, promise, _, _ in strip_runs(c["lens"], K)[1:]:
                d_cov = filled((n, 6), -1)
                _, code = promised(pkg, lambda: g.profile_reads_device(d_w, d_o, n, promise, PROFILE_MIN_COUNT, d_cov))
                out[f"K={K} {run}"] = (records(d_cov, pkg.READ_COV_DTYPE), code)
    return out


@functools.lru_cache(maxsize=None)
def want_profile():
    out = {}
    for K in KS:
        c = profile_case(K)
        cov = tks.expect_profile(c["pcodes"], c["poffs"], K, c["nodes"], PROFILE_MIN_COUNT)
        marked = cov.copy()
        marked[c["lens"] == c["lens"].max()] = (TOO_LONG, 0, 0, 0, 0, 0)
        out.update({f"K={K} host": (cov,), f"K={K} one wave": (cov, 0), f"K={K} short": (marked, EINVAL)})
    return out


def check_profile(pkg, got, want, what):
    assert got[0].dtype == pkg.READ_COV_DTYPE and len(got) == len(want)
    tks.assert_cov_equal(got[0], want[0], what)
    assert got[1:] == want[1:], f"{what}: error code {got[1:]}, expected {want[1:]}"


def strides_profile(reached):
    for K in KS:
        strides_strip("profile", profile_case(K)["lens"], K, 1, reached)


# ---- correct_reads -------------------------------------------------------------------------------------------------------------------------
CORRECT_MIN_COUNT = 3
CORRECT_TAIL = 40


@functools.lru_cache(maxsize=None)
def correct_case(K):
    """the case of test_read_correct.py with a second, differently seeded draw of 40 reads of its workload behind it: the hand-made
    reads, the one of K - 1 bases among them, are the last of the case, and a read that is skipped needs a normal read 12 reads
    further on.  The restatement of the tail is computed for the tail, with its own read numbers in the edits"""
    from soapdenovo_trans_amd import synth
    c = trc.case(K)
    tail, toffs = synth.sample_reads(*synth.make_transcriptome(25, seed=K), n_reads=CORRECT_TAIL, read_len=c["L"], seed=K + 501, err=0.003, ragged=True)
    n = len(c["boffs"]) - 1
    fix, codes, edits = trc.expected(K, CORRECT_MIN_COUNT)
    tfix, tcodes, tedits = rc.expect_correct(tail, toffs, K, c["count"], CORRECT_MIN_COUNT)
    assert (np.diff(toffs.astype(np.int64)) >= K).all() and int(tfix["fixed"].sum()) == len(tedits)
    want = (np.concatenate([fix, tfix]), np.concatenate([codes, tcodes]), np.concatenate([edits, tedits + np.uint64(n << 18)]))
    return dict(c, batch=np.concatenate([c["batch"], tail]), boffs=np.concatenate([c["boffs"], toffs[1:] + c["boffs"][-1]]), want=want)


def run_correct(pkg, synth):
    out = {}
    for K in KS:
        c = correct_case(K)
        words, n = synth.pack_2bit(c["batch"]), len(c["boffs"]) - 1
        lens = np.diff(c["boffs"].astype(np.int64))
        with trc.counted_context(pkg, synth, c) as g:
            out[f"K={K} host"] = g.correct_reads(words, c["boffs"], CORRECT_MIN_COUNT)
            d_w, d_o = dev(words), dev(c["boffs"])
            cap = int(lens.sum())                           # (room for an edit at every base)
            for run, promise, _, _ in strip_runs(lens, K)[1:]:
                d_fix = filled((n, 4), -1)
                d_out = filled((len(words),), -1)
                d_ed = filled((cap,), -1, "int64")
                try:
                    edits, code = g.correct_reads_device(d_w, len(words), d_o, n, promise, CORRECT_MIN_COUNT, d_fix, d_out, d_ed, cap), 0
                except pkg.SdtError as e:
                    assert "longer" in str(e), str(e)
                    edits, code = e.needed, e.code
                ed = d_ed.cpu().numpy().view(np.uint64)
                assert (ed[edits:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
                out[f"K={K} {run}"] = (records(d_fix, pkg.READ_FIX_DTYPE), d_out.cpu().numpy().view(np.uint32), np.sort(ed[:edits]), code)
    return out


@functools.lru_cache(maxsize=None)
def want_correct():
    from soapdenovo_trans_amd import synth
    out = {}
    for K in KS:
        c = correct_case(K)
        fix, codes, edits = c["want"]
        lens = np.diff(c["boffs"].astype(np.int64))
        # the read that is too long: marked, as it came in the output, none of its edits
        long_reads = np.nonzero(lens == lens.max())[0]
        marked, undone = fix.copy(), codes.copy()
        for r in long_reads.tolist():
            marked[r] = (TOO_LONG, 0, 0, 0)
            undone[int(c["boffs"][r]):int(c["boffs"][r + 1])] = c["batch"][int(c["boffs"][r]):int(c["boffs"][r + 1])]
        left = np.array([e for e in edits.tolist() if (e >> 18) not in set(long_reads.tolist())], dtype=np.uint64)
        assert len(left) < len(edits), "the longest read must hold edits"
        out.update({f"K={K} host": (fix, synth.pack_2bit(codes), edits), f"K={K} one wave": (fix, synth.pack_2bit(codes), edits, 0),
                    f"K={K} short": (marked, synth.pack_2bit(undone), left, EINVAL)})
    return out


def check_correct(pkg, got, want, what):
    assert got[0].dtype == pkg.READ_FIX_DTYPE and len(got) == len(want)
    rc.assert_fix_equal(got[0], want[0], what)
    bad = np.nonzero(got[1] != want[1])[0] if got[1].shape == want[1].shape else None
    assert bad is not None and bad.size == 0, f"{what}: out_words differ at words {None if bad is None else bad[:8].tolist()}"
    assert got[2].dtype == np.uint64 and got[2].tolist() == want[2].tolist(), f"{what}: edits differ"
    assert got[3:] == want[3:], f"{what}: error code {got[3:]}, expected {want[3:]}"


def strides_correct(reached):
    for K in KS:
        strides_strip("correct", np.diff(correct_case(K)["boffs"].astype(np.int64)), K, 1, reached)


# ---- select_reads ----------------------------------------------------------------------------------------------------------------------------
SELECT_CV, SELECT_SEED = trs.SETTINGS[1]


def run_select(pkg, synth):
    out = {}
    for K in KS:
        c = trs.case(K)
        words, n = synth.pack_2bit(c["batch"]), len(c["boffs"]) - 1
        lens = np.diff(c["boffs"].astype(np.int64))
        prm = dict(target=trs.TARGET, max_cv_pct=SELECT_CV, seed=SELECT_SEED)
        with trs.counted_context(pkg, synth, c) as g:
            d_w, d_o = dev(words), dev(c["boffs"])
            for paired in (False, True):
                out[f"K={K} paired={paired} host"] = g.select_reads(words, c["boffs"], paired=paired, **prm)
                for run, promise, _, _ in strip_runs(lens, K)[1:]:
                    d_pick, d_keep = filled((n, 4), -2), dev(np.full(n, 7, dtype=np.uint8))
                    kept, code = promised(pkg, lambda: g.select_reads_device(d_w, d_o, n, promise, d_pick, d_keep, paired=paired, **prm))
                    pick, keep = records(d_pick, pkg.READ_PICK_DTYPE), d_keep.cpu().numpy()
                    out[f"K={K} paired={paired} {run}"] = (pick, keep, int(keep.sum()) if kept is None else kept, code)
    return out


@functools.lru_cache(maxsize=None)
def want_select():
    out = {}
    for K in KS:
        c = trs.case(K)
        lens = np.diff(c["boffs"].astype(np.int64))
        for paired in (False, True):
            want = trs.expected(K, SELECT_CV, SELECT_SEED, paired)
            out[f"K={K} paired={paired} host"] = want
            out[f"K={K} paired={paired} one wave"] = want + (0,)
        # a read that is too long is marked and dropped as short, and counts as a read without k-mers for its mate (include/sdt_gpu.h)
        longest = lens == lens.max()
        kc = [[] if longest[r] else c["kc"][r] for r in range(len(lens))]
        for paired in (False, True):
            pick, keep, _ = rs.expect_select(c["batch"], c["boffs"], K, c["count"], trs.TARGET, SELECT_CV, SELECT_SEED, paired=paired, kmer_counts=kc)
            pick[longest] = (TOO_LONG, 0, 0, rs.SHORT)
            keep[longest] = 0
            out[f"K={K} paired={paired} short"] = (pick, keep, int(keep.sum()), EINVAL)
        r = int(np.nonzero(longest)[0][0])                  # its mate is decided alone
        mate, whole = out[f"K={K} paired=True short"][0][r ^ 1], trs.expected(K, SELECT_CV, SELECT_SEED, True)[0][r ^ 1]
        assert mate["kmers"] == whole["kmers"] and (mate["cov"] != whole["cov"] or mate["verdict"] != whole["verdict"] or whole["kmers"] == 0)
    return out


def check_select(pkg, got, want, what):
    trs.assert_select(pkg, got[:3], want[:3], what)
    assert got[3:] == want[3:], f"{what}: error code {got[3:]}, expected {want[3:]}"


def strides_select(reached):
    for K in KS:
        lens = np.diff(trs.case(K)["boffs"].astype(np.int64))
        strides_strip("select", lens, K, 1, reached)
        strides_strip("select paired", lens, K, 2, reached)


# ---- trim_reads --------------------------------------------------------------------------------------------------------------------------------
def trim_settings(K):
    """(min_count, min_cov, min_len, flags): plain, and with SDT_TRIM_CORRECTED"""
    return trt.settings(K)[0], trt.settings(K)[4]


@functools.lru_cache(maxsize=None)
def trim_short_case(K):
    """The case of test_read_trim.py holds a read of 8 300 k-mers, so every launch over it has one wavefront per workgroup.  Here: two
    draws of its generator (other transcripts, other reads), each without its three long reads, one behind the other -- 156 reads of
    at most 137 + 2 K bases, which four wavefronts of a workgroup share.  Both draws' inputs are counted into one table; the counts
    and the restatement are computed for the whole"""
    draws = [trt.case(K), trt.case(K, seed=7000 + K)]
    counted = np.concatenate([d["counted"] for d in draws])
    coffs = np.concatenate([draws[0]["coffs"], draws[1]["coffs"][1:] + draws[0]["coffs"][-1]])
    o = ob.Oracle(K, nsets=5)
    o.add_reads(counted, coffs)
    count = rc.table_counts(tks.node_dict_oracle(o))
    reads = [d["batch"][int(d["boffs"][r]):int(d["boffs"][r + 1])] for d in draws for r in range(len(d["boffs"]) - 1) if r not in d["tags"]["long"]]
    batch, boffs = trc.concat(reads)
    assert len(reads) >= 8 * 12 and max(len(r) for r in reads) == 137 + 2 * K      # (the read whose stretch begins at k-mer 64 and ends at 128)
    return dict(K=K, counted=counted, coffs=coffs, count=count, batch=batch, boffs=boffs, kc=rt.read_kmer_counts(batch, boffs, K, count),
                oracle=(o.kmers_in_reads(), o.node_count()))


def trim_batches(K):
    """(name, case): the case of test_read_trim.py (one wavefront per workgroup) and the short reads of two draws (four)"""
    return (("whole case", trt.case(K)), ("short reads", trim_short_case(K)))


def run_trim(pkg, synth):
    out = {}
    for K in KS:
        for name, c in trim_batches(K):
            words, n = synth.pack_2bit(c["batch"]), len(c["boffs"]) - 1
            lens = np.diff(c["boffs"].astype(np.int64))
            with trt.counted_context(pkg, synth, c) as g:
                d_w, d_o = dev(words), dev(c["boffs"])
                for prm in trim_settings(K):
                    out[f"K={K} {name} flags={prm[3]} host"] = g.trim_reads(words, c["boffs"], *prm)
                    for run, promise, _, _ in strip_runs(lens, K)[1:]:
                        d_trim, d_keep = filled((n, 6), -2), dev(np.full(n, 7, dtype=np.uint8))
                        kept, code = promised(pkg, lambda: g.trim_reads_device(d_w, d_o, n, promise, d_trim, d_keep, *prm))
                        trim, keep = records(d_trim, pkg.READ_TRIM_DTYPE), d_keep.cpu().numpy()
                        out[f"K={K} {name} flags={prm[3]} {run}"] = (trim, keep, int(keep.sum()) if kept is None else kept, code)
    return out


@functools.lru_cache(maxsize=None)
def want_trim():
    out = {}
    for K in KS:
        for name, c in trim_batches(K):
            lens = np.diff(c["boffs"].astype(np.int64))
            longest = int(lens.max())
            for prm in trim_settings(K):
                want = trt.expected(K, prm) if name == "whole case" else rt.expect_trim(c["batch"], c["boffs"], K, c["count"], prm, kmer_counts=c["kc"])
                marked = rt.expect_trim(c["batch"], c["boffs"], K, c["count"], prm, kmer_counts=c["kc"], max_read_len=longest - 1)
                assert (marked[0]["kmers"] == TOO_LONG).sum() == (lens == longest).sum() >= 1
                if name == "short reads":                   # (the batch still holds what the case is about)
                    assert {rt.WHOLE, rt.TRIMMED, rt.DROPPED, rt.SHORT} <= set(want[0]["verdict"].tolist()) and 20 <= want[2] <= len(lens) - 20
                tag = f"K={K} {name} flags={prm[3]}"
                out.update({f"{tag} host": want, f"{tag} one wave": want + (0,), f"{tag} short": marked + (EINVAL,)})
    return out


def check_trim(pkg, got, want, what):
    trt.assert_trim(pkg, got[:3], want[:3], what)
    assert got[3:] == want[3:], f"{what}: error code {got[3:]}, expected {want[3:]}"


def strides_trim(reached):
    for K in KS:
        for name, c in trim_batches(K):
            lens = np.diff(c["boffs"].astype(np.int64))
            # the whole case: one wavefront per workgroup in every run; the short reads: four in the host form and under the short promise
            assert [w for _, _, w, _ in strip_runs(lens, K)] == ([1, 1, 1] if name == "whole case" else [4, 1, 4])
            strides_strip(f"trim, {name}", lens, K, 1, reached)


# ---- the stages that need no table: a workgroup of 4 wavefronts, a read (a pair) each ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def dedup_paired_case():
    """three draws of rd.paired_case(): 120 pairs (one draw has 40, too few for 12 wavefronts); not a tiling -- the draws share the two
    empty reads and nothing else, and the restatement is computed on the whole"""
    pairs = [pr for seed in (20240918, 20240928, 20240938) for pr in rd.paired_case(seed)["pairs"]]
    codes, offs = rd.concat([r for pr in pairs for r in pr])
    return dict(codes=codes, offs=offs, pairs=pairs)


def run_dedup(pkg, synth):
    c, p = rd.case(), dedup_paired_case()
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"single": g.dedup_reads(synth.pack_2bit(c["codes"]), c["offs"]),
                "paired": g.dedup_reads(synth.pack_2bit(p["codes"]), p["offs"], paired=True),
                "mate swap": g.dedup_reads(synth.pack_2bit(p["codes"]), p["offs"], paired=True, flags=rd.MATE_SWAP)}


@functools.lru_cache(maxsize=None)
def want_dedup():
    c, p = rd.case(), dedup_paired_case()
    want = {"single": rd.expect_dedup(c["codes"], c["offs"]), "paired": rd.expect_dedup(p["codes"], p["offs"], paired=True),
            "mate swap": rd.expect_dedup(p["codes"], p["offs"], paired=True, flags=rd.MATE_SWAP)}
    # the draws stay apart: three times the classes of one, less the class of the empty pair that they share
    one = len(set(rd.expect_dedup(rd.paired_case()["codes"], rd.paired_case()["offs"], paired=True)[0]["first"].tolist()))
    assert len(set(want["paired"][0]["first"].tolist())) == 3 * one - 2
    return want


def strides_dedup(reached):
    for what, c, unit in (("dedup", rd.case(), 1), ("dedup paired", dedup_paired_case(), 2)):
        lens = np.diff(c["offs"].astype(np.int64))
        assert_strides(what, lens, lens == 0, unit, 4, reached)


def run_clip(pkg, synth):
    c = rcl.case()
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"clip": g.clip_reads(synth.pack_2bit(c["codes"]), c["offs"], c["adapters"], c["params"])}


def strides_clip(reached):
    lens = np.diff(rcl.case()["offs"].astype(np.int64))
    assert_strides("clip", lens, lens == 0, 1, 4, reached)


@functools.lru_cache(maxsize=None)
def overlap_case():
    """three draws of ru.case(): 120 pairs"""
    pairs = [pr for seed in (20241020, 20241030, 20241040) for pr in ru.case(seed)["pairs"]]
    codes, offs = rd.concat([r for pr in pairs for r in pr])
    return dict(codes=codes, offs=offs, pairs=pairs, params=ru.case()["params"])


def run_overlap(pkg, synth):
    c = overlap_case()
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"overlap": g.overlap_pairs(synth.pack_2bit(c["codes"]), c["offs"], c["params"])}


@functools.lru_cache(maxsize=None)
def want_overlap():
    c = overlap_case()
    want = ru.expect_overlap(c["codes"], c["offs"], c["params"])
    n = len(ru.case()["offs"]) - 1
    ru.assert_overlap_equal(want[0][:n], ru.case_expect()[0], "the first draw is the case")
    return {"overlap": want}


def strides_overlap(reached):
    c = overlap_case()
    lens = np.diff(c["offs"].astype(np.int64))
    short = lens < c["params"]["min_overlap"]                  # a pair with such a mate is tried at no shift
    assert_strides("overlap", lens, np.repeat(short[0::2] | short[1::2], 2), 2, 4, reached)


def run_complexity(pkg, synth):
    c = cu.case()
    words = synth.pack_2bit(c["codes"])
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"filter": g.complexity_reads(words, c["offs"], c["params"]), "trim": g.complexity_reads(words, c["offs"], dict(c["params"], **TRIM))}


def strides_complexity(reached):
    lens = np.diff(cu.case()["offs"].astype(np.int64))
    assert_strides("complexity", lens, lens == 0, 1, 4, reached)


def run_quality(pkg, synth):
    c = qu.case()
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"quality": g.quality_reads(c["quals"], c["offs"], c["params"])}


def strides_quality(reached):
    lens = np.diff(qu.case()["offs"].astype(np.int64))
    assert_strides("quality", lens, lens == 0, 1, 4, reached)


SCREEN_K = 21


@functools.lru_cache(maxsize=None)
def screen_case():
    """four draws of su.read_case(21) against the one set of su.set_case(21), 228 reads, in an order drawn once: a draw alone has 57
    reads in ascending length, three of each"""
    draws = [su.read_case(SCREEN_K)] + [su.read_case(SCREEN_K, seed) for seed in (3021, 4021, 5021)]
    reads = [r for d in draws for r in d["reads"]]
    facts = [f for d in draws for f in d["facts"]]
    order = np.random.default_rng(57).permutation(len(reads)).tolist()
    codes, offs = su.concat([reads[i] for i in order])
    return dict(codes=codes, offs=offs, facts=[facts[i] for i in order])


def screen_settings():
    return (("single", False, su.params()), ("paired", True, su.params()), ("keep matched", False, su.params(flags=su.KEEP_MATCHED)))


def run_screen(pkg, synth):
    c = screen_case()
    words = synth.pack_2bit(c["codes"])
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        loaded = load_case(g, synth, SCREEN_K)                 # (k_screen_build in one workgroup)
        out = {"set": (loaded, g.screen_lookup(lookup_queries(SCREEN_K)[0]))}
        for name, paired, p in screen_settings():
            out[name] = g.screen_reads(words, c["offs"], paired=paired, params=p)
    return out


@functools.lru_cache(maxsize=None)
def want_screen():
    c, d = screen_case(), su.set_dict(SCREEN_K)
    out = {"set": (len(d), lookup_queries(SCREEN_K)[1])}
    for name, paired, p in screen_settings():
        out[name] = su.expect_screen(c["codes"], c["offs"], SCREEN_K, d, p, paired=paired, facts=c["facts"])
        assert 0 < out[name][2] < len(c["facts"])
    return out


def check_screen(pkg, got, want, what):
    if len(want) == 2:                                      # the set: the k-mers loaded, the reference of every query
        assert got[0] == want[0] and got[1].dtype == want[1].dtype and got[1].tolist() == want[1].tolist(), f"{what}: the set differs"
    else:
        assert_screen(pkg, got, want, what)


def strides_screen(reached):
    lens = np.diff(screen_case()["offs"].astype(np.int64))
    assert_strides("screen", lens, lens < SCREEN_K, 1, 4, reached)
    assert_strides("screen paired", lens, lens < SCREEN_K, 2, 4, reached)
    n = len(lookup_queries(SCREEN_K)[0])
    assert n >= 8 * 256 and su.SET_POSITIONS >= 8 * 256
    reached["screen_lookup, 256 lanes"] = n // 256


# ---- the compactions (a lane per read and per word: SDT_SCAN_BLOCKS) -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compact_case():
    """the input of test_compactions_at_offsets_past_2_32: length_mix() forty times over, every third read dropped / the random ranges
    of the trim's own test"""
    codes0, offs0 = length_mix()
    n0 = len(offs0) - 1
    codes, offs = trc.concat([codes0[int(offs0[r]):int(offs0[r + 1])] for _ in range(40) for r in range(n0)])
    keep = (np.arange(len(offs) - 1) % 3 != 1).astype(np.uint8)
    return dict(words=rs.pack_words(codes), offs=offs, keep=keep, trim=np.tile(range_sets(offs0)["random ranges"], 40))


def run_compact(pkg, synth):
    c = compact_case()
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        return {"reads": g.compact_reads(c["words"], c["offs"], c["keep"]), "trimmed": g.compact_trimmed(c["words"], c["offs"], c["trim"])}


@functools.lru_cache(maxsize=None)
def want_compact():
    c = compact_case()
    return {"reads": rs.expect_compact(c["words"], c["offs"], c["keep"]), "trimmed": rt.expect_compact_trimmed(c["words"], c["offs"], c["trim"])}


def check_compact(pkg, got, want, what):
    (ow, oo), (ww, wo) = got, want
    assert ow.dtype == np.uint32 and oo.dtype == np.uint64
    assert oo.tolist() == np.asarray(wo).tolist(), f"{what}: offsets differ"
    assert ow.tolist() == np.asarray(ww).tolist(), f"{what}: words differ"


def strides_compact(reached):
    c = compact_case()
    n, nw = len(c["offs"]) - 1, len(want_compact()["reads"][0])
    # (1 960 reads for 256 lanes: every lane takes 7 reads at least, and 2 words at least)
    assert n >= 7 * 256 and nw >= 2 * 256 and len(want_compact()["trimmed"][0]) >= 2 * 256
    reached["compact, 256 lanes: reads"] = n // 256
    reached["compact, 256 lanes: words"] = nw // 256


# ---- align_reads: a wavefront per read over the contig index ------------------------------------------------------------------------------
ALIGN_LEN = 32


@functools.lru_cache(maxsize=None)
def align_case():
    """the first of the small map cases whose reads are ragged (the very first has reads of 100 bases only: no read is shorter than the
    one a wavefront took before it, and none is skipped)"""
    import map_util as mu
    for name in mu.case_names():
        info = mu.load_case(name)
        codes, offs = mu.case_reads(info)[:2]
        if len(set(np.diff(offs.astype(np.int64)).tolist())) > 1:
            return dict(info=info, codes=codes, offs=offs, K=mu.case_contigs(info)[0])
    raise AssertionError("no map case with ragged reads")


def align_per_read(nh, best_foot, hits):
    """per read: the hit count; best hit, footprint flag, overflow flag; and the hits of all reads in order, as (contig, offset, read
    offset, k-mers, strand)"""
    return (np.array(nh, dtype=np.int64), np.array(best_foot, dtype=np.int64).reshape(-1, 3), np.array(hits, dtype=np.int64).reshape(-1, 5))


def run_align(pkg, synth):
    from test_gpu_parity import _index_case
    c = align_case()
    n = len(c["offs"]) - 1
    with pkg.PregraphGPU(c["K"], est_distinct=1 << 12, flags=pkg.SDT_FLAG_CONTIG_INDEX) as g:
        _index_case(pkg, synth, c["info"], g)
        g.finish_count()
        info_w, hits = g.align_reads(synth.pack_2bit(c["codes"]), c["offs"], align_len_all=ALIGN_LEN)
    nh_all, bf, flat = [], [], []
    for r in range(n):
        w = int(info_w[r])
        start, nh = w & ((1 << 40) - 1), (w >> 40) & 255
        nh_all.append(nh)
        bf.append(((w >> 48) & 255, (w >> 56) & 1, (w >> 57) & 1))
        assert nh or w == 0
        for h in ([hits[r]] + list(hits[start:start + nh - 1]) if nh else []):     # hit 0 sits at hits[read], the rest in the tail
            flat.append((int(h[0]), int(np.int32(h[1])), int(h[2]), int(h[3]) & 0x7FFFFFFF, int(h[3]) >> 31))
    return {"align": align_per_read(nh_all, bf, flat)}


@functools.lru_cache(maxsize=None)
def want_align():
    import map_util as mu
    c = align_case()
    o = mu.build_oracle(c["info"])
    assert o.K == c["K"]
    nh_all, bf, flat = [], [], []
    for r in range(len(c["offs"]) - 1):
        n, hits, best, foot = o.map_read(c["codes"][int(c["offs"][r]):int(c["offs"][r + 1])], ALIGN_LEN)
        assert n >= 0
        nh_all.append(n)
        bf.append((best, foot, 0) if n else (0, 0, 0))
        flat += [(ctg, off, roff, km, 1 if strand == "-" else 0) for ctg, off, roff, km, strand in (hits if n else [])]
    assert sum(1 for x in nh_all if x) > len(nh_all) // 2 and max(nh_all) > 1
    return {"align": align_per_read(nh_all, bf, flat)}


def check_align(pkg, got, want, what):
    for name, a, b in zip(("hit counts", "best hit / footprint / overflow", "hits"), got, want):
        assert a.shape == b.shape, f"{what}: {name}: {a.shape}, expected {b.shape}"
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differ at {bad[:8].tolist()}: got {a[bad[:4]].tolist()} want {b[bad[:4]].tolist()}"


def strides_align(reached):
    c = align_case()
    lens = np.diff(c["offs"].astype(np.int64))
    assert (int(lens.max()) - c["K"] + 1 + 2 * 20) * 8 * 4 <= 48 * 1024       # (launch_align: 4 wavefronts per workgroup at this length)
    assert_strides("align", lens, lens < c["K"] + 1, 1, 4, reached)


# ---- the kept forms: the kernels once more, over the batches kept in HBM ---------------------------------------------------------------
KEPT_BASE, KEPT_PAIRS = 3, 110


def kept_layout(pairs, singles):
    """the layout of the stages' kept-reads tests, which is the host program's: the read-1 file as one kept batch (ordinals base,
    base + 2, ...), the read-2 file as another (base + 1, base + 3, ...; one read short, so the last pair has one mate), single reads
    behind the pair range; no read has ordinals 0 .. 2.  Here with 110 pairs and 111 + 110 + len(singles) reads"""
    assert len(pairs) > KEPT_PAIRS
    r1 = [a for a, _ in pairs[:KEPT_PAIRS]] + [pairs[KEPT_PAIRS][0]]
    r2 = [b for _, b in pairs[:KEPT_PAIRS]]
    first, end = KEPT_BASE, KEPT_BASE + 2 * (KEPT_PAIRS + 1)
    ords = [KEPT_BASE + 2 * t for t in range(KEPT_PAIRS + 1)] + [KEPT_BASE + 1 + 2 * t for t in range(KEPT_PAIRS)] + [end + i for i in range(len(singles))]
    codes, offs = rd.concat(r1 + r2 + list(singles))
    total = end + len(singles)
    present = np.zeros(total, dtype=bool)
    present[ords] = True
    assert (~present).sum() == 4
    return dict(batches=((r1, KEPT_BASE, 2), (r2, KEPT_BASE + 1, 2), (list(singles), end, 1)), ords=ords, ranges=[(first, end)], total=total,
                present=present, codes=codes, offs=offs, lens=[np.array([len(r) for r in b], dtype=np.int64) for b in (r1, r2, singles)])


def keep_layout(g, synth, lay):
    for batch, b, stride in lay["batches"]:
        g.set_read_ordinal(b, stride)
        bc, bo = rd.concat(batch)
        g.keep_reads(synth.pack_2bit(bc), bo)


@functools.lru_cache(maxsize=None)
def kept_layouts():
    sc = screen_case()
    sreads = [sc["codes"][int(sc["offs"][i]):int(sc["offs"][i + 1])] for i in range(len(sc["offs"]) - 1)]
    cx = cu.case()["reads"]
    ov = overlap_case()["pairs"]
    return dict(dedup=kept_layout(dedup_paired_case()["pairs"], rd.case()["reads"]),
                overlap=kept_layout(ov, list(ov[KEPT_PAIRS + 1]) + list(ov[KEPT_PAIRS + 2])),
                complexity=kept_layout([(cx[t], cx[(t + 20) % len(cx)]) for t in range(KEPT_PAIRS + 1)], cx),      # (the empty read in both files)
                screen=kept_layout([(sreads[2 * t], sreads[2 * t + 1]) for t in range(KEPT_PAIRS + 1)], sreads))


def run_kept(pkg, synth):
    lays = kept_layouts()
    out = {}
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        lay = lays["dedup"]
        keep_layout(g, synth, lay)
        for flags in (0, rd.MATE_SWAP):
            dup, n, kept = g.dedup_kept_reads(lay["total"], lay["ranges"], flags=flags)
            out[f"dedup flags={flags}"] = (dup[lay["present"]], n, kept)
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        lay = lays["overlap"]
        keep_layout(g, synth, lay)
        ov, n, kept = g.overlap_kept_pairs(lay["total"], lay["ranges"], overlap_case()["params"])
        out["overlap"] = (ov[lay["present"]], n, kept)
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        lay = lays["complexity"]
        keep_layout(g, synth, lay)
        for name, prm in (("filter", cu.case()["params"]), ("trim", dict(cu.case()["params"], **TRIM))):
            cx, n, kept = g.complexity_kept_reads(lay["total"], prm)
            out[f"complexity {name}"] = (cx[lay["present"]], n, kept)
    with pkg.PregraphGPU(31, est_distinct=1 << 12) as g:
        lay = lays["screen"]
        load_case(g, synth, SCREEN_K)
        keep_layout(g, synth, lay)
        for flags in (0, su.KEEP_MATCHED):
            rec, n, kept = g.screen_kept_reads(lay["total"], lay["ranges"], params=su.params(flags=flags))
            out[f"screen flags={flags}"] = (rec[lay["present"]], n, kept)
    return out


@functools.lru_cache(maxsize=None)
def want_kept():
    lays = kept_layouts()
    out = {}
    by_ordinal = lambda lay, rec: np.concatenate([rec, np.zeros(lay["total"] - len(rec), dtype=rec.dtype)])[lay["present"]]
    lay = lays["dedup"]
    for flags in (0, rd.MATE_SWAP):
        dup, _, kept = rd.expect_dedup(lay["codes"], lay["offs"], flags=flags, ordinals=lay["ords"], units=rs.ranged_units(lay["ords"], lay["ranges"]))
        out[f"dedup flags={flags}"] = (by_ordinal(lay, dup), len(lay["ords"]), kept)
    assert out["dedup flags=0"][2] > out[f"dedup flags={rd.MATE_SWAP}"][2] > 0
    lay = lays["overlap"]
    ov, _, kept = ru.expect_overlap(lay["codes"], lay["offs"], overlap_case()["params"], pair_ranges=lay["ranges"], ordinals=lay["ords"])
    assert (ov["insert"] > 0).sum() >= 40 and {ru.WHOLE, ru.CLIPPED, ru.DROPPED} == set(by_ordinal(lay, ov)["verdict"].tolist())
    out["overlap"] = (by_ordinal(lay, ov), len(lay["ords"]), kept)
    lay = lays["complexity"]
    for name, prm in (("filter", cu.case()["params"]), ("trim", dict(cu.case()["params"], **TRIM))):
        cx, _, kept = cu.expect_complexity(lay["codes"], lay["offs"], prm, ordinals=lay["ords"])
        out[f"complexity {name}"] = (by_ordinal(lay, cx), len(lay["ords"]), kept)
    lay = lays["screen"]
    d = su.set_dict(SCREEN_K)
    facts = su.all_facts(lay["codes"], lay["offs"], SCREEN_K, d)
    by_ord = {o: i for i, o in enumerate(lay["ords"])}
    units = [[by_ord[o] for o in u] for u in su.ranged_units(lay["ords"], lay["ranges"])]
    for flags in (0, su.KEEP_MATCHED):
        rec, _, kept = su.verdicts(facts, np.diff(lay["offs"].astype(np.int64)).tolist(), su.params(flags=flags), units)
        placed = np.zeros(lay["total"], dtype=su.DTYPE)
        placed[lay["ords"]] = rec
        assert 0 < kept < len(lay["ords"])
        out[f"screen flags={flags}"] = (placed[lay["present"]], len(lay["ords"]), kept)
    return out


def check_kept(pkg, got, want, what):
    stage = what.split()[1].rstrip(",")                     # (what: "kept <stage> ...")
    dtype, same = {"dedup": (pkg.READ_DUP_DTYPE, rd.assert_dup_equal), "overlap": (pkg.READ_OVERLAP_DTYPE, ru.assert_overlap_equal),
                   "complexity": (pkg.READ_COMPLEXITY_DTYPE, cu.assert_cx_equal), "screen": (pkg.READ_SCREEN_DTYPE, su.assert_records_equal)}[stage]
    assert got[0].dtype == dtype
    same(got[0], want[0], what)
    assert got[1:] == want[1:], f"{what}: (reads, reads kept) = {got[1:]}, expected {want[1:]}"


def strides_kept(reached):
    """every kept batch is a launch of its own: the conditions hold for each of the three batches of a layout"""
    lays = kept_layouts()
    for stage, skip in (("dedup", lambda l: l == 0), ("complexity", lambda l: l == 0), ("screen", lambda l: l < SCREEN_K)):
        r1, r2, singles = lays[stage]["lens"]
        for name, lens in (("the read-1 batch", r1), ("the read-2 batch", r2), ("the single reads", singles)):
            assert_strides(f"{stage} kept, {name}", lens, skip(lens), 1, 4, reached)
    # the pairs of the overlap are units across the two batches
    r1, r2, _ = lays["overlap"]["lens"]
    lens = np.stack([r1[:KEPT_PAIRS], r2]).T.reshape(-1)
    short = lens < overlap_case()["params"]["min_overlap"]
    assert_strides("overlap kept", lens, np.repeat(short[0::2] | short[1::2], 2), 2, 4, reached)


# ---- the stages ------------------------------------------------------------------------------------------------------------------------------
RUNS = dict(search=run_search, profile=run_profile, correct=run_correct, select=run_select, trim=run_trim, dedup=run_dedup, clip=run_clip,
            overlap=run_overlap, complexity=run_complexity, quality=run_quality, screen=run_screen, compact=run_compact, align=run_align, kept=run_kept)
# stage -> (the restatement of every run, the stage's comparison, the conditions on its input)
STAGES = dict(
    search=(want_search, check_search, strides_search),
    profile=(want_profile, check_profile, strides_profile),
    correct=(want_correct, check_correct, strides_correct),
    select=(want_select, check_select, strides_select),
    trim=(want_trim, check_trim, strides_trim),
    dedup=(want_dedup, assert_dedup, strides_dedup),
    clip=(lambda: {"clip": rcl.case_expect()}, assert_clip, strides_clip),
    overlap=(want_overlap, assert_overlap, strides_overlap),
    complexity=(lambda: {"filter": cu.case_expect(), "trim": cu.case_expect(trim=True)}, assert_cx, strides_complexity),
    quality=(lambda: {"quality": qu.case_expect()}, assert_q, strides_quality),
    screen=(want_screen, check_screen, strides_screen),
    compact=(want_compact, check_compact, strides_compact),
    align=(want_align, check_align, strides_align),
    kept=(want_kept, check_kept, strides_kept),
)
assert set(RUNS) == set(STAGES)

CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from soapdenovo_trans_amd import synth
import test_read_stage_strides as me
np.savez({path!r}, **me.flatten(me.RUNS[{stage!r}](pkg, synth)))
"""

_unhooked = {}


def run_child(tmp_path, stage, blocks):
    path = str(tmp_path / f"{stage}.npz")
    env = dict(os.environ, SDT_TEST_HOOKS="1", SDT_SCAN_BLOCKS="1", SDT_WAVE_BLOCKS=str(blocks))
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path, stage=stage)], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return unflatten(np.load(path))


def test_the_file_form_keeps_the_outputs(tmp_path):
    """CPU: what a child saves is what the parent loads -- records keep their fields, counts and error codes their value"""
    runs = {"K=31 a|b": (np.arange(12, dtype=np.uint32).view(su.DTYPE), np.zeros(0, dtype=np.uint8), 7), "z": (np.full(1, 3, dtype=np.uint64), EINVAL)}
    np.savez(str(tmp_path / "runs.npz"), **flatten(runs))
    back = unflatten(np.load(str(tmp_path / "runs.npz")))
    assert set(back) == set(runs)
    for name, outs in runs.items():
        assert len(back[name]) == len(outs)
        for x, y in zip(back[name], outs):
            assert (x.dtype == y.dtype and x.tolist() == y.tolist()) if isinstance(y, np.ndarray) else (type(x) is int and x == y)


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_inputs_hold_the_stride_conditions(synth, stage):
    """CPU: the conditions depend on the inputs alone (synth: the cases draw their reads from the package's generator)"""
    reached = {}
    STAGES[stage][2](reached)
    assert reached and min(reached.values()) >= 2, reached
    print(reached)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", WAVE_BLOCKS)
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_strides(pkg, synth, tmp_path, stage, blocks):
    """the stage's runs in SDT_WAVE_BLOCKS = `blocks` workgroups of wavefronts and one workgroup of lanes, against the restatement and
    against the run without the hooks"""
    assert "SDT_WAVE_BLOCKS" not in os.environ and "SDT_SCAN_BLOCKS" not in os.environ and pkg.SDT_EINVAL == EINVAL
    want_of, check, strides = STAGES[stage]
    reached = {}
    strides(reached)                                        # the input can show what the test is about
    print(f"{stage}: items per wavefront / lane: {reached}")
    want = want_of()
    hooked = run_child(tmp_path, stage, blocks)
    if stage not in _unhooked:
        _unhooked[stage] = RUNS[stage](pkg, synth)
    plain = _unhooked[stage]
    assert set(hooked) == set(want) == set(plain), (sorted(hooked), sorted(want), sorted(plain))
    for run in sorted(want):
        check(pkg, hooked[run], want[run], f"{stage} {run}, {blocks} workgroups, against the restatement")
        check(pkg, plain[run], want[run], f"{stage} {run}, no hooks, against the restatement")
        check(pkg, hooked[run], plain[run], f"{stage} {run}, {blocks} workgroups, against the run without the hooks")
