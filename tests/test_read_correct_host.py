"""CPU: the read-correction entry points exist at every layer (header, library, binding, host program), and the Python restatement
of the rule (read_correct_util.py) -- what the GPU tests expect -- does what a corrector should, on its own, against a
collections.Counter: planted substitutions come back, and hardly anything else changes."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import read_correct_util as rc
from test_kmer_search import canon_kmers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_correct_reads", "sdt_gpu_correct_reads_device", "sdt_gpu_correct_kept_reads", "sdt_gpu_kept_batches",
           "sdt_gpu_fetch_kept_batch"]


def test_header_declares_and_library_exports_the_five_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+kmers,\s*weak,\s*runs,\s*fixed;\s*\}\s*sdt_read_fix;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_fix_dtype_is_the_c_struct(pkg):
    dt = pkg.READ_FIX_DTYPE
    assert dt.itemsize == 16
    assert dt.names == ("kmers", "weak", "runs", "fixed") == rc.FIX_FIELDS
    assert all(dt.fields[n][0] == np.uint32 and dt.fields[n][1] == 4 * i for i, n in enumerate(dt.names))
    for m in ("correct_reads", "correct_reads_device", "correct_kept_reads", "kept_batches", "fetch_kept_batch"):
        assert callable(getattr(pkg.PregraphGPU, m))


def test_make_builds_sdt_kmers_and_its_usage_names_correct(pkg):
    subprocess.run(["make", "-C", pkg.CSRC_DIR], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    assert os.path.exists(exe), "make -C csrc does not build sdt-kmers"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "usage" in r.stderr and "correct" in r.stderr and "profile" in r.stderr and "query" in r.stderr
    assert "readFix" in r.stderr and "edits" in r.stderr and "corrected.fa" in r.stderr
    r = subprocess.run([exe, "correct", "-s", "x.cfg", "-K", "31"], capture_output=True, text=True)      # no -o
    assert r.returncode != 0 and "usage" in r.stderr


# ---- the rule itself -------------------------------------------------------------------------------------------------------------
def test_runs_and_candidates_by_hand():
    assert rc.runs_of([False, True, True, False, True]) == [(1, 2), (4, 4)]
    assert rc.runs_of([True] * 3) == [(0, 2)] and rc.runs_of([False] * 3) == []
    K, n = 5, 20
    assert rc.candidate_base(0, n - 1, n, K) is None                     # nothing solid
    assert rc.candidate_base(3, 7, n, K) == 7                            # interior, l == K
    assert rc.candidate_base(3, 6, n, K) is None and rc.candidate_base(3, 8, n, K) is None
    assert rc.candidate_base(0, 2, n, K) == 2 and rc.candidate_base(0, 4, n, K) == 4 and rc.candidate_base(0, 5, n, K) is None
    assert rc.candidate_base(17, 19, n, K) == 21 and rc.candidate_base(15, 19, n, K) == 19 and rc.candidate_base(14, 19, n, K) is None
    # one read, one error, a table that holds the clean read three times: the error comes back, whichever base it is in
    rng = np.random.default_rng(4)
    clean = rng.integers(0, 4, size=40, dtype=np.uint8)
    table = collections.Counter({k: 3 for k in canon_kmers(clean, 11)})
    for p in range(40):
        bad = clean.copy()
        bad[p] ^= 1
        rec, subs = rc.correct_read(bad, 11, rc.table_counts(table), 3)
        assert subs == [(p, int(clean[p]))] and rec == (30, min(p, 29) - max(p - 10, 0) + 1, 1, 1), (p, rec, subs)
        assert rc.correct_read(bad, 11, rc.table_counts(table), 0) == ((30, 0, 0, 0), [])
    assert rc.correct_read(clean[:10], 11, rc.table_counts(table), 3) == ((0, 0, 0, 0), [])
    assert rc.correct_read(clean, 11, rc.table_counts(table), 4) == ((30, 30, 1, 0), [])


def boundary_positions(K, L):
    return [0, 1, K - 2, K - 1, K, K + 1, L - K - 2, L - K - 1, L - K, L - K + 1, L - 2, L - 1]


@pytest.mark.parametrize("K,L", [(21, 150), (31, 150), (63, 250)])
def test_the_rule_restores_planted_substitutions(synth, K, L):
    """clean fixed-length reads of 25 transcripts, one substitution planted in each of 1 600 of them at the boundary positions in
    rotation (a further 100 + 100 get two, K + 3 and K - 5 apart); the table is a Counter of the k-mers of all reads as planted;
    min_count 3.  Of the planted reads whose clean copy is entirely solid >= 95 % come back clean, <= 1 % come back changed and wrong"""
    tx = synth.make_transcriptome(25, seed=K)
    codes, offs = synth.sample_reads(*tx, n_reads=6000, read_len=L, seed=K + 1, err=0.0)
    offs = offs.astype(np.int64)
    assert (np.diff(offs) == L).all()
    clean = codes.copy()
    pos = boundary_positions(K, L)
    for r in range(1600):
        p = offs[r] + pos[r % len(pos)]
        codes[p] = (codes[p] + 1 + r % 3) & 3
    p1 = K + 7
    for r in range(1600, 1800):
        for p in (p1, p1 + (K + 3 if r < 1700 else K - 5)):
            codes[offs[r] + p] = (codes[offs[r] + p] + 1 + r % 3) & 3
    table = collections.Counter()
    for r in range(len(offs) - 1):
        table.update(canon_kmers(codes[offs[r]:offs[r + 1]], K))
    count = rc.table_counts(table)
    mc = 3

    def outcome(r):
        good = clean[offs[r]:offs[r + 1]]
        if not all(count(k) >= mc for k in canon_kmers(good, K)):
            return None
        read = codes[offs[r]:offs[r + 1]].copy()
        rec, subs = rc.correct_read(read, K, count, mc)
        assert rec[0] == L - K + 1 and rec[3] == len(subs)
        for p, x in subs:
            assert read[p] != x
            read[p] = x
        return "restored" if (read == good).all() else ("unchanged" if not subs else "wrong")

    one = collections.Counter(outcome(r) for r in range(1600))
    solid = 1600 - one[None]
    print(f"K={K}: restored {one['restored']} / {solid}, changed but wrong {one['wrong']}, left alone {one['unchanged']}")
    assert solid >= 1000, "too few planted reads have an entirely solid clean copy for the test to mean anything"
    assert one["restored"] >= 0.95 * solid
    assert one["wrong"] <= 0.01 * solid
    far = collections.Counter(outcome(r) for r in range(1600, 1700))
    near = collections.Counter(outcome(r) for r in range(1700, 1800))
    print(f"K={K}: two errors K + 3 apart: {dict(far)}; K - 5 apart: {dict(near)}")
    assert far["restored"] > (100 - far[None]) / 2 and 100 - far[None] >= 50        # two interior runs of K k-mers: both come back
    assert near["unchanged"] > (100 - near[None]) / 2 and 100 - near[None] >= 50    # one run of 2K - 5 k-mers: no candidate
    # clean reads stay clean: nothing is weak in a read whose k-mers are all solid
    for r in range(1800, 2000):
        if all(count(k) >= mc for k in canon_kmers(clean[offs[r]:offs[r + 1]], K)):
            assert rc.correct_read(codes[offs[r]:offs[r + 1]], K, count, mc) == ((L - K + 1, 0, 0, 0), [])
