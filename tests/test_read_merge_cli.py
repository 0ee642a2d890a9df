"""GPU (-m gpu): `sdt-kmers merge` on a FASTQ library (single reads, a pair of files with planted fragments, an interleaved p= file), on
a FASTA library of a pair of files with mismatching mates, and on a library without pairs, against the Python restatements of the
overlap rule, of the merge rule and of the five files (read_overlap_util.py, read_merge_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_merge_util as mu
import read_overlap_util as ro
from read_select_util import LETTERS
from test_read_overlap_cli import library

pytestmark = pytest.mark.gpu

K = 31
FILES = ("readMerge", "merge.fa", "merge.pairs.fa", "merge.single.fa", "insertHist")


def expected(stream, ranges, op, mp):
    """-> (the five texts, the summary line, the overlap records, the merge records, the merged reads)"""
    codes, offs = ro.concat(stream)
    n = len(stream)
    ov = ro.expect_overlap(codes, offs, op, pair_ranges=ranges, ordinals=range(n))[0]
    mg, merged = mu.expect_merge(codes, offs, ov, mp, pair_ranges=ranges, ordinals=range(n))
    texts = mu.cli_texts(codes, offs, ov, mg, merged, ranges)
    return texts[:5], texts[5], ov, mg, merged


def run_and_compare(pkg, tmp_path, cfg, prefix, options, want):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "merge", "-s", cfg, "-K", str(K), "-p", "4", *options, "-o", str(tmp_path / prefix)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    texts, summary = want[:2]
    for ext, text in zip(FILES, texts):
        got = (tmp_path / f"{prefix}.{ext}").read_text()
        assert got == text, f"{prefix}.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    assert [x for x in r.stdout.splitlines() if x.startswith("merge:")] == [summary]
    return r


def test_sdt_kmers_merge_fastq_library(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path)
    op, mp = ro.params(min_overlap=25, max_err_pct=5, min_len=40), mu.params(min_len=45, max_len=150)
    want = expected(stream, ranges, op, mp)
    ov, mg, merged = want[2:]
    first, end = ranges[0]
    inserts = ov["insert"][first:end:2]
    # some pairs merge, some overlap and are kept apart by either limit, some do not overlap; nothing outside the pair range merges
    assert len(merged) >= 10 and (inserts > 150).sum() >= 2 and ((inserts > 0) & (inserts < 45)).sum() >= 1 and (inserts == 0).sum() >= 8
    assert not mg["merged"][:first].any() and not mg["merged"][end:].any() and first & 1
    run_and_compare(pkg, tmp_path, cfg, "out", ("--min-overlap", "25", "--max-err", "5", "--min-len", "40", "--min-merged", "45", "--max-merged", "150"), want)
    # a merged pair is in the merged file under its first mate's number and in no other file
    names = [int(x[1:]) - 1 for x in want[0][1].splitlines()[0::2]]
    assert names == [r for r in range(first, end, 2) if mg["merged"][r]]
    others = {int(x[1:]) - 1 for t in want[0][2:4] for x in t.splitlines()[0::2]}
    assert not others & set(names) and not others & {r + 1 for r in names}
    # the defaults
    run_and_compare(pkg, tmp_path, cfg, "dflt", (), expected(stream, ranges, ro.params(), mu.params()))


def test_sdt_kmers_merge_fasta_library_and_without_pairs(pkg, tmp_path):
    """f1= / f2= files whose mates differ in their overlap: without qualities the base of mate 1 stays; a fragment longer than a block of
    the walk's buffer is not needed for that.  And a library without pairs: nothing merges, every file but the merged one is overlap's"""
    rng = np.random.default_rng(34)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    pairs = []
    for i in range(30):
        F = int(rng.integers(50, 190))
        frag = rnd(F)
        a = np.concatenate([frag, rnd(max(100 - F, 0))])[:100].astype(np.uint8)
        b = np.concatenate([ro.revcomp(frag), rnd(max(100 - F, 0))])[:100].astype(np.uint8)
        if i % 3 == 0 and F < 170:                                         # one or two mismatch columns
            for q in (3, 17)[: 1 + i % 2]:
                b[q] = (b[q] + 1) & 3
        pairs.append((a, b) if i % 5 else (rnd(100), rnd(90)))
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    for m in (0, 1):
        (tmp_path / f"f_{m + 1}.fa").write_bytes(b"".join(b">r%d/%d\n%s\n" % (i, m + 1, letters[pr[m]].tobytes()) for i, pr in enumerate(pairs)))
    cfg = tmp_path / "fa.cfg"
    cfg.write_text(f"max_rd_len=100\n[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nf1={tmp_path / 'f_1.fa'}\nf2={tmp_path / 'f_2.fa'}\n")
    stream = [r for pr in pairs for r in pr]
    want = expected(stream, [(0, len(stream))], ro.params(), mu.params())
    mg, merged = want[3:]
    assert len(merged) >= 12 and (mg["mismatches"] > 0).sum() >= 6 and not mg["from_b"].any()
    run_and_compare(pkg, tmp_path, str(cfg), "fa", (), want)
    # no pairs: the q= library of single reads alone
    scfg, sstream, sranges = library(tmp_path)
    singles = sstream[:sranges[0][0]]
    only = tmp_path / "single.cfg"
    only.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n")
    want = expected(singles, [], ro.params(), mu.params())
    assert want[0][1] == "" and want[0][4] == "# pairs 0 overlapping 0 clipped 0 median 0\n" and want[1].split()[2:10] == [str(len(singles)), "pairs", "0", "overlapping", "0", "merged", "0", "mismatch"]
    run_and_compare(pkg, tmp_path, str(only), "one", (), want)
    # wrong options exit non-zero and write nothing
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    for opts in (("--max-err", "101"), ("--min-merged", "x"), ("--phred", "33"), ("--mate-swap",)):
        r = subprocess.run([exe, "merge", "-s", scfg, "-K", str(K), *opts, "-o", str(tmp_path / "bad")], capture_output=True, text=True)
        assert r.returncode != 0 and opts[0] in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
