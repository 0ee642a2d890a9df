"""GPU (-m gpu): `sdt-kmers complexity` on a library of single reads and a library of a pair of files made of the reads of the case,
against the numpy restatement of the rule and of the four files (read_complexity_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_complexity_util as cu
from test_read_dedup_cli import write_fastq

pytestmark = pytest.mark.gpu

K = 31


def library(tmp_path, with_pairs=True):
    """the reads of the case that have 40 .. 250 bases, in the case's order: 35 single reads (q=, the smaller avg_ins: streamed first,
    so the pairs start at an odd ordinal) and 35 pairs (q1= / q2=); returns the config, the stream in ordinal order and the pair
    ranges.  Without pairs: the single reads alone"""
    c = cu.case()
    pool = [r for r in c["reads"] if 40 <= len(r) <= 250]
    assert len(pool) >= 105
    singles, r1, r2 = pool[:35], pool[35:70], pool[70:105]
    write_fastq(tmp_path / "s.fq", singles, "")
    text = f"max_rd_len=250\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
    if with_pairs:
        write_fastq(tmp_path / "p_1.fq", r1, "/1")
        write_fastq(tmp_path / "p_2.fq", r2, "/2")
        text += f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n"
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(text)
    if not with_pairs:
        return str(cfg), singles, []
    return str(cfg), singles + [r for pair in zip(r1, r2) for r in pair], [(len(singles), len(singles) + 2 * len(r1))]


def run_and_compare(pkg, tmp_path, cfg, stream, ranges, p, options):
    codes, offs = cu.concat(stream)
    cx = cu.expect_complexity(codes, offs, p)[0]
    texts = cu.cli_texts(codes, offs, cx, ranges)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "complexity", "-s", cfg, "-K", str(K), "-p", "4", *options, "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in zip(("readComplexity", "cx.pairs.fa", "cx.single.fa", "scoreHist"), texts):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    last = [x for x in r.stdout.splitlines() if "with a low window" in x]
    v = cx["verdict"]
    assert len(last) == 1 and [int(x) for x in last[0].replace(";", "").replace(",", "").replace(":", "").split() if x.isdigit()] == [
        len(stream), int((cx["low"] > 0).sum()), int((v == 2).sum()), int((v == 3).sum()), int(offs[-1]), int(cx["len"].sum())]
    return cx, texts


def test_sdt_kmers_complexity_cli(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path)
    cx, (rec_txt, pairs_txt, single_txt, hist_txt) = run_and_compare(pkg, tmp_path, cfg, stream, ranges, cu.params(min_len=20), ("--min-len", "20"))
    first, end = ranges[0]
    live = cx["len"] > 0
    npairs = (end - first) // 2
    lost_one = [t for t in range(npairs) if live[first + 2 * t] != live[first + 2 * t + 1]]
    lost_both = [t for t in range(npairs) if not live[first + 2 * t] and not live[first + 2 * t + 1]]
    assert first & 1 and len(lost_one) >= 5 and lost_both and {cu.WHOLE, cu.DROPPED} == set(cx["verdict"].tolist())
    # pairs are in the pairs file only when both mates survive, next to each other; the survivor of a broken pair is a single read
    names = [int(x[1:]) - 1 for x in pairs_txt.splitlines()[0::2]]
    assert names and all(first <= a < end and b == a + 1 and live[a] and live[b] for a, b in zip(names[0::2], names[1::2]))
    assert all((a - first) % 2 == 0 for a in names[0::2]) and len(names) == 2 * sum(bool(live[first + 2 * t] and live[first + 2 * t + 1]) for t in range(npairs))
    singles_out = {int(x[1:]) - 1 for x in single_txt.splitlines()[0::2]}
    assert {first + 2 * t + (0 if live[first + 2 * t] else 1) for t in lost_one} <= singles_out


def test_sdt_kmers_complexity_cli_trim_low(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path)
    cx, texts = run_and_compare(pkg, tmp_path, cfg, stream, ranges, cu.params(max_score_pct=9, max_low_pct=0, min_len=25, flags=cu.TRIM),
                                ("--trim-low", "--max-score", "9", "--min-len", "25"))
    assert {cu.WHOLE, cu.CLIPPED, cu.DROPPED} == set(cx["verdict"].tolist()) and (cx["start"] > 0).sum() >= 5
    assert texts[3].splitlines()[-1].endswith(f"clipped {int((cx['verdict'] == cu.CLIPPED).sum())}")


def test_sdt_kmers_complexity_cli_without_pairs(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path, with_pairs=False)
    cx, texts = run_and_compare(pkg, tmp_path, cfg, stream, ranges, cu.params(max_low_pct=30), ("--max-low", "30"))
    assert texts[1] == "" and texts[2].count(">") == int((cx["len"] > 0).sum()) and (cx["verdict"] == cu.DROPPED).any()
