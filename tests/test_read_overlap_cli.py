"""GPU (-m gpu): `sdt-kmers overlap` on a library of single reads, a library of a pair of files with planted fragments and a library of
an interleaved p= file, against the Python restatement of the rule and of the four files (read_overlap_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_overlap_util as ru
from read_select_util import LETTERS
from test_read_dedup_cli import write_fastq

pytestmark = pytest.mark.gpu

K = 31


def library(tmp_path):
    """21 single reads of 50 .. 100 bases (q=, the smallest avg_ins: streamed first, so the pairs start at an odd ordinal), 40 pairs of
    up to 100 bases (q1= / q2=) and 12 reads of an interleaved FASTA file (p=, the largest avg_ins: streamed last, as single reads).  Of
    the pairs a quarter read through a fragment of 40 .. 90 bases into different adapters, a quarter meet in the middle of a fragment
    of 130 .. 165, a quarter have mates of 100 and 60 bases on a fragment of 80, a quarter are unrelated; pair 6 has a fragment of 32
    bases (both mates fall below --min-len), pair 10 a second mate of 33 bases (it alone does).  The p= file holds read-through pairs
    too: nothing is known about them.  Returns the config, the stream in ordinal order and the pair ranges"""
    rng = np.random.default_rng(33)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)

    def planted(F, La, Lb):
        frag = rnd(F)
        a = np.concatenate([frag, rnd(La - F)]) if La > F else frag[:La]
        b = np.concatenate([ru.revcomp(frag), rnd(Lb - F)]) if Lb > F else ru.revcomp(frag)[:Lb]
        return a.astype(np.uint8), b.astype(np.uint8)

    singles = [rnd(int(rng.integers(50, 101))) for _ in range(21)]
    pairs = []
    for i in range(40):
        kind = i % 4
        if kind == 0:
            pairs.append(planted(int(rng.integers(40, 91)), 100, 100))
        elif kind == 1:
            pairs.append(planted(int(rng.integers(130, 166)), 100, 100))
        elif kind == 2:
            pairs.append(planted(32, 100, 100) if i == 6 else (planted(50, 100, 33) if i == 10 else planted(80, 100, 60)))
        else:
            pairs.append((rnd(int(rng.integers(60, 101))), rnd(int(rng.integers(60, 101)))))
    inter = [r for _ in range(6) for r in planted(60, 100, 100)]
    write_fastq(tmp_path / "s.fq", singles, "")
    write_fastq(tmp_path / "p_1.fq", [a for a, _ in pairs], "/1")
    write_fastq(tmp_path / "p_2.fq", [b for _, b in pairs], "/2")
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    (tmp_path / "inter.fa").write_bytes(b"".join(b">i%d\n%s\n" % (i, letters[r].tobytes()) for i, r in enumerate(inter)))
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n"
                   f"[LIB]\navg_ins=300\nreverse_seq=0\nasm_flags=3\np={tmp_path / 'inter.fa'}\n")
    stream = singles + [r for pair in pairs for r in pair] + inter
    return str(cfg), stream, [(len(singles), len(singles) + 2 * len(pairs))]


def test_sdt_kmers_overlap_cli(pkg, tmp_path):
    cfg, stream, ranges = library(tmp_path)
    codes, offs = ru.concat(stream)
    n = len(stream)
    p = ru.params(min_overlap=25, max_err_pct=5, min_len=40)
    ov = ru.expect_overlap(codes, offs, p, pair_ranges=ranges, ordinals=range(n))[0]
    rec_txt, pairs_txt, single_txt, hist_txt = ru.cli_texts(codes, offs, ov, ranges)
    first, end = ranges[0]
    live = ov["len"] > 0
    assert first & 1 and not live[first + 12] and not live[first + 13] and live[first + 20] and not live[first + 21]
    assert {ru.WHOLE, ru.CLIPPED, ru.DROPPED} == set(ov["verdict"].tolist()) and (ov["insert"][first:end:2] > 0).sum() >= 25
    assert (ov["insert"][:first] == 0).all() and (ov["insert"][end:] == 0).all() and (ov["verdict"][end:] == ru.WHOLE).all()
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "overlap", "-s", cfg, "-K", str(K), "-p", "4", "--min-overlap", "25", "--max-err", "5", "--min-len", "40", "-o",
                        str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in (("readOverlap", rec_txt), ("overlap.pairs.fa", pairs_txt), ("overlap.single.fa", single_txt), ("insertHist", hist_txt)):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    # pairs are in the pairs file only when both mates survive, next to each other; the survivor of a broken pair is a single read
    names = [int(x[1:]) - 1 for x in pairs_txt.splitlines()[0::2]]
    assert names and all(first <= a < end and b == a + 1 and live[a] and live[b] for a, b in zip(names[0::2], names[1::2]))
    assert first + 20 in [int(x[1:]) - 1 for x in single_txt.splitlines()[0::2]]
    inserts = sorted(int(x) for x in ov["insert"][first:end:2] if x)
    assert hist_txt.splitlines()[-1].split()[:6] == ["#", "pairs", "40", "overlapping", str(len(inserts)), "clipped"]
    last = [x for x in r.stdout.splitlines() if "whole" in x]
    v = ov["verdict"]
    assert len(last) == 1 and [int(x) for x in last[0].replace(";", "").replace(",", "").replace(":", "").split() if x.isdigit()] == [
        n, int((v == 0).sum()), int((v == 2).sum()), int((v == 3).sum()), int(offs[-1]), int(ov["len"].sum()), 40, len(inserts),
        inserts[(len(inserts) - 1) // 2]]
    # the defaults: min_overlap 30, 10 %, no min_len
    r = subprocess.run([exe, "overlap", "-s", cfg, "-K", str(K), "-p", "4", "-o", str(tmp_path / "dflt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dflt = ru.expect_overlap(codes, offs, ru.params(), pair_ranges=ranges, ordinals=range(n))[0]
    for ext, text in zip(("readOverlap", "overlap.pairs.fa", "overlap.single.fa", "insertHist"), ru.cli_texts(codes, offs, dflt, ranges)):
        assert (tmp_path / f"dflt.{ext}").read_text() == text, f"dflt.{ext} differs from the rule"


def test_sdt_kmers_overlap_without_pairs_and_wrong_options(pkg, tmp_path):
    """a library without pairs is allowed: everything is whole, the histogram is its summary line; wrong options exit non-zero and write
    nothing"""
    cfg, stream, ranges = library(tmp_path)
    singles = stream[:ranges[0][0]]
    only = tmp_path / "single.cfg"
    only.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n")
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    r = subprocess.run([exe, "overlap", "-s", str(only), "-K", str(K), "-o", str(tmp_path / "one")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    codes, offs = ru.concat(singles)
    ov = ru.expect_overlap(codes, offs, ru.params(), pair_ranges=[], ordinals=range(len(singles)))[0]
    assert (ov["verdict"] == ru.WHOLE).all()
    for ext, text in zip(("readOverlap", "overlap.pairs.fa", "overlap.single.fa", "insertHist"), ru.cli_texts(codes, offs, ov, [])):
        assert (tmp_path / f"one.{ext}").read_text() == text, f"one.{ext} differs from the rule"
    assert (tmp_path / "one.insertHist").read_text() == "# pairs 0 overlapping 0 clipped 0 median 0\n"
    for opts in (("--max-err", "101"), ("--min-overlap", "0"), ("-a", str(tmp_path / "s.fq")), ("--error-pct", "10"), ("--mate-swap",)):
        r = subprocess.run([exe, "overlap", "-s", cfg, "-K", str(K), *opts, "-o", str(tmp_path / "bad")], capture_output=True, text=True)
        assert r.returncode != 0 and opts[0] in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
