"""GPU (-m gpu): `sdt-kmers clip` on a library of single reads and a library of a pair of files with planted adapters and tails, against
the Python restatement of the rule and of the four files (read_clip_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_clip_util as rc
from test_read_dedup_cli import write_fastq

pytestmark = pytest.mark.gpu

K = 31


def library(tmp_path):
    """41 single reads of 50 .. 100 bases (q=, the smaller avg_ins: streamed first, so the pairs start at an odd ordinal) and 40 pairs
    of up to 100 bases (q1= / q2=); every third read carries a read-through 3' adapter, an A tail, the remnant of a 5' adapter with a
    T head, or several of them; pairs 5 and 22 lose read 2, pair 9 loses read 1, pair 30 loses both; returns the config, the stream in
    ordinal order, the pair ranges and the adapters [(name, codes, end)] in the order -a then -g"""
    rng = np.random.default_rng(32)

    def seq(L):                                           # (ends away from A and T: no chance tail joins a planted one)
        s = rng.integers(0, 4, size=L, dtype=np.uint8)
        s[0], s[-1] = rc.C, rc.G
        return s

    adapters = [("truseq_like", seq(33), 0), ("second", seq(58), 0), ("switch_oligo", seq(30), 1)]
    As, Ts = (lambda n: np.full(n, rc.A, dtype=np.uint8)), (lambda n: np.full(n, rc.T, dtype=np.uint8))

    def dress(i, L):
        kind = i % 9
        if kind == 0:
            return np.concatenate([seq(L - 25), adapters[0][1][:25]])
        if kind == 3:
            return np.concatenate([seq(L - 40), As(12), adapters[1][1][:28]])
        if kind == 6:
            return np.concatenate([adapters[2][1][-14:], Ts(8), seq(L - 22)])
        return seq(L)

    singles = [dress(i, int(rng.integers(50, 101))) for i in range(41)]
    r1 = [dress(i + 1, 80) for i in range(40)]
    r2 = [dress(i + 2, int(rng.integers(60, 101))) for i in range(40)]
    gone = lambda: np.concatenate([seq(12), adapters[0][1], seq(20)])          # 12 bases are left: fewer than --min-len
    r2[5], r2[22], r1[9], r1[30], r2[30] = gone(), gone(), gone(), gone(), As(70)
    singles[20] = gone()
    write_fastq(tmp_path / "s.fq", singles, "")
    write_fastq(tmp_path / "p_1.fq", r1, "/1")
    write_fastq(tmp_path / "p_2.fq", r2, "/2")
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n")
    (tmp_path / "a3.fa").write_text(rc.fasta_of([(n, a) for n, a, e in adapters if e == 0]).replace("CG", "cg", 3))       # (either case)
    (tmp_path / "a5.fa").write_text(rc.fasta_of([(n, a) for n, a, e in adapters if e == 1]))
    stream = singles + [r for pair in zip(r1, r2) for r in pair]
    return str(cfg), stream, [(len(singles), len(singles) + 2 * len(r1))], adapters


def test_sdt_kmers_clip_cli(pkg, tmp_path):
    cfg, stream, ranges, adapters = library(tmp_path)
    codes, offs = rc.concat(stream)
    n = len(stream)
    p = rc.params(min_len=30, min_tail=6, tail3_bases=1 << rc.A, tail5_bases=1 << rc.T)
    clip, (rec_txt, pairs_txt, single_txt, stats_txt) = rc.expect_cli(codes, offs, [(nm, a) for nm, a, _ in adapters], [e for _, _, e in adapters], p, ranges)
    first = ranges[0][0]
    live = clip["len"] > 0
    lost_one = [t for t in range(40) if live[first + 2 * t] != live[first + 2 * t + 1]]
    assert first & 1 and {5, 9, 22} <= set(lost_one) and not live[first + 60] and not live[first + 61]
    assert {rc.WHOLE, rc.CLIPPED, rc.DROPPED} == set(clip["verdict"].tolist()) and (clip["tail3"] > 0).any() and (clip["tail5"] > 0).any()
    assert {int(a) & 0xFFFF for a in clip["adapters"]} >= {0, 1, 2} and (clip["adapters"] >> 16 == 3).any()
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "clip", "-s", cfg, "-K", str(K), "-p", "4", "-a", str(tmp_path / "a3.fa"), "-g", str(tmp_path / "a5.fa"), "--tail3", "A",
                        "--tail5", "t", "--min-tail", "6", "--min-len", "30", "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in (("readClip", rec_txt), ("clip.pairs.fa", pairs_txt), ("clip.single.fa", single_txt), ("clipStats", stats_txt)):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    # pairs are in the pairs file only when both mates survive, next to each other; the survivor of a broken pair is a single read
    names = [int(x[1:]) - 1 for x in pairs_txt.splitlines()[0::2]]
    assert names and all(first <= a < ranges[0][1] and b == a + 1 and live[a] and live[b] for a, b in zip(names[0::2], names[1::2]))
    assert all((a - first) % 2 == 0 for a in names[0::2]) and len(names) == 2 * sum(bool(live[first + 2 * t] and live[first + 2 * t + 1]) for t in range(40))
    singles_out = [int(x[1:]) - 1 for x in single_txt.splitlines()[0::2]]
    assert {first + 2 * 5, first + 2 * 22, first + 2 * 9 + 1} <= set(singles_out)
    last = [x for x in r.stdout.splitlines() if "whole" in x]
    v = clip["verdict"]
    assert len(last) == 1 and [int(x) for x in last[0].replace(";", "").replace(",", "").replace(":", "").split() if x.isdigit()] == [
        n, int((v == 0).sum()), int((v == 2).sum()), int((v == 3).sum()), int(offs[-1]), int(clip["len"].sum())]


def test_sdt_kmers_clip_refuses_a_bad_adapter_file(pkg, tmp_path):
    cfg, stream, ranges, adapters = library(tmp_path)
    bad = tmp_path / "bad.fa"
    bad.write_text(">good\nACGTACGT\n>iupac\nACGTRCGT\n")
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    r = subprocess.run([exe, "clip", "-s", cfg, "-K", str(K), "-a", str(bad), "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode != 0 and f"{bad} line 4: 'R' is not one of ACGT" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
