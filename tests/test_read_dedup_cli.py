"""GPU (-m gpu): `sdt-kmers dedup` on a library of single reads and a library of a pair of files with planted copies, against the Python
restatement of the rule and of the four files (read_dedup_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_dedup_util as rd
from read_select_util import LETTERS, ranged_units

pytestmark = pytest.mark.gpu

K = 31


def write_fastq(path, reads, tag):
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    with open(path, "wb") as fo:
        for i, r in enumerate(reads):
            fo.write(b"@r%d%s\n%s\n+\n%s\n" % (i, tag.encode(), letters[r].tobytes(), b"I" * len(r)))


def library(tmp_path):
    """41 single reads of 50 .. 100 bases (q=, the smaller avg_ins: streamed first, so the pairs start at an odd ordinal) and 40 pairs
    of 80 bases (q1= / q2=), with copies of reads, copies of pairs, pairs read from the other strand, and a single read that equals a
    mate; returns the config, the stream in ordinal order and the pair ranges"""
    rng = np.random.default_rng(31)
    seq = lambda L: rng.integers(0, 4, size=L, dtype=np.uint8)
    singles = [seq(int(rng.integers(50, 101))) for _ in range(41)]
    r1 = [seq(80) for _ in range(40)]
    r2 = [seq(80) for _ in range(40)]
    for dst, src in ((7, 2), (19, 2), (30, 2), (11, 5), (40, 33), (12, 13)):
        singles[dst] = singles[src]
    singles[25] = singles[24][:-1]
    for dst, src in ((9, 1), (21, 1), (38, 1), (15, 14), (39, 0)):
        r1[dst], r2[dst] = r1[src], r2[src]
    for dst, src in ((17, 3), (35, 14)):                  # the same fragment from the other strand
        r1[dst], r2[dst] = r2[src], r1[src]
    r2[26] = r2[27]                                       # one mate in common is not a copy
    singles[3] = r1[4]
    write_fastq(tmp_path / "s.fq", singles, "")
    write_fastq(tmp_path / "p_1.fq", r1, "/1")
    write_fastq(tmp_path / "p_2.fq", r2, "/2")
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n")
    stream = singles + [r for pair in zip(r1, r2) for r in pair]
    return str(cfg), stream, [(len(singles), len(singles) + 2 * len(r1))]


@pytest.mark.parametrize("swap", [False, True])
def test_sdt_kmers_dedup_cli(pkg, tmp_path, swap):
    cfg, stream, ranges = library(tmp_path)
    codes, offs = rd.concat(stream)
    n = len(stream)
    units = ranged_units(range(n), ranges)
    dup, keep, kept = rd.expect_dedup(codes, offs, flags=rd.MATE_SWAP if swap else 0, units=units)
    plain = rd.expect_dedup(codes, offs, units=units)[0]
    assert {1, 2, 4} <= set(plain["copies"].tolist()) and ranges[0][0] & 1
    if swap:
        assert ((plain["verdict"] == rd.KEPT) & (dup["verdict"] == rd.DROPPED)).sum() == 4
    dup_txt, pairs_txt, single_txt, lev_txt = rd.cli_texts(codes, offs, dup, keep, ranges)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "dedup", "-s", cfg, "-K", str(K), "-p", "4", "-o", str(tmp_path / "out")] + (["--mate-swap"] if swap else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in (("readDup", dup_txt), ("dedup.pairs.fa", pairs_txt), ("dedup.single.fa", single_txt), ("dupLevels", lev_txt)):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    # pairs are in the pairs file only when the unit is kept, both mates next to each other; the levels add up to the stream
    names = [int(x[1:]) - 1 for x in pairs_txt.splitlines()[0::2]]
    assert names and all(ranges[0][0] <= a < ranges[0][1] and b == a + 1 and keep[a] and keep[b] for a, b in zip(names[0::2], names[1::2]))
    assert all((a - ranges[0][0]) % 2 == 0 for a in names[0::2])
    levels = [tuple(int(x) for x in line.split()) for line in lev_txt.splitlines()]
    assert sum(lv[2] for lv in levels) == n and sum(lv[1] for lv in levels) == len(set(dup["first"].tolist()))
    assert levels == sorted(levels) and len(levels) >= 3
    last = [x for x in r.stdout.splitlines() if "reads kept" in x]
    assert len(last) == 1 and [int(x) for x in last[0].split() if x.isdigit()] == [kept, n, sum(lv[1] for lv in levels)]
