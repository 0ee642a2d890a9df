"""GPU (-m gpu): `sdt-kmers qc` on the library of tests/test_read_quality_cli.py (single reads and a reverse_seq pair of files) and on
a FASTA library, against the numpy restatement of the rule and of the three files (read_qc_util.py), and what it refuses."""
import os
import subprocess

import numpy as np
import pytest

import read_qc_util as qc
import read_quality_util as qu
from read_dedup_util import concat
from read_select_util import LETTERS
from test_read_quality_cli import library, write_fastq

pytestmark = pytest.mark.gpu

K = 31
FILES = ("qcBases", "qcQuals", "qcReads")


def tool(pkg):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    return exe


def by_class(codes, offs, quals, classes, cycles, flags=0):
    return {k: qc.expect(codes, offs, quals, classes=classes, cycles=cycles, flags=flags, class_sel=k) for k in sorted(set(classes.tolist()))}


def test_sdt_kmers_qc_cli(pkg, tmp_path):
    """35 single reads (class 0) and 60 pairs (classes 1 and 2) of 40 .. 250 bases under 100 cycles, forward and from the end: the
    three files and the line per class are those of the rule; under the default of 1 024 cycles no read reaches the last row"""
    cfg, stream_bases, stream_quals, ranges = library(tmp_path)
    codes, offs = concat(stream_bases)
    quals, _ = qu.concat_bytes(stream_quals)
    n = len(offs) - 1
    first, end = ranges[0]
    classes = np.array([0 if not first <= r < end else 1 + (r - first) % 2 for r in range(n)], dtype=np.uint8)
    assert [(classes == k).sum() for k in (0, 1, 2)] == [35, 60, 60] and (np.diff(offs.astype(np.int64)) > 100).sum() >= 30
    exe = tool(pkg)
    for opts, cycles, flags in ((("--cycles", "100"), 100, 0), (("--cycles", "100", "--from-end"), 100, qc.FROM_END), ((), 1024, 0)):
        want = qc.cli_texts(by_class(codes, offs, quals, classes, cycles, flags), {0: True, 1: True, 2: True}, cycles)
        out = tmp_path / f"out{cycles}{flags}"
        r = subprocess.run([exe, "qc", "-s", cfg, "-K", str(K), "-p", "4", *opts, "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for ext, text in zip(FILES, want):
            got = open(f"{out}.{ext}").read()
            assert got == text, f"{opts}: {ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
        assert "".join(x + "\n" for x in r.stdout.splitlines() if x.startswith("qc: ")) == want[3], r.stdout
        assert f"{n} reads\n" in r.stdout
        assert ("100+" in want[0]) == (cycles == 100) and "\n1 " in want[1] and "meanq 2 " in want[2]


def test_sdt_kmers_qc_of_a_fasta_library_and_refusals(pkg, tmp_path):
    exe = tool(pkg)
    rng = np.random.default_rng(46)
    bases = [rng.integers(0, 4, size=int(L), dtype=np.uint8) for L in rng.integers(1, 90, 40)]
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    (tmp_path / "reads.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, letters[r].tobytes()) for i, r in enumerate(bases)))
    (tmp_path / "fa.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nf={tmp_path / 'reads.fa'}\n")
    codes, offs = concat(bases)
    want = qc.cli_texts({0: qc.expect(codes, offs, None, cycles=50)}, {0: False}, 50)
    out = str(tmp_path / "fa")
    r = subprocess.run([exe, "qc", "-s", str(tmp_path / "fa.cfg"), "-K", str(K), "--cycles", "50", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in zip(FILES, want):
        assert open(f"{out}.{ext}").read() == text, ext
    assert want[1] == "# class row bases mean_x100 min q10 q25 median q75 q90 max\n# class 0: no qualities\n"
    assert "# meanq class 0: no qualities\n" in want[2] and " q20 - q30 -\n" in r.stdout and want[3] in r.stdout
    # refused before a file is written: the cycles, an option of another stage, a quality line that is three bytes short
    out = str(tmp_path / "no")
    for opts, say in ((("--cycles", "0"), "--cycles"), (("--cycles", "4097"), "--cycles"), (("--cut-q", "20"), "--cut-q belongs to qtrim"),
                      (("--min-len", "5"), "--min-len belongs to"), (("--phred", "50"), "--phred")):
        r = subprocess.run([exe, "qc", "-s", str(tmp_path / "fa.cfg"), "-K", str(K), *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    quals = [np.full(len(b), 33 + 38, dtype=np.uint8) for b in bases]
    long_enough = next(i for i, b in enumerate(bases) if len(b) > 3)
    write_fastq(tmp_path / "short.fq", bases, quals, "", cut_quality_of=long_enough)
    (tmp_path / "short.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 'short.fq'}\n")
    r = subprocess.run([exe, "qc", "-s", str(tmp_path / "short.cfg"), "-K", str(K), "-o", out], capture_output=True, text=True)
    assert r.returncode not in (0, 255) and "quality line that is not as long as their sequence line" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]
    # --phred 64 on the same bytes: every quality is 0 below the offset or the byte minus 64
    write_fastq(tmp_path / "good.fq", bases, quals, "")
    (tmp_path / "good.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 'good.fq'}\n")
    out = str(tmp_path / "p64")
    r = subprocess.run([exe, "qc", "-s", str(tmp_path / "good.cfg"), "-K", str(K), "--cycles", "50", "--phred", "64", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = qc.cli_texts({0: qc.expect(codes, offs, qu.concat_bytes(quals)[0], cycles=50, phred_offset=64)}, {0: True}, 50)
    for ext, text in zip(FILES, want):
        assert open(f"{out}.{ext}").read() == text, ext
    assert " 700 7 7 7 7 7 7 7\n" in want[1]
