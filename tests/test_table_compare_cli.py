"""GPU (-m gpu): `sdt-kmers compare` on two small FASTQ configs -- the reads of a golden case as A, a part of them and reads of another
transcriptome as B -- against the Python restatement of the rule and of the three outputs (table_compare_util.py); the refusals of its
options; a second config that is not there."""
import os
import subprocess

import numpy as np
import pytest

import asm_support_util as au
import golden_util as gu
import table_compare_util as tu

pytestmark = pytest.mark.gpu

K, MIN_COUNT = 23, 2


def exe_of(pkg):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    return exe


def test_sdt_kmers_compare_cli(pkg, synth, tmp_path):
    info = gu.load_case("se100_k23_p8")
    acodes, aoffs = gu.case_reads(info)
    n = len(aoffs) - 1
    L = info["max_rd_len"]
    # B: the first 1 500 reads of A, and 600 reads of 100 bases from four transcripts that A has never seen
    tx = synth.make_transcriptome(4, seed=913, lo=300, hi=600)
    ncodes, noffs = synth.sample_reads(*tx, n_reads=600, read_len=L, seed=914, err=0.002)
    reads = [acodes[int(aoffs[i]):int(aoffs[i + 1])] for i in range(1500)] + [ncodes[int(noffs[i]):int(noffs[i + 1])] for i in range(600)]
    bcodes, boffs = au.concat(reads)
    A, B = au.oracle_counts(acodes, aoffs, K)[0], au.oracle_counts(bcodes, boffs, K)[0]
    for name, codes, offs in (("a", acodes, aoffs), ("b", bcodes, boffs)):
        synth.write_fastq(str(tmp_path / f"{name}.fq"), codes, offs)
        synth.write_config(str(tmp_path / f"{name}.cfg"), L, fastq=[str(tmp_path / f"{name}.fq")])
    m, t = tu.compare(A, B, 64, 48)
    sel = tu.select(A, B, 2, tu.U32, 0, 0)                                        # the solid k-mers of A that B does not hold
    X, Y, S = (int(x) for x in t[:3])
    assert n == info["n"] and 0 < S < min(X, Y) and Y - S > 1000 and 100 < len(sel) < X - S
    exe = exe_of(pkg)
    base = [exe, "compare", "-s", str(tmp_path / "a.cfg"), "--against", str(tmp_path / "b.cfg"), "-K", str(K), "-p", "4", "-c", str(MIN_COUNT), "--rows", "64",
            "--cols", "48"]
    r = subprocess.run(base + ["--select", "2:4294967295:0:0", "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.cmpMatrix").read_text() == tu.matrix_text(m)
    assert (tmp_path / "out.cmpKmers").read_text() == tu.kmers_text(sel, K)[0]
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("compare: ")] == [tu.summary_text(t, m, MIN_COUNT).rstrip("\n")]
    assert f"A: {n} reads, {len(A)} nodes allocated, {sum(A.values())} kmer in reads" in lines
    assert f"B: 2100 reads, {len(B)} nodes allocated, {sum(B.values())} kmer in reads" in lines
    # a list cut short: at most --max-list lines, every one a member, and the last line says how many matched; no --select: no list
    r = subprocess.run(base + ["--select", "0:4294967295:0:4294967295", "--max-list", "7", "-o", str(tmp_path / "cut")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "cut.cmpKmers").read_text().splitlines()
    everything = {f"{tu.kmer_text(k, K)} {ca} {cb}" for k, ca, cb in tu.select(A, B, 0, tu.U32, 0, tu.U32)}
    assert len(got) == 8 and got[-1] == f"# {len(A)} matched" and set(got[:7]) <= everything and len(set(got[:7])) == 7 and got[:7] == sorted(
        got[:7], key=lambda l: [au.LETTERS.index(c) for c in l.split()[0]])
    assert (tmp_path / "cut.cmpMatrix").read_text() == tu.matrix_text(m)
    r = subprocess.run(base + ["-d", "1", "-o", str(tmp_path / "plain")], capture_output=True, text=True)
    assert r.returncode == 0 and not (tmp_path / "plain.cmpKmers").exists(), r.stderr
    # -d 1 is applied to both tables: the k-mers seen once are deleted (their nodes stay, the rule ignores the flag), and each says so
    assert sum(l.startswith("A: ") and l.endswith(" kmer removed") for l in r.stdout.splitlines()) == 1
    assert sum(l.startswith("B: ") and l.endswith(" kmer removed") for l in r.stdout.splitlines()) == 1
    assert (tmp_path / "plain.cmpMatrix").read_text() == tu.matrix_text(m)


def test_option_refusals_and_a_missing_config(pkg, synth, tmp_path):
    exe = exe_of(pkg)
    cfg, out = str(tmp_path / "none.cfg"), str(tmp_path / "out")                  # (never opened: the options are refused first)
    for sub in ("profile", "evaluate", "query", "qc"):
        for opt in (("--against", cfg), ("--cols", "8"), ("--select", "1:2:0:0"), ("--max-list", "5")):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to compare" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    base = [exe, "compare", "-s", cfg, "--against", cfg, "-K", "31"]
    r = subprocess.run([exe, "compare", "-s", cfg, "-K", "31", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "--against b.cfg" in r.stderr
    r = subprocess.run(base + ["--assembly", "x.fa", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "--assembly belongs to evaluate" in r.stderr
    for opts, say in ((("--rows", "2"), "must exceed -c 2"), (("--cols", "2"), "must exceed -c 2"), (("--rows", "64", "-c", "64"), "must exceed -c 64"),
                      (("--rows", "1"), "--rows 1"), (("--cols", "x"), "--cols x"), (("--rows", "8193"), "--rows 8193"),
                      (("--rows", "8192", "--cols", "3"), "16384 at most"), (("--max-list", "x"), "--max-list x")):
        r = subprocess.run(base + [*opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    for text in ("1:2:3", "1:2:3:4:5", "5:4:0:0", "1:2:9:3", "a:2:0:0", "1:2:0:4294967296", "1:2:0:0x", ""):
        r = subprocess.run(base + ["--select", text, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and f"--select {text}: MINA:MAXA:MINB:MAXB is expected" in r.stderr, f"{text!r}: {r.returncode} {r.stderr[:200]}"
    # a.cfg is there, b.cfg is not: said and refused before the device is touched or anything is written
    codes, offs = au.concat([np.zeros(60, dtype=np.uint8)])
    synth.write_fastq(str(tmp_path / "a.fq"), codes, offs)
    synth.write_config(str(tmp_path / "a.cfg"), 100, fastq=[str(tmp_path / "a.fq")])
    missing = str(tmp_path / "b.cfg")
    r = subprocess.run([exe, "compare", "-s", str(tmp_path / "a.cfg"), "--against", missing, "-K", "31", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and f"Cannot open {missing}" in r.stdout and "reads," not in r.stdout, r.stdout + r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
