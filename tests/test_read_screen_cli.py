"""GPU (-m gpu): `sdt-kmers screen` on a tiny library of a pair of FASTQ files and a single-end FASTA file, with two reference files,
against the Python restatement of the rule and of the four files (read_screen_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import read_screen_util as su
from test_read_dedup_cli import write_fastq

pytestmark = pytest.mark.gpu

K = 31
SCREEN_K = 21


def letters(codes):
    return "".join(su.LETTERS[int(c)] for c in codes)


def references(tmp_path):
    """two files, three references: rRNA-like (900 bases, wrapped, with NN inside and a lower-case line), PhiX-like (400 bases) and, in
    the second file, one that shares a stretch with the first and is therefore never attributed for it"""
    rng = np.random.default_rng(61)
    seq = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    a, b = seq(900), seq(400)
    c = np.concatenate([seq(150), a[300:380], seq(150)])
    ta = letters(a[:500]) + "NN" + letters(a[500:])
    wrapped = "\n".join(ta[i:i + 70] for i in range(0, len(ta), 70))
    wrapped = wrapped[:71] + wrapped[71:142].lower() + wrapped[142:]
    texts = [f">rRNA_28S some description\n{wrapped}\n\n>phiX\n{letters(b)}\n", f">mito x\n{letters(c)}\n"]
    paths = []
    for i, t in enumerate(texts):
        p = tmp_path / f"refs{i}.fa"
        p.write_text(t)
        paths.append(str(p))
    return paths, texts, (a, b, c)


def library(tmp_path, refs):
    """30 single reads (f=, the smaller avg_ins: streamed first) and 30 pairs (q1= / q2=): reads cut from the references, either strand,
    and random ones, so that pairs have the first mate, the second, both and neither matched"""
    a, b, c = refs
    rng = np.random.default_rng(62)

    def cut(src):
        n = int(rng.integers(50, 120))
        at = int(rng.integers(0, len(src) - n + 1))
        r = src[at:at + n].copy()
        return su.revcomp(r) if rng.random() < 0.5 else r

    rand = lambda: rng.integers(0, 4, size=int(rng.integers(15, 120)), dtype=np.uint8)
    pick = lambda i: (cut(a), rand(), cut(b), rand(), cut(c), rand())[i % 6]
    singles = [pick(i) for i in range(30)]
    r1 = [pick(i // 2) for i in range(30)]
    r2 = [pick(i // 3 + 1) for i in range(30)]
    with open(tmp_path / "s.fa", "w") as fo:
        for i, r in enumerate(singles):
            fo.write(f">s{i}\n{letters(r)}\n")
    write_fastq(tmp_path / "p_1.fq", r1, "/1")
    write_fastq(tmp_path / "p_2.fq", r2, "/2")
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=250\n[LIB]\navg_ins=100\nasm_flags=1\nf={tmp_path / 's.fa'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n")
    return str(cfg), singles + [r for pair in zip(r1, r2) for r in pair], [(len(singles), len(singles) + 2 * len(r1))]


@pytest.mark.parametrize("keep_matched", (False, True))
def test_sdt_kmers_screen_cli(pkg, tmp_path, keep_matched):
    paths, texts, refs = references(tmp_path)
    cfg, stream, ranges = library(tmp_path, refs)
    seqs, ref_of_seq, names, bases = su.parse_refs(texts)
    assert names == ["rRNA_28S", "phiX", "mito"] and bases == [900, 400, 380] and ref_of_seq == [0, 0, 1, 2]
    d = su.build_set(seqs, ref_of_seq, SCREEN_K)
    p = su.params(min_hits=2, min_hit_pct=10, flags=su.KEEP_MATCHED if keep_matched else 0)
    codes, offs = su.concat(stream)
    facts = su.all_facts(codes, offs, SCREEN_K, d)
    lens = np.diff(offs.astype(np.int64)).tolist()
    rec = su.verdicts(facts, lens, p, su.ranged_units(range(len(stream)), ranges))[0]
    first, end = ranges[0]
    m = [su.read_matched(f[0], f[1], p) for f in facts]
    assert {(m[first + 2 * t], m[first + 2 * t + 1]) for t in range((end - first) // 2)} == {(True, False), (False, True), (True, True), (False, False)}
    assert {0, 1, 2, su.NO_REF} == set(f[2] for f in facts)
    want = su.cli_texts(codes, offs, rec, ranges, names, bases, p)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    options = ["-r", paths[0], "-r", paths[1], "--screen-k", str(SCREEN_K), "--min-hits", "2", "--min-hit-pct", "10"] + (["--keep-matched"] if keep_matched else [])
    r = subprocess.run([exe, "screen", "-s", cfg, "-K", str(K), "-p", "4", *options, "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in zip(("readScreen", "screen.pairs.fa", "screen.single.fa", "screenStats"), want):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    assert want[1] and want[2] and want[3].splitlines()[-1] == f"# reads 90 matched {sum(m)} kept {int((rec['verdict'] == 0).sum())} dropped {int((rec['verdict'] == 1).sum())}"
    # both mates of a pair go the same way
    assert all(rec["verdict"][first + 2 * t] == rec["verdict"][first + 2 * t + 1] for t in range((end - first) // 2))


def test_sdt_kmers_screen_cli_malformed_reference(pkg, tmp_path):
    """a reference file with a record that has no sequence, or with bases before the first header, stops the run before any data file is
    written; so does a set without a k-mer"""
    paths, texts, refs = references(tmp_path)
    cfg, _, _ = library(tmp_path, refs)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    for name, text, say in (("empty_record.fa", ">a\nACGTACGTACGTACGTACGTACGTACGTACGT\n>b\n>c\nACGT\n", "empty_record.fa line 3:"),
                            ("headless.fa", "\nACGT\n>a\nACGT\n", "headless.fa line 2:"), ("short.fa", ">a\nACGTNACGTNACGT\n", "no k-mer")):
        bad = tmp_path / name
        bad.write_text(text)
        first = [] if name == "short.fa" else ["-r", paths[0]]
        r = subprocess.run([exe, "screen", "-s", cfg, "-K", str(K), *first, "-r", str(bad), "-o", str(tmp_path / "out")], capture_output=True, text=True)
        assert r.returncode == 2 and say in r.stderr, f"{name}: {r.returncode} {r.stderr[:300]}"
        assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
