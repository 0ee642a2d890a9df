"""GPU (-m gpu): `sdt-kmers qtrim` on a library of single reads and a reverse_seq library of a pair of files, against the numpy
restatement of the rule and of the four files (read_quality_util.py), and its two refusals of input without usable qualities."""
import os
import subprocess

import numpy as np
import pytest

import read_quality_util as qu
from read_dedup_util import concat
from read_select_util import LETTERS

pytestmark = pytest.mark.gpu

K = 31
P = qu.params(min_len=20, max_ee_ppm=30000)
OPTIONS = ("--min-len", "20", "--max-ee", "30000")


def write_fastq(path, reads, quals, tag, cut_quality_of=None):
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    with open(path, "wb") as fo:
        for i, (r, q) in enumerate(zip(reads, quals)):
            fo.write(b"@r%d%s\n%s\n+\n%s\n" % (i, tag.encode(), letters[r].tobytes(), q.tobytes()[:-3] if i == cut_quality_of else q.tobytes()))


def library(tmp_path):
    """the reads of the case that have 40 .. 250 bases and as many with the qualities of a sequencer as make 155: 35 single reads (q=,
    the smaller avg_ins: streamed first, so the pairs start at an odd ordinal) and 60 pairs (q1= / q2=) of a reverse_seq library, whose
    reads arrive reverse-complemented with their qualities reversed; returns the config, the stream (bases, qualities) in ordinal
    order and the pair ranges"""
    c = qu.case()
    rng = np.random.default_rng(44)
    pool = [r for r in c["reads"] if 40 <= len(r) <= 250 and 33 <= int(r.min()) and int(r.max()) <= 126]
    pool += [(qu.realistic(rng, int(rng.integers(40, 201)), i) + 33).astype(np.uint8) for i in range(155 - len(pool))]
    assert len(pool) == 155 and all(33 <= int(q.min()) and int(q.max()) <= 126 for q in pool)         # printable: they go into a FASTQ file
    pool = [pool[int(i)] for i in rng.permutation(155)]
    bases = [rng.integers(0, 4, size=len(q), dtype=np.uint8) for q in pool]
    write_fastq(tmp_path / "s.fq", bases[:35], pool[:35], "")
    write_fastq(tmp_path / "p_1.fq", bases[35:95], pool[35:95], "/1")
    write_fastq(tmp_path / "p_2.fq", bases[95:155], pool[95:155], "/2")
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len=250\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n"
                   f"[LIB]\navg_ins=200\nreverse_seq=1\nasm_flags=3\nq1={tmp_path / 'p_1.fq'}\nq2={tmp_path / 'p_2.fq'}\n")
    rc = lambda b: (b[::-1] ^ 2).astype(np.uint8)                                                    # A0 C1 T2 G3
    order = [i for pair in zip(range(35, 95), range(95, 155)) for i in pair]
    stream_bases = bases[:35] + [rc(bases[i]) for i in order]
    stream_quals = pool[:35] + [pool[i][::-1] for i in order]
    return str(cfg), stream_bases, stream_quals, [(35, 155)]


def test_sdt_kmers_qtrim_cli(pkg, tmp_path):
    cfg, stream_bases, stream_quals, ranges = library(tmp_path)
    codes, offs = concat(stream_bases)
    quals, qoffs = qu.concat_bytes(stream_quals)
    assert offs.tolist() == qoffs.tolist()
    out = qu.expect_quality(quals, offs, P)[0]
    why = qu.causes(out, P)
    assert {qu.WHOLE, qu.CLIPPED, qu.DROPPED} == set(out["verdict"].tolist()) and all(why.count(k) >= 3 for k in ("short", "low", "errors"))
    assert (out["start"] > 0).sum() >= 10
    texts = qu.cli_texts(codes, offs, out, ranges, P)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "qtrim", "-s", cfg, "-K", str(K), "-p", "4", *OPTIONS, "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for ext, text in zip(("readQual", "qtrim.pairs.fa", "qtrim.single.fa", "lenHist"), texts):
        got = (tmp_path / f"out.{ext}").read_text()
        assert got == text, f"out.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
    v = out["verdict"]
    summary = texts[3].splitlines()[-1]
    assert summary == (f"# reads 155 whole {int((v == 0).sum())} clipped {int((v == 2).sum())} dropped {int((v == 3).sum())} short {why.count('short')} "
                       f"low {why.count('low')} errors {why.count('errors')} bases_in {int(offs[-1])} bases_out {int(out['len'].sum())}")
    last = [x for x in r.stdout.splitlines() if "expected errors" in x]
    assert len(last) == 1 and [int(x) for x in last[0].replace(";", " ").replace(",", " ").replace(":", " ").replace("(", " ").replace(")", " ").split() if x.isdigit()] == [
        155, int((v == 0).sum()), int((v == 2).sum()), int((v == 3).sum()), why.count("short"), why.count("low"), why.count("errors"), int(offs[-1]), int(out["len"].sum())]
    # pairs are in the pairs file only when both mates survive, next to each other; the survivor of a broken pair is a single read
    first, end = ranges[0]
    live = out["len"] > 0
    npairs = (end - first) // 2
    lost_one = [t for t in range(npairs) if live[first + 2 * t] != live[first + 2 * t + 1]]
    assert first & 1 and len(lost_one) >= 5
    names = [int(x[1:]) - 1 for x in texts[1].splitlines()[0::2]]
    assert names and all(first <= a < end and b == a + 1 and live[a] and live[b] for a, b in zip(names[0::2], names[1::2]))
    singles_out = {int(x[1:]) - 1 for x in texts[2].splitlines()[0::2]}
    assert {first + 2 * t + (0 if live[first + 2 * t] else 1) for t in lost_one} <= singles_out


def test_sdt_kmers_qtrim_refuses_input_without_qualities(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    rng = np.random.default_rng(45)
    bases = [rng.integers(0, 4, size=60, dtype=np.uint8) for _ in range(20)]
    quals = [np.full(60, 33 + 38, dtype=np.uint8) for _ in range(20)]
    out = str(tmp_path / "out")
    # a library with a FASTA file
    write_fastq(tmp_path / "good.fq", bases, quals, "")
    letters = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    (tmp_path / "reads.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, letters[r].tobytes()) for i, r in enumerate(bases)))
    (tmp_path / "fa.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 'good.fq'}\nf={tmp_path / 'reads.fa'}\n")
    r = subprocess.run([exe, "qtrim", "-s", str(tmp_path / "fa.cfg"), "-K", str(K), "-o", out], capture_output=True, text=True)
    assert r.returncode not in (0, 255) and "qtrim needs base qualities" in r.stderr and "reads.fa" in r.stderr
    # a FASTQ file in which one quality line is three bytes short
    write_fastq(tmp_path / "short.fq", bases, quals, "", cut_quality_of=13)
    (tmp_path / "short.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 'short.fq'}\n")
    r = subprocess.run([exe, "qtrim", "-s", str(tmp_path / "short.cfg"), "-K", str(K), "-o", out], capture_output=True, text=True)
    assert r.returncode not in (0, 255) and "quality line that is not as long as their sequence line" in r.stderr and "sdt-kmers: 1 records" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
    # the file with whole quality lines passes
    (tmp_path / "good.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 'good.fq'}\n")
    r = subprocess.run([exe, "qtrim", "-s", str(tmp_path / "good.cfg"), "-K", str(K), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.lenHist").read_text() == "60 20\n# reads 20 whole 20 clipped 0 dropped 0 short 0 low 0 errors 0 bases_in 1200 bases_out 1200\n"
