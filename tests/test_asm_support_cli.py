"""GPU (-m gpu): `sdt-kmers evaluate` on the named case written as wrapped FASTA, one contig with a run of N inside, against the Python
restatement of the rule and of the three outputs (asm_support_util.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import asm_support_util as au

pytestmark = pytest.mark.gpu

K, ROWS, MIN_COUNT = au.NAMED_K, au.NAMED_ROWS, au.NAMED_MIN_COUNT


def wrap(text, width):
    return "\n".join(text[i:i + width] for i in range(0, len(text), width))


def test_sdt_kmers_evaluate_cli(pkg, synth, tmp_path):
    case = au.named_case(synth)
    # the library: the reads of the case and five poly-G reads, so that the table HAS the node a run of N would hit if an N were a G
    rcodes, roffs = case["reads"]
    reads = [rcodes[int(a):int(b)] for a, b in zip(roffs[:-1], roffs[1:])] + [np.full(150, 3, dtype=np.uint8)] * 5
    codes, offs = au.concat(reads)
    counts = au.oracle_counts(codes, offs, K)[0]
    poly_c = au.canon_kmers(np.full(K, 3, dtype=np.uint8), K)[0]
    assert counts[poly_c] == 5 * (150 - K + 1)
    synth.write_fastq(str(tmp_path / "reads.fq"), codes, offs)
    synth.write_config(str(tmp_path / "lib.cfg"), 150, fastq=[str(tmp_path / "reads.fq")])
    # the assembly in two files: every sequence of the case a contig, wrapped at 70 and at 61 columns, a line in lower case; whole0 with
    # 40 N in its middle, which cut it into two segments
    names = sorted(case["at"], key=case["at"].get)
    texts = ["", ""]
    for i, name in enumerate(names):
        t = au.text_of(case["seqs"][case["at"][name]])
        if name == "whole0":
            t = t[:1000] + "N" * 40 + t[1000:]
        body = wrap(t, 70 if i % 2 else 61)
        if i % 5 == 0:
            body = body[:62] + body[62:124].lower() + body[124:]
        texts[i % 2] += f">{name} length={len(t)}\n{body}\n" + ("\n" if i % 7 == 0 else "")
    paths = []
    for i, t in enumerate(texts):
        (tmp_path / f"asm{i}.fa").write_text(t)
        paths.append(str(tmp_path / f"asm{i}.fa"))
    segs, ref_of_seq, seg_start, cnames, bases = au.parse_fasta(texts)
    assert len(segs) == len(names) + 1 and sorted(cnames) == sorted(names)     # whole0 gives two segments; the contig of K - 1 bases is a segment too
    w0 = cnames.index("whole0")
    assert ref_of_seq.count(w0) == 2 and [seg_start[j] for j, r in enumerate(ref_of_seq) if r == w0] == [0, 1040]
    rec, cn = au.support(segs, K, counts, MIN_COUNT)
    assert poly_c not in cn                                                    # the N run never yields a poly-G k-mer
    m = au.spectrum(counts, cn, ROWS)
    want_support, want_spectrum = au.support_text(rec, ref_of_seq, seg_start, cnames, bases), au.spectrum_text(m)
    S, N, F, V, D, E, C, P, Q = au.summary_fields(au.totals(rec), m, MIN_COUNT, K)
    assert S == len(segs) and 0 < C < E < D and 0 < V < F < N and P == str(10000 * C // E)
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "evaluate", "-s", str(tmp_path / "lib.cfg"), "-K", str(K), "-p", "4", "--assembly", paths[0], "--assembly", paths[1],
                        "--rows", str(ROWS), "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.asmSupport").read_text() == want_support
    assert (tmp_path / "out.asmSpectrum").read_text() == want_spectrum
    line, = [l for l in r.stdout.splitlines() if l.startswith("evaluate: ")]
    mt = re.fullmatch(r"evaluate: sequences (\d+) kmers (\d+) found (\d+) solid (\d+) nodes (\d+) solid_nodes (\d+) covered (\d+) completeness_x100 (\S+) qv_x100 (\S+)", line)
    assert mt, line
    assert [int(x) for x in mt.groups()[:7]] == [S, N, F, V, D, E, C] and mt.group(8) == P          # P is exact
    assert abs(int(mt.group(9)) - int(Q)) <= 1, (mt.group(9), Q)                                     # libm's rounding is the only freedom
    # the contig with the N run, in its own coordinates: its longest gap lies past the run or before it, never across
    row = [l.split() for l in want_support.splitlines() if l.split()[1] == "whole0"][0]
    assert int(row[2]) == len(case["seqs"][case["at"]["whole0"]]) and int(row[3]) == int(row[2]) - 2 * (K - 1)
