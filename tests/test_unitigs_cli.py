"""GPU (-m gpu): `sdt-kmers unitigs` on the built cases of the bubble tests, against the Python restatement of the rule and of the four
outputs (unitig_util.py): prefix.unitigs, prefix.unitigs.fa, prefix.unitigs.gfa and the summary line, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_util as uu

pytestmark = pytest.mark.gpu
COMPLEMENT = str.maketrans("ACGT", "TGCA")


def library(tmp_path, case):
    letters = np.frombuffer(cu.LETTERS.encode(), dtype=np.uint8)
    with open(tmp_path / "s.fq", "wb") as fo:
        for i, r in enumerate(case["counted"]):
            fo.write(b"@r%d\n%s\n+\n%s\n" % (i, letters[r].tobytes(), b"I" * len(r)))
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len={case['L']}\n[LIB]\navg_ins=100\nasm_flags=1\nq={tmp_path / 's.fq'}\n")
    return str(cfg)


def run(pkg, cfg, K, out, *more):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "unitigs", "-s", cfg, "-K", str(K), "-p", "4", "-o", str(out)] + list(more), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("K", [31, 63])
def test_sdt_kmers_unitigs_cli(pkg, tmp_path, K):
    case = bu.built_case(K)
    cfg = library(tmp_path, case)
    runs = (("a", [], uu.Unitigs(case["nodes"], K, **uu.DEFAULTS)),
            ("b", ["-c", "1", "--max-count", "0", "--min-link", "1"], uu.Unitigs(case["nodes"], K, min_count=1, max_count=0, min_link=1)),
            ("c", ["--max-count", "40", "--min-link", "3"], uu.Unitigs(case["nodes"], K, min_count=2, max_count=40, min_link=3)))
    assert [len(m.unitigs) for _, _, m in runs][:2] == [36, 41] and runs[2][2].info != runs[0][2].info
    exts = (("unitigs", uu.unitigs_text), ("unitigs.fa", uu.fasta_text), ("unitigs.gfa", uu.gfa_text))
    for name, args, model in runs:
        lines = run(pkg, cfg, K, tmp_path / name, *args)
        for ext, text in exts:
            got, want = (tmp_path / f"{name}.{ext}").read_text(), text(model)
            assert got == want, f"K={K} {name}.{ext} differs from the rule ({len(got)} bytes, {len(want)} expected)"
        assert [x for x in lines if x.startswith("unitigs: ")] == [uu.summary_line(model)]
    # every L line's overlap, on the S lines of the file itself
    gfa = [x.split("\t") for x in (tmp_path / "a.unitigs.gfa").read_text().splitlines()]
    seq = {x[1]: x[2] for x in gfa if x[0] == "S"}
    oriented = lambda name, sign: seq[name] if sign == "+" else seq[name][::-1].translate(COMPLEMENT)
    links = [x for x in gfa if x[0] == "L"]
    assert gfa[0] == ["H", "VN:Z:1.0"] and len(seq) == 36 and len(links) == 25 and all(x[5] == f"{K - 1}M" for x in links)
    for _, a, sa, b, sb, _, _ in links:
        assert oriented(a, sa)[-(K - 1):] == oriented(b, sb)[:K - 1], (a, sa, b, sb)
    # a second run writes the same bytes
    run(pkg, cfg, K, tmp_path / "again")
    for ext, _ in exts:
        assert (tmp_path / f"again.{ext}").read_bytes() == (tmp_path / f"a.{ext}").read_bytes(), ext
