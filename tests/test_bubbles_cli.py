"""GPU (-m gpu): `sdt-kmers bubbles` on the built case of the bubble tests, against the Python restatement of the rule and of the two
files (bubble_util.py): prefix.bubbles, prefix.bubbles.fa and the summary line, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu

pytestmark = pytest.mark.gpu


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
    r = subprocess.run([exe, "bubbles", "-s", cfg, "-K", str(K), "-p", "4", "-o", str(out)] + list(more), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("K", [31, 63])
def test_sdt_kmers_bubbles_cli(pkg, tmp_path, K):
    case = bu.built_case(K)
    cfg = library(tmp_path, case)
    runs = (("a", ["--max-branch", "4000"], case["model"]),
            ("b", ["-c", "1", "--max-count", "0", "--min-link", "1"], bu.Bubbles(case["nodes"], K, min_count=1, max_count=0, min_link=1, max_len=1000)),
            ("c", ["--max-count", "40", "--min-link", "3", "--max-branch", "4000"], bu.Bubbles(case["nodes"], K, min_count=2, max_count=40, min_link=3, max_len=4000)))
    assert [len(m.bubbles) for _, _, m in runs][:2] == [8, 8] and runs[1][2].bubbles != runs[0][2].bubbles      # (b: the count-1 bubble for the long one)
    for name, args, model in runs:
        lines = run(pkg, cfg, K, tmp_path / name, *args)
        for ext, text in (("bubbles", bu.bubbles_text(model)), ("bubbles.fa", bu.fasta_text(model))):
            got = (tmp_path / f"{name}.{ext}").read_text()
            assert got == text, f"K={K} {name}.{ext} differs from the rule ({len(got)} bytes, {len(text)} expected)"
        assert [x for x in lines if x.startswith("bubbles: ")] == [bu.summary_line(model)]
    kinds = [line.split()[-1] for line in (tmp_path / "a.bubbles").read_text().splitlines()]
    assert sorted(set(kinds)) == ["0", "1", "2"]
    fa = (tmp_path / "a.bubbles.fa").read_text().splitlines()
    assert len(fa) == 4 * 8 and fa[0].startswith(">1_a len=") and fa[2].startswith(">1_b len=")
    # a second run writes the same bytes
    run(pkg, cfg, K, tmp_path / "again", "--max-branch", "4000")
    for ext in ("bubbles", "bubbles.fa"):
        assert (tmp_path / f"again.{ext}").read_bytes() == (tmp_path / f"a.{ext}").read_bytes(), ext
