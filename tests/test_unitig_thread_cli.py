"""GPU (-m gpu): `sdt-kmers thread` on the built cases of the bubble tests, written as FASTA, against the Python restatement of the rule
and of its outputs (unitig_thread_util.py): prefix.readPaths, prefix.unitigReads and the summary line, byte for byte; and the unitig
files against what `sdt-kmers unitigs` writes from the same input."""
import os
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_thread_util as tu

pytestmark = pytest.mark.gpu


def library(tmp_path, case):
    letters = np.frombuffer(cu.LETTERS.encode(), dtype=np.uint8)
    with open(tmp_path / "s.fa", "wb") as fo:
        for i, r in enumerate(case["counted"]):
            fo.write(b">r%d\n%s\n" % (i, letters[r].tobytes()))
    cfg = tmp_path / "lib.cfg"
    cfg.write_text(f"max_rd_len={case['L']}\n[LIB]\navg_ins=100\nasm_flags=1\nf={tmp_path / 's.fa'}\n")
    return str(cfg)


def run(pkg, sub, cfg, K, out, *more):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, sub, "-s", cfg, "-K", str(K), "-p", "4", "-o", str(out)] + list(more), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("K", [31, 65])
def test_sdt_kmers_thread_cli(pkg, tmp_path, K):
    case = bu.built_case(K)
    cfg = library(tmp_path, case)
    for name, args, (mc, ml) in (("a", [], (2, 1)), ("b", ["-c", "1"], (1, 1))):
        th = tu.bubble_threading(K, mc, ml)
        rec, offs, segs = tu.bubble_records(K, mc, ml)
        lines = run(pkg, "thread", cfg, K, tmp_path / name, *args)
        run(pkg, "unitigs", cfg, K, tmp_path / (name + "_u"), *args)
        assert (tmp_path / f"{name}.readPaths").read_text() == tu.read_paths_text(rec, offs, segs), f"K={K} {name}.readPaths"
        assert (tmp_path / f"{name}.unitigReads").read_text() == tu.unitig_reads_text(len(th.m.unitigs), rec, offs, segs), f"K={K} {name}.unitigReads"
        assert [x for x in lines if x.startswith("thread: ")] == [tu.summary_line(rec, segs)]
        for ext in ("unitigs", "unitigs.fa", "unitigs.gfa"):
            assert (tmp_path / f"{name}.{ext}").read_bytes() == (tmp_path / f"{name}_u.{ext}").read_bytes(), ext
