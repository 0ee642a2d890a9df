"""CPU: the stream arithmetic of the level-1 scatter's read walk (csrc/sdt_sk_walk.h) -- the base window a lane takes its bases from
(every start phase, read lengths 1..300, the clamp at the tile's last readable word), the rolling canonical m-mer, and the one-pass
cut of a record's bases (every start offset 0..31, every length, the 24-byte, the 16-byte and the 2-word keys' form) against the
stream accessors the kernel used before.  tools/sk_walk_check.cpp includes the plain headers alone and runs under ASan + UBSan as a
stand-alone program: the tile is a heap block of exactly the readable words."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")


def test_window_roll_and_cut_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "sk_walk_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert sorted(includes) == ["../soapdenovo-trans_amd/csrc/sdt_sk_record1.h", "../soapdenovo-trans_amd/csrc/sdt_sk_walk.h"], includes
    hdr = open(os.path.join(CSRC, "sdt_sk_walk.h")).read()
    assert not re.search(r"#include\s+[<\"](?!stdint\.h|sdt_sk_record2\.h)", hdr), "sdt_sk_walk.h is plain C++ over <stdint.h> (and the header that defines SDT_SK_HD)"
    exe = str(tmp_path / "sk_walk_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("sk_walk_check: ok"), r.stdout + r.stderr


def test_the_kernel_uses_these_functions():
    """the walk takes its bases, its canonical m-mers and its records' bases through sdt_sk_walk.h (a copy of the arithmetic inside the
    kernel would leave the test above testing nothing), and fetches no base from the tile by itself"""
    seq = open(os.path.join(CSRC, "sdt_sk_scatter_seq.cuh")).read()
    assert '#include "sdt_sk_walk.h"' in seq
    kernel = seq[seq.index("void k_sk_scatter_reads_seq("):]
    for fn in ("sk_win_init(", "sk_win_refill(", "sk_roll_init(", "sk_roll_step("):
        assert kernel.count(fn) == 1, fn
    assert seq.count("sk_cut_bases<BW, TAIL_PAD>(") == 1
    assert "sk_stream_word(" not in seq, "records are cut by sk_cut_bases"
    assert "pb >> 4" not in seq and "pb & 15" not in seq, "no per-base fetch from the tile"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("sdt_sk_walk.h") >= 2, "the library and the scatter's units depend on the header"
