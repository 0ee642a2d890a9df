"""CPU: the 16-byte compact level-2 record of 1-word keys (csrc/sdt_sk_record2.h) -- pack / unpack round trips for every K in 17..31,
every run length up to the cap and all context flags, zero padding bits, and a run cap that never admits a run that does not fit.
tools/sk_compact_check.cpp includes that header alone and runs under UBSan as a stand-alone program (a shift by 64 is the likely slip)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")


def test_pack_unpack_and_run_cap_clean_under_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "sk_compact_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["../soapdenovo-trans_amd/csrc/sdt_sk_record2.h"], includes
    assert not re.search(r"#include\s+[<\"](?!stdint\.h)", open(os.path.join(CSRC, "sdt_sk_record2.h")).read()), "sdt_sk_record2.h is plain C++ over <stdint.h>"
    exe = str(tmp_path / "sk_compact_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("sk_compact_check: ok"), r.stdout + r.stderr


def test_the_library_uses_these_functions():
    """the kernels and the host must take the record format and the cap from sdt_sk_record2.h (a copy of the logic inside a kernel
    would leave the test above testing nothing), and every stage derives "compact" from the same two facts"""
    fmt = open(os.path.join(CSRC, "sdt_superkmer.cuh")).read()
    assert '#include "sdt_sk_record2.h"' in fmt
    assert "sk_max_run(" not in fmt.replace("(sk_max_run)", ""), "the run cap is defined once, in sdt_sk_record2.h"
    kernels = open(os.path.join(CSRC, "sdt_superkmer_kernels.cuh")).read()
    assert kernels.count("sk_pack2(") == 1 and kernels.count("sk_unpack2(") == 1
    host = open(os.path.join(CSRC, "sdt_pipeline.hip")).read() + open(os.path.join(CSRC, "sdt_pipeline.hpp")).read()
    assert host.count("sk_compact2(") == 1, "one place decides who takes the compact form"
    for fn in ("sk_alloc", "sk_split", "sk_launch_count", "sk_scatter_launch"):
        body = host[host.index(f" {fn}(sdt_ctx *c"):]
        assert "sk_compact(c)" in body[:body.index("\n}\n")], f"{fn} does not ask sk_compact()"
