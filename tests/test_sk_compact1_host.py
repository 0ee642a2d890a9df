"""CPU: the 16-byte compact level-1 record of 1-word keys without ordinals (csrc/sdt_sk_record1.h) -- pack / unpack round trips for
every K in 17..31, level-2 buckets of 10..12 bits, every run length up to the cap and all context flags, zero padding bits, a run cap
that never admits a run that does not fit, and the step to the compact level-2 record bit for bit what sk_pack2 makes of the 24-byte
record of the same run.  tools/sk_compact1_check.cpp includes the two record headers alone and runs under UBSan as a stand-alone
program."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")


def test_pack_unpack_convert_and_run_cap_clean_under_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "sk_compact1_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert sorted(includes) == ["../soapdenovo-trans_amd/csrc/sdt_sk_record1.h", "../soapdenovo-trans_amd/csrc/sdt_sk_record2.h"], includes
    hdr = open(os.path.join(CSRC, "sdt_sk_record1.h")).read()
    assert not re.search(r"#include\s+[<\"](?!stdint\.h|sdt_sk_record2\.h)", hdr), "sdt_sk_record1.h is plain C++ over <stdint.h> and the level-2 record's header"
    exe = str(tmp_path / "sk_compact1_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("sk_compact1_check: ok"), r.stdout + r.stderr


def test_the_library_uses_these_functions():
    """level 1, level 2 and the host take the format, the cap and the record size from sdt_sk_record1.h (a copy of the logic inside a
    kernel would leave the test above testing nothing), and one host function gives the words of a level-1 record"""
    fmt = open(os.path.join(CSRC, "sdt_superkmer.cuh")).read()
    assert '#include "sdt_sk_record1.h"' in fmt
    seq = open(os.path.join(CSRC, "sdt_sk_scatter_seq.cuh")).read()
    kernels = open(os.path.join(CSRC, "sdt_superkmer_kernels.cuh")).read()
    # both level-1 kernels store through sk_store_record1, the one place that packs
    assert seq.count("sk_pack1(") == 1 and "sk_pack1(" not in kernels
    assert seq.count("sk_store_record1<NW, C1>(") == 1 and kernels.count("sk_store_record1<NW, C1>(") == 1
    assert kernels.count("sk_rec1c_to_rec2c(") == 1, "level 2 converts with sk_rec1c_to_rec2c"
    for text in (seq, kernels, fmt):
        assert "sk_max_run1(" not in text, "the cap comes from the host, which asks sdt_sk_record1.h"
    hpp = open(os.path.join(CSRC, "sdt_pipeline.hpp")).read()
    host = open(os.path.join(CSRC, "sdt_pipeline.hip")).read()
    sharded = open(os.path.join(CSRC, "sdt_sharded.hip")).read()
    assert (hpp + host + sharded).count("sk_compact1(") == 1, "one place decides who takes the compact level-1 form"
    assert "sk_rec1_words(const sdt_ctx *c)" in hpp
    assert "sk_rec_words(c->nw)" not in host + sharded, "a level-1 record's size is asked of sk_rec1_words(c)"
    assert sharded.count("sk_rec1_words(c)") >= 3 and host.count("sk_rec1_words(c)") >= 1
    body = host[host.index(" sk_scatter_launch(sdt_ctx *c"):]
    assert "sk_max_run1(" in body[:body.index("\n}\n")], "the level-1 scatter's cap is sk_max_run1"
