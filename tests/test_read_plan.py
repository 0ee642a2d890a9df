"""CPU: what the read stages on the counted table decide on the host before anything reaches the device (csrc/sdt_read_plan.h): the
launch geometry of a strip kernel, the check of a host stream, and the cut of a host batch into staged pieces -- with the first test
of the cut's bases cap, which no GPU test can reach (2^29 bases).  tools/read_plan_check.cpp includes that header alone and runs
under AddressSanitizer + UBSan as a stand-alone program; every offsets array it cuts is malloc'ed to exactly the size promised."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")
STAGES = ("sdt_search.hip", "sdt_correct.hip", "sdt_select.hip", "sdt_trim.hip")


def test_geometry_pieces_and_stream_checks_clean_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "read_plan_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"], includes
    assert not re.search(r"#include\s+[<\"](?!stdint\.h)", open(os.path.join(CSRC, "sdt_read_plan.h")).read()), "sdt_read_plan.h is plain C++ over <stdint.h>"
    exe = str(tmp_path / "read_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("read_plan_check: ok"), r.stdout + r.stderr


def test_the_library_uses_this_plan():
    """the read stages must take their geometry, their stream check and their pieces from sdt_read_plan.h through sdt_readstage.hpp (a
    copy of the logic inside a .hip would leave the test above testing nothing)"""
    layer = open(os.path.join(CSRC, "sdt_readstage.hpp")).read()
    assert '#include "sdt_read_plan.h"' in layer
    for call in ("strip_geometry(", "check_stream(", "next_piece("):
        assert call in layer, f"sdt_readstage.hpp does not call {call})"
    plan = open(os.path.join(CSRC, "sdt_read_plan.h")).read()
    texts = {name: open(os.path.join(CSRC, name)).read() for name in STAGES + ("sdt_compact.hpp",)}
    for name in STAGES:
        assert "launch_strip(" in texts[name] and "for_each_piece(" in texts[name], f"{name} launches or stages on its own"
    # each decision is written down once: the refusal, the two stream messages, the state of the kept reads, the cut
    everything = layer + plan + "".join(texts.values())
    for once in ("per-wavefront LDS strip", "offsets not monotonic at read", "packed_words too short", "the reads were not kept"):
        assert everything.count(once) == 1, once
    assert len(re.findall(r"<= (?:piece_bases|PROFILE_CHUNK_BASES)", everything)) == 1, "the bases cap is applied in one place"
    assert not re.search(r"#define \w+_LAUNCH", everything)
