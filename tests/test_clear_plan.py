"""CPU: how much of the node table's clear debt a launch of the level-1 scatter takes along (csrc/sdt_clear_plan.h) -- covered +
remainder = debt for ragged slot counts, no tiles, the cap per tile and slot counts past 2^32, and the kernel's tile loop replayed on a
table of exactly the promised size.  tools/clear_plan_check.cpp includes that header alone and runs under AddressSanitizer + UBSan as a
stand-alone program."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")


def test_clear_plan_clean_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "clear_plan_check.cpp")
    includes = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert includes == ["../soapdenovo-trans_amd/csrc/sdt_clear_plan.h"], includes
    assert not re.search(r"#include\s+[<\"](?!stdint\.h)", open(os.path.join(CSRC, "sdt_clear_plan.h")).read()), "sdt_clear_plan.h is plain C++ over <stdint.h>"
    exe = str(tmp_path / "clear_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("clear_plan_check: ok"), r.stdout + r.stderr


def test_the_library_uses_this_plan():
    """the scatter's host side takes its units per tile and the covered range from plan_clear, and the kernel its unit from the same header"""
    pipe = open(os.path.join(CSRC, "sdt_pipeline.hip")).read()
    launch = pipe[pipe.index("int sk_scatter_launch("):].split("\n}\n", 1)[0]
    assert "plan_clear(c->clear_lo, c->clear_hi," in launch and "clear_cap_units(" in launch and "CLEAR_UNIT_SLOTS" in launch
    kern = open(os.path.join(CSRC, "sdt_sk_scatter_seq.cuh")).read()
    assert '#include "sdt_clear_plan.h"' in kern and "CLEAR_UNIT_SLOTS" in kern[kern.index("sk_clear_tile("):]
    everything = "".join(open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".cuh", ".hpp", ".h")))
    assert len(re.findall(r"^inline ClearPlan plan_clear\(", everything, re.M)) == 1
