"""CPU: the growth schedule of the layout replay (csrc/sdt_layout_plan.h) as a stand-alone program under AddressSanitizer + UBSan --
against a simulation that makes every put, and against the growth lines the reference's own tables left in the unit fixtures."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
FIXTURES = ["unit_31.txt", "unit_63.txt", "unit_127.txt"]


def recorded_lines():
    """the `init size max`, `grow count size max` and `prime n next` lines of the fixtures, each once, as arguments"""
    lines = []
    for name in FIXTURES:
        got = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", name)) if re.match(r"(init|grow|prime) \d", ln)]
        assert {"init", "grow", "prime"} <= {g[0] for g in got}, name
        lines += [g for g in got if g not in lines]
    return lines


def test_fixtures_record_the_first_growth():
    lines = recorded_lines()
    assert ["init", "1031", "793"] in lines and ["grow", "793", "2063", "1588"] in lines


def test_growth_schedule_clean_under_sanitizers(tmp_path):
    """tools/layout_plan_check.cpp: generations of sets of 0 .. 2.1e8 keys from both initial sizes == a put-by-put simulation, the
    two limit refusals, the list capacity, the fixtures' lines; includes sdt_layout_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "layout_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_layout_plan.h"]
    plan = open(os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "sdt_layout_plan.h")).read()
    assert "hip" not in " ".join(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", plan)).lower()
    exe = str(tmp_path / "layout_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    lines = recorded_lines()
    r = subprocess.run([exe] + [w for ln in lines for w in ln], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith(f"layout_plan_check: ok ({len(lines)} recorded lines)"), r.stdout + r.stderr
    # a line that the rule does not give is noticed
    r = subprocess.run([exe, "grow", "793", "2063", "1587"], capture_output=True, text=True)
    assert r.returncode == 1 and "no generation [793, 1587) in 2063 slots" in r.stderr
