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
    # (a stage with records and a keep mask stages through staged_records, which is the layer's own for_each_piece body)
    assert "for_each_piece(" in layer[layer.index("static int staged_records("):].split("\n}\n", 1)[0]
    for name in STAGES:
        assert "launch_strip(" in texts[name] and ("for_each_piece(" in texts[name] or "staged_records<" in texts[name]), \
            f"{name} launches or stages on its own"
        assert "next_piece(" not in texts[name], f"{name} cuts its pieces on its own"
    # each decision is written down once: the refusal, the two stream messages, the state of the kept reads, the cut
    everything = layer + plan + "".join(texts.values())
    for once in ("per-wavefront LDS strip", "offsets not monotonic at read", "packed_words too short", "the reads were not kept"):
        assert everything.count(once) == 1, once
    assert len(re.findall(r"<= (?:piece_bases|PROFILE_CHUNK_BASES)", everything)) == 1, "the bases cap is applied in one place"
    assert not re.search(r"#define \w+_LAUNCH", everything)
    # the grid of the kernels that give every wavefront a read is decided once, in wave_blocks of sdt_read_plan.h, and its three
    # users go through it with the value of SDT_WAVE_BLOCKS: wave_grid, the strip geometry (through strip_plan), the launch of
    # k_align_reads
    body = lambda text, head: text[text.index(head):].split("\n}\n", 1)[0]
    assert len(re.findall(r"^constexpr uint32_t wave_blocks\(", plan, re.M)) == 1
    assert "wave_blocks(" in body(plan, "inline StripGeometry strip_geometry(")
    assert "wave_blocks(" in body(layer, "static int wave_grid(") and "wave_blocks_forced()" in body(layer, "static int wave_grid(")
    assert re.search(r"strip_geometry\([^;]*wave_blocks_forced\(\)\);", body(layer, "static int strip_plan("))
    mapstage = open(os.path.join(CSRC, "sdt_mapstage.hip")).read()
    launch = body(mapstage, "static int launch_align(")
    assert '#include "sdt_read_plan.h"' in mapstage
    assert re.search(r"blocks = wave_blocks\([^;]*wave_blocks_forced\(\)\);", launch) and "k_align_reads<NWV>, dim3(blocks)" in launch
    stage_units = [n for n in sorted(os.listdir(CSRC)) if re.match(r"sdt_(search|correct|select|trim|dedup|clip|overlap|complexity|quality|screen|mapstage)\w*\.(hip|cuh|hpp|h)$", n)]
    cap = "".join(open(os.path.join(CSRC, n)).read() for n in stage_units + ["sdt_readstage.hpp", "sdt_read_plan.h", "sdt_compact.hpp"])
    assert len(re.findall(r"cu_count \* 32", re.sub(r"//.*", "", cap))) == 1, "the cap of the grid is applied in one place"
    assert cap.count('sdt_test_env("SDT_WAVE_BLOCKS")') == 0 and open(os.path.join(CSRC, "sdt_ctx.hpp")).read().count('sdt_test_env("SDT_WAVE_BLOCKS")') == 1
