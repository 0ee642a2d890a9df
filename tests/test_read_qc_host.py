"""CPU: the QC report exists at every layer (header, library, binding); the numpy restatement of the rule (read_qc_util.py) -- what
the GPU tests expect -- against a second one, base by base in plain Python; the kernel's lane walk, restated, against the rule on the
case; the case holds what it promises; the pure checks the stage adds to csrc/sdt_read_plan.h and the device-free half of
`sdt-kmers qc` (csrc/host/qcsplit.c) as stand-alone programs under AddressSanitizer + UBSan; the command line's refusals that need no
device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import read_qc_util as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_qc_report_words", "sdt_gpu_qc_reads", "sdt_gpu_qc_reads_device"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("THE CALL ADDS TO THE REPORT", "203 + 99 R", "row = min(i, C)", "row = min(n - 1 - i, C)", "totals[4]", "floor(100 (#C + #G) / n)",
                  "floor(sum of q / n)", "untouched when quals is NULL", "report(A ++ B) =", "d_report not 8-byte aligned", "class_sel > 255",
                  "NO limit on the read length", "a kept form", "HTML or plots"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared and hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+cycles,\s*phred_offset,\s*flags,\s*class_sel,\s*reserved;\s*\}\s*sdt_qc_params;", src)
    assert "#define SDT_ABI_VERSION 8" in src and "#define SDT_QC_MAX_CYCLES 4096" in src and re.search(r"#define SDT_QC_FROM_END\s+1u", src)


def test_binding_is_the_c_layout(pkg):
    assert ctypes.sizeof(pkg.QcParams) == 20
    assert [(f, getattr(pkg.QcParams, f).offset) for f, _ in pkg.QcParams._fields_] == [(f, 4 * i) for i, f in enumerate(
        ("cycles", "phred_offset", "flags", "class_sel", "reserved"))]
    d = pkg.QcParams()
    assert (d.cycles, d.phred_offset, d.flags, d.class_sel, d.reserved) == (1024, 33, 0, 0, 0)      # the defaults of the command line
    assert (pkg.QC_MAX_CYCLES, pkg.QC_FROM_END, pkg.QC_QUALS, pkg.QC_GC_BINS, pkg.QC_TOTALS) == (4096, qc.FROM_END, qc.QUALS, qc.GC_BINS, qc.TOTALS)
    for C in (1, 150, 4096):
        assert pkg.qc_report_words(C) == qc.report_words(C)
        rep = np.arange(qc.report_words(C), dtype=np.uint64)
        mine, theirs = pkg.qc_sections(rep, C), qc.sections(rep, C)
        assert list(mine) == ["totals", "base", "qual", "len", "gc", "meanq"]
        assert all(mine[k].shape == theirs[k].shape and (mine[k] == theirs[k]).all() and mine[k].base is not None for k in mine)
    assert pkg.qc_report_words(0) == 0 and pkg.qc_report_words(4097) == 0
    for m in ("qc_reads", "qc_reads_device"):
        assert callable(getattr(pkg.PregraphGPU, m))
    assert qc.RANGE_DTYPE == pkg.READ_TRIM_DTYPE


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_case_holds_what_it_says():
    assert qc.case_holds() >= 20


def test_numpy_restatement_equals_the_loop_base_by_base():
    """50 reads of the case that cover its lengths up to 450 bases, under several cycles, both directions, with and without qualities,
    ranges and classes, and with the device form's clamp on ranges that overrun"""
    c = qc.case()
    pick = [int(np.nonzero(c["lens"] == L)[0][0]) for L in qc.LENGTHS] + list(range(30))
    codes, offs = qc.concat([c["reads"][r] for r in pick])
    quals = np.concatenate([c["qreads"][r] for r in pick])
    ranges, classes = c["ranges"][pick], c["classes"][pick]
    assert len(pick) == 50
    over = ranges.copy()
    over["len"][::3] += 7
    over["start"][5::11] += 500
    for C in (1, 7, 150, 500):
        for flags in (0, qc.FROM_END):
            for kw in (dict(), dict(quals=quals), dict(quals=quals, ranges=ranges), dict(quals=quals, ranges=ranges, classes=classes, class_sel=2),
                       dict(quals=quals, phred_offset=64), dict(quals=quals, phred_offset=0), dict(quals=quals, ranges=over, clamp=True)):
                a = qc.expect(codes, offs, cycles=C, flags=flags, **kw)
                b = qc.expect_loop(codes, offs, cycles=C, flags=flags, **kw)
                qc.assert_report(a, b, C, f"cycles = {C}, flags = {flags}, {sorted(kw)}")
                qc.identities(a, C, "quals" in kw)
    assert qc.expect(codes, offs, quals, over, cycles=7, clamp=True)[4] >= 15


def test_lane_walk_of_the_kernel_equals_the_rule(synth):
    """what the lanes of k_qc_reads load and count, pass by pass: tiles of 152 and of 5 rows, both directions, several grids, a delta
    between the bytes and the bases as the host form's pieces have it; and no word or quality word without a counted base is loaded"""
    c = qc.case()
    words = qc.pack(synth, c["codes"])
    qbuf = np.concatenate([c["quals"], np.zeros(8, dtype=np.uint8)])
    for C, tile, blocks, waves in ((150, qc.TILE, 2, 16), (150, 5, 3, 4), (7, 5, 1, 16), (1, qc.TILE, 2, 2), (400, qc.TILE, 2, 16), (151, 151, 1, 1)):
        for flags in (0, qc.FROM_END):
            got = qc.lane_walk(words, qbuf, c["offs"], c["ranges"], None, cycles=C, flags=flags, tile=tile, blocks=blocks, waves=waves)
            qc.assert_report(got, qc.case_expect(cycles=C, flags=flags), C, f"cycles = {C}, tile = {tile}, flags = {flags}")
    got = qc.lane_walk(words, None, c["offs"], None, c["classes"], cycles=150, class_sel=1)
    qc.assert_report(got, qc.case_expect(quals=False, ranges=False, classes=True, class_sel=1), 150, "without qualities, by class")
    # the bytes 8 further on than the bases: delta = 8
    shifted = np.concatenate([np.full(8, 255, dtype=np.uint8), qbuf])
    for flags in (0, qc.FROM_END):
        got = qc.lane_walk(words, shifted, c["offs"], c["ranges"], None, cycles=150, flags=flags, delta=8)
        qc.assert_report(got, qc.case_expect(flags=flags), 150, "delta = 8")
    # a batch whose only counted bases are bases [37, 41) of a read of 100: one word of the stream, two quality words at most
    codes, offs = qc.concat([np.arange(100, dtype=np.uint8) & 3])
    rg = np.zeros(1, dtype=qc.RANGE_DTYPE)
    rg["start"], rg["len"] = 37, 4
    touched = {}
    got = qc.lane_walk(qc.pack(synth, codes), np.full(104, 40, dtype=np.uint8), offs, rg, None, cycles=2, touched=touched)
    qc.assert_report(got, qc.expect(codes, offs, np.full(100, 40, dtype=np.uint8), rg, cycles=2), 2, "four bases")
    assert touched["words"] == {2} and touched["quals"] == {9, 10}


# ---- the pure checks of csrc/sdt_read_plan.h, and the device-free half of `sdt-kmers qc` --------------------------------------------------
def test_parameter_checks_layout_and_grid_clean_under_sanitizers(pkg, tmp_path):
    """tools/qc_plan_check.cpp: every refusal and the values next to it, the layout against the table of the rule, the grid; includes
    sdt_read_plan.h alone.  The tile rows it prints are those the binding and the tests restate"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "qc_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "qc_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == f"qc_plan_check: ok tile {pkg.QC_TILE} waves 16\n", r.stdout + r.stderr
    assert qc.TILE == pkg.QC_TILE


def test_the_three_files_and_the_summary_clean_under_sanitizers(tmp_path):
    """tools/qc_host_check.c: qcsplit.c on hand-made reports"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "qc_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "qc_host_check.c"), os.path.join(host, "qcsplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "qc_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_cli_texts_of_the_restatement_on_a_hand_made_report():
    """the Python twin of qcsplit.c gives the texts that tools/qc_host_check.c holds the C code to"""
    C = 3
    r0 = np.zeros(qc.report_words(C), dtype=np.uint64)
    s = qc.sections(r0, C)
    s["totals"][:3] = (4, 1, 9)
    s["base"][0, :2], s["base"][1, 3], s["base"][2, 2], s["base"][3, 1] = (2, 1), 2, 1, 3
    s["qual"][0, 30], s["qual"][0, 2], s["qual"][1, 20], s["qual"][1, 21], s["qual"][2, 40], s["qual"][3, 0], s["qual"][3, 93] = 2, 1, 1, 1, 1, 1, 2
    s["len"][:] = 1
    s["gc"][[0, 50, 100]] = 1
    s["meanq"][[2, 25, 60]] = 1
    r2 = np.zeros(qc.report_words(C), dtype=np.uint64)
    t = qc.sections(r2, C)
    t["totals"][0], t["totals"][2], t["base"][0, 0], t["base"][0, 3], t["len"][1], t["gc"][0], t["gc"][100] = 2, 2, 1, 1, 2, 1, 1
    bases, quals, reads, lines = qc.cli_texts({0: r0, 2: r2}, {0: True, 2: False}, C)
    assert bases == "# class row reads A C T G\n0 0 3 2 1 0 0\n0 1 2 0 0 0 2\n0 2 1 0 0 1 0\n0 3+ 3 0 3 0 0\n2 0 2 1 0 0 1\n"
    assert quals == ("# class row bases mean_x100 min q10 q25 median q75 q90 max\n0 0 3 2066 2 2 2 30 30 30 30\n0 1 2 2050 20 20 20 20 21 21 21\n"
                     "0 2 1 4000 40 40 40 40 40 40 40\n0 3+ 3 6200 0 0 0 93 93 93 93\n# class 2: no qualities\n")
    assert reads == ("# hist class bin reads\nlen 0 0 1\nlen 0 1 1\nlen 0 2 1\nlen 0 3+ 1\nlen 2 1 2\ngc 0 0 1\ngc 0 50 1\ngc 0 100 1\ngc 2 0 1\ngc 2 100 1\n"
                     "meanq 0 2 1\nmeanq 0 25 1\nmeanq 0 60 1\n# meanq class 2: no qualities\n")
    assert lines == "qc: class 0 reads 4 empty 1 bases 9 gc 6666 q20 7777 q30 5555\nqc: class 2 reads 2 empty 0 bases 2 gc 5000 q20 - q30 -\n"


def test_sdt_kmers_usage_knows_qc(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "qc"], capture_output=True, text=True)
    assert r.returncode == 255
    for word in ("sdt-kmers qc -s lib.cfg -K k [-p threads] [--cycles C, default 1024] [--phred 33|64, default 33] [--from-end] -o prefix",
                 "prefix.qcBases", "prefix.qcQuals", "prefix.qcReads", "# class row reads A C T G", "# class row bases mean_x100 min q10 q25 median q75 q90 max",
                 "# hist class bin reads", "written as C+", "qc: class K reads R empty E bases B gc G q20 X q30 Y", "ceil(p * bases / 100)",
                 "# class K: no qualities"):
        assert word in r.stderr, f"the usage text lacks {word!r}"
    cfg, out = str(tmp_path / "none.cfg"), str(tmp_path / "out")     # (never opened: the options are refused first)
    for opts, say in ((("--cycles", "0"), "--cycles"), (("--cycles", "4097"), "--cycles"), (("--cycles", "x"), "--cycles"), (("--phred", "0"), "--phred"),
                      (("--cut-q", "20"), "--cut-q belongs to qtrim"), (("--low-q", "2"), "--low-q belongs to qtrim"), (("--tail3", "A"), "--tail3 belongs to clip"),
                      (("--min-len", "5"), "--min-len belongs to trim, clip, overlap, complexity and qtrim")):
        r = subprocess.run([exe, "qc", "-s", cfg, "-K", "31", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    for sub in ("profile", "qtrim", "clip", "merge"):
        for opt in (("--cycles", "100"), ("--from-end",)):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to qc" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    # the options are fine, the library config is not there
    r = subprocess.run([exe, "qc", "-s", cfg, "-K", "31", "--cycles", "4096", "--phred", "64", "--from-end", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "belongs to" not in r.stderr and "whole number" not in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
