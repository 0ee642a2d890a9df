"""CPU: the mate overlap exists at every layer (header, library, binding); the Python restatement of the rule (read_overlap_util.py)
-- what the GPU tests expect -- against a second, independently written brute force over strings; the case of
tests/test_read_overlap.py holds what it promises; the pure checks the stage adds to csrc/sdt_read_plan.h and the device-free half of
`sdt-kmers overlap` (csrc/host/overlapsplit.c) as stand-alone programs under AddressSanitizer + UBSan; the refusals of the command
line that need no device."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_overlap_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_overlap_pairs", "sdt_gpu_overlap_pairs_device", "sdt_gpu_overlap_kept_pairs"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("b'[q] = b[Lb - 1 - q] ^ 2", "100 h <= max_err_pct o", "greatest score o - 3 h", "the greatest F wins", "len = min(L, F)",
                  "merging the mates into one read", "needs qualities", "indels", "mate 2 is not reverse-complemented", "any change to clip",
                  "min_overlap 30, max_err_pct 10, min_len 0", "none had an admissible shift", "NO limit on the read length",
                  "an array of sdt_read_overlap through a pointer cast"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+overlap,\s*mismatches,\s*insert,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_overlap;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_overlap,\s*max_err_pct,\s*min_len,\s*flags;\s*\}\s*sdt_overlap_params;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_overlap_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_OVERLAP_DTYPE
    assert dt.itemsize == 24 and dt.names == ru.OVERLAP_FIELDS and dt == ru.OVERLAP_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.OverlapParams) == 16
    assert [(f, getattr(pkg.OverlapParams, f).offset) for f, _ in pkg.OverlapParams._fields_] == [(f, 4 * i) for i, f in enumerate(ru.PARAM_FIELDS)]
    d = pkg.OverlapParams()
    assert {f: getattr(d, f) for f in ru.PARAM_FIELDS} == ru.DEFAULTS           # the defaults of the command line
    assert (pkg.OVERLAP_WHOLE, pkg.OVERLAP_CLIPPED, pkg.OVERLAP_DROPPED) == (ru.WHOLE, ru.CLIPPED, ru.DROPPED) == (pkg.TRIM_WHOLE, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED)
    for m in ("overlap_pairs", "overlap_pairs_device", "overlap_kept_pairs"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def brute_force(a, b, p):
    """the rule once more, over strings: b' is built as text, every d is tried, none is skipped, every admissible shift goes into a list
    and the best is picked from the list -> (the records of a and b, the admissible shifts as (score, F, o, h))"""
    sa = "".join("ACTG"[int(x)] for x in a)
    sb = "".join("ACTG"[int(x)] for x in b)
    bp = sb[::-1].translate(str.maketrans("ACTG", "TGAC"))
    La, Lb = len(sa), len(sb)
    admissible = []
    for d in range(-Lb + 1, La):
        cols = [i for i in range(La) if 0 <= i - d < Lb]
        o = len(cols)
        h = sum(sa[i] != bp[i - d] for i in cols)
        if o >= p["min_overlap"] and 100 * h <= p["max_err_pct"] * o:
            admissible.append((o - 3 * h, d + Lb, o, h))
    o, h, F = (0, 0, 0)
    if admissible:
        _, F, o, h = max(admissible)
    recs = []
    for L in (La, Lb):
        ln = min(L, F) if admissible else L
        recs.append((o, h, F, 0, 0, ru.DROPPED) if ln < max(p["min_len"], 1) else (o, h, F, 0, ln, ru.WHOLE if ln == L else ru.CLIPPED))
    return recs, admissible


def test_restatement_equals_brute_force():
    """the 600 pairs over A and T of 0 .. 90 bases under min_overlap 6 and 15 %: overlaps, ties in score and clipped pairs abound"""
    reads, codes, offs = ru.at_pairs()
    assert len(reads) == 1200 and {int(x) for x in codes.tolist()} == {ru.A, ru.T} and 0 in {len(r) for r in reads} and max(len(r) for r in reads) == 90
    got = ru.at_expect()[0]
    p = ru.AT_PARAMS
    overlapping = ties = clipped = 0
    for t in range(600):
        a, b = reads[2 * t], reads[2 * t + 1]
        want, admissible = brute_force(a, b, p)
        assert [tuple(int(x) for x in got[2 * t + m].tolist()) for m in (0, 1)] == want, f"pair {t}: {a.tolist()} {b.tolist()}"
        if admissible:
            overlapping += 1
            top = max(s for s, _, _, _ in admissible)
            ties += sum(s == top for s, _, _, _ in admissible) > 1
            clipped += any(w[5] == ru.CLIPPED for w in want)
    # the floors of the input; a run of this test counted 198 overlapping pairs
    assert overlapping >= 100 and ties >= 10 and clipped >= 50, (overlapping, ties, clipped)
    # with min_len, on a part of the pairs
    q = dict(p, min_len=25)
    part = ru.expect_overlap(codes[:int(offs[200])], offs[:201], q)[0]
    for t in range(100):
        assert [tuple(int(x) for x in part[2 * t + m].tolist()) for m in (0, 1)] == brute_force(reads[2 * t], reads[2 * t + 1], q)[0]
    assert ru.DROPPED in part["verdict"].tolist()


def test_restatement_on_the_examples_of_the_rule():
    A, C, T, G = ru.A, ru.C, ru.T, ru.G
    frag = [C, T, G, C, A, G, T, C, C, A]
    rc = ru.revcomp(frag).tolist()
    assert rc == [A ^ 2, C ^ 2, C ^ 2, T ^ 2, G ^ 2, A ^ 2, C ^ 2, G ^ 2, T ^ 2, C ^ 2]
    # both mates read through a fragment of 10 into different adapters
    assert ru.pair_overlap(frag + [G, G, A], rc + [T, C, T], 5, 0) == (10, 0, 10)
    assert ru.read_record(13, (10, 0, 10), 0) == (10, 0, 10, 0, 10, ru.CLIPPED)
    # the mates meet in the middle of a longer fragment: insert 14, both whole
    assert ru.pair_overlap(frag, ru.revcomp(frag[4:] + [G, A, T, T]).tolist(), 5, 0) == (6, 0, 14)
    assert ru.read_record(10, (6, 0, 14), 0) == (6, 0, 14, 0, 10, ru.WHOLE)
    # too short an overlap; a mate of no bases
    assert ru.pair_overlap(frag, ru.revcomp(frag[6:] + [G, A, T, T, G, C]).tolist(), 5, 0) == (0, 0, 0)
    assert ru.pair_overlap(frag, [], 1, 100) == (0, 0, 0) and ru.pair_overlap([], [], 1, 100) == (0, 0, 0)
    # one mismatch in ten columns: 10 % admits it, 9 % does not
    bad = list(rc)
    bad[3] ^= 1
    assert ru.pair_overlap(frag, bad, 5, 10) == (10, 1, 10) and ru.pair_overlap(frag, bad, 10, 9) == (0, 0, 0)
    # min_len; a dropped read's record still says what was found
    assert ru.read_record(13, (10, 0, 10), 11) == (10, 0, 10, 0, 0, ru.DROPPED)
    assert ru.read_record(0, (0, 0, 0), 0) == (0, 0, 0, 0, 0, ru.DROPPED)
    # among equal scores the greatest insert wins: ATAT on TATA' fits one base to the left and one to the right
    at = [A, T] * 4
    assert ru.shift_stats(at, ru.revcomp(np.roll(at, 1)), -1) == ru.shift_stats(at, ru.revcomp(np.roll(at, 1)), 1) == (7, 0)
    assert ru.pair_overlap(at, ru.revcomp(np.roll(at, 1)), 6, 0) == (7, 0, 9)


def test_the_case_holds_what_it_says():
    c = ru.case()
    assert len(c["pairs"]) == 40 and len(c["reads"]) == 80 and ru.case_holds() >= 25
    assert max(len(r) for r in c["reads"]) == 2500 and min(len(r) for r in c["reads"]) == 0
    # the other two parameter sets of the GPU test change what is found
    every, exact = ru.case_expect(1, 100)[0], ru.case_expect(30, 0)[0]
    assert (every["insert"] > 0).sum() > (ru.case_expect()[0]["insert"] > 0).sum() > (exact["insert"] > 0).sum() > 0
    # the texts of the command line tool on the case, by hand on its smallest part
    ov = ru.case_expect()[0]
    rec, pairs, single, hist = ru.cli_texts(c["codes"], c["offs"], ov, [(0, len(c["reads"]))])
    assert rec.count("\n") == len(c["reads"]) and pairs.count(">") + single.count(">") == int((ov["len"] > 0).sum())
    inserts = sorted(int(x) for x in ov["insert"][0::2] if x)
    assert hist.splitlines()[-1] == f"# pairs 40 overlapping {len(inserts)} clipped 5 median {inserts[(len(inserts) - 1) // 2]}"
    assert hist.splitlines()[0] == "50 1" and "100 2\n" in hist
    assert ru.cli_texts(c["codes"], c["offs"], ov, [])[3] == "# pairs 0 overlapping 0 clipped 0 median 0\n"


# ---- the pure checks of csrc/sdt_read_plan.h --------------------------------------------------------------------------------------------
def test_parameter_checks_and_shift_span_clean_under_sanitizers(tmp_path):
    """tools/overlap_plan_check.cpp: every refusal, the boundaries 100 / 101 %, the pair ranges, the span of the shifts against a walk
    over every shift; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "overlap_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "overlap_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("overlap_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers overlap` --------------------------------------------------------------------------------------
def test_record_line_and_insert_histogram_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "overlap_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "overlap_host_check.c"), os.path.join(host, "overlapsplit.c")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "overlap_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_overlap(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("overlap",), ("overlap", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers overlap -s lib.cfg -K k", "--min-overlap N, default 30", "--max-err PCT, default 10", "--min-len L, default 0",
                     "prefix.readOverlap", "prefix.overlap.pairs.fa", "prefix.overlap.single.fa", "prefix.insertHist",
                     "overlap mismatches insert start len verdict", "# pairs P overlapping V clipped C median M"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "clip", "query"):
        r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", "--max-err", "10", "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and "--max-err belongs to overlap" in r.stderr, f"{sub}: {r.returncode} {r.stderr[:200]}"
    for opt in (("-a", "x.fa"), ("-g", "x.fa"), ("--tail3", "A"), ("--tail5", "T"), ("--error-pct", "10"), ("--min-tail", "10"), ("--tail-error-pct", "20")):
        r = subprocess.run([exe, "overlap", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and f"{opt[0]} belongs to clip" in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opt, say in ((("--mate-swap",), "--mate-swap belongs to dedup"), (("--target", "5"), "--target belongs to normalize"),
                     (("--min-cov", "5"), "--min-cov belongs to trim")):
        r = subprocess.run([exe, "overlap", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opt, bad, say in (("--max-err", "101", "whole number"), ("--max-err", "x", "whole number"), ("--min-overlap", "0", "at least 1"),
                          ("--min-overlap", "-3", "whole number"), ("--min-len", "-1", "whole number"), ("--min-len", "1e3", "whole number")):
        r = subprocess.run([exe, "overlap", "-s", cfg, "-K", "31", opt, bad, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and opt in r.stderr and say in r.stderr, f"{opt} {bad}: {r.returncode} {r.stderr[:200]}"
    # the options are fine, the library config is not there: refused before the device is touched
    r = subprocess.run([exe, "overlap", "-s", cfg, "-K", "31", "--min-overlap", "20", "--max-err", "100", "--min-len", "0", "-o", out], capture_output=True,
                       text=True)
    assert r.returncode == 255
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
