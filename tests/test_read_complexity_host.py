"""CPU: the low-complexity filter exists at every layer (header, library, binding); the numpy restatement of the rule
(read_complexity_util.py) -- what the GPU tests expect -- against a second, independently written restatement over strings; the chance
figures of the header at a tenth of their size; the case of tests/test_read_complexity.py holds what it promises; the pure checks the
stage adds to csrc/sdt_read_plan.h and the device-free half of `sdt-kmers complexity` (csrc/host/cxsplit.c) as stand-alone programs
under AddressSanitizer + UBSan; the refusals of the command line that need no device."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_complexity_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_complexity_reads", "sdt_gpu_complexity_reads_device", "sdt_gpu_complexity_kept_reads"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("W = max(1, ceil(L / 32) - 1)", "[32 j, min(32 j + 64, L))", "D_j = sum over t of c_t (c_t - 1)",
                  "100 D_j >= max_score_pct l_j (l_j - 1)", "A homopolymer scores 100", "the first among equals", "100 B > max_low_pct L",
                  "max_low_pct must be 0", "entropy or other scores", "masking bases inside a kept read", "more than one kept stretch per read",
                  "a window other than 64 bases every 32", "pair-aware decisions", "any change to clip, overlap or pass 1",
                  "max_score_pct 10, max_low_pct 50, min_len 0", "a choice, not a measurement", "removes all 64 of its bases",
                  "NO limit on the read length", "an array of sdt_read_complexity through a pointer cast", "arrives as poly-G"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+windows,\s*low,\s*score,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_complexity;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+max_score_pct,\s*max_low_pct,\s*min_len,\s*flags;\s*\}\s*sdt_complexity_params;", src)
    assert re.search(r"#define\s+SDT_COMPLEXITY_TRIM\s+1u", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_complexity_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_COMPLEXITY_DTYPE
    assert dt.itemsize == 24 and dt.names == cu.CX_FIELDS and dt == cu.CX_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.ComplexityParams) == 16
    assert [(f, getattr(pkg.ComplexityParams, f).offset) for f, _ in pkg.ComplexityParams._fields_] == [(f, 4 * i) for i, f in enumerate(cu.PARAM_FIELDS)]
    d = pkg.ComplexityParams()
    assert {f: getattr(d, f) for f in cu.PARAM_FIELDS} == cu.DEFAULTS           # the defaults of the command line
    assert (pkg.COMPLEXITY_WHOLE, pkg.COMPLEXITY_CLIPPED, pkg.COMPLEXITY_DROPPED) == (cu.WHOLE, cu.CLIPPED, cu.DROPPED) == (pkg.TRIM_WHOLE, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED)
    assert pkg.SDT_COMPLEXITY_TRIM == cu.TRIM == 1
    for m in ("complexity_reads", "complexity_reads_device", "complexity_kept_reads"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def by_strings(read, p):
    """the rule once more, over strings: the windows by walking their starts, D as the ordered pairs i != j of equal triplet texts, one
    boolean per base in a list, the clean stretch by a scan -> (the record, the lengths of the clean stretches)"""
    s = "".join("ACTG"[int(x)] for x in read)
    L = len(s)
    low = [False] * L
    windows = nlow = score = 0
    b = 0
    while L > 0 and (b == 0 or b + 32 < L):
        win = s[b:b + 64]
        trips = [win[i:i + 3] for i in range(len(win) - 2)]
        l = len(trips)
        D = sum(trips.count(t) - 1 for t in trips)        # for every i, the j != i with the same three letters
        if l >= 2:
            score = max(score, (100 * D) // (l * (l - 1)))
            if 100 * D >= p["max_score_pct"] * l * (l - 1):
                nlow += 1
                for i in range(b, b + len(win)):
                    low[i] = True
        windows += 1
        b += 32
    stretches, i = [], 0
    while i < L:
        if low[i]:
            i += 1
            continue
        j = i
        while j < L and not low[j]:
            j += 1
        stretches.append((i, j - i))
        i = j
    if p["flags"] & cu.TRIM:
        start, ln = 0, 0
        for st, n in stretches:
            if n > ln:
                start, ln = st, n
    else:
        start, ln = 0, L
        if 100 * sum(low) > p["max_low_pct"] * L:
            ln = 0
    if ln < max(p["min_len"], 1):
        return (windows, nlow, score, 0, 0, cu.DROPPED), [n for _, n in stretches]
    return (windows, nlow, score, start, ln, cu.WHOLE if ln == L else cu.CLIPPED), [n for _, n in stretches]


def test_restatement_equals_the_second_restatement():
    """600 random reads of 0 .. 200 bases, the first 300 over A and T, the others over all four letters, under 20 %, filter (max_low_pct
    50, min_len 20) and trim.  Seed 3 was checked on the CPU against the floors below: 259 reads with a low window, 341 without, and 15
    clipped reads in which two or more clean stretches tie for the longest (seeds 1, 2, 4 and 5 gave 4, 8, 5 and 10 ties)."""
    rng = np.random.default_rng(3)

    def random_read(letters):
        """uniform over the letters, with up to two stretches of 24 .. 40 bases in which nine bases of ten are one letter: uniform
        sequence alone is almost never low under 20 %.  Clean stretches are multiples of 32 bases but for the last, so half of the
        lengths are multiples of 32: there the last stretch can tie with an earlier one"""
        L = 32 * int(rng.integers(0, 7)) if rng.random() < 0.5 else int(rng.integers(0, 201))
        r = rng.choice(letters, size=L)
        for _ in range(int(rng.integers(0, 3))):
            n = int(rng.integers(24, 41))
            at = int(rng.integers(0, max(L - n, 0) + 1))
            n = min(n, L - at)
            r[at:at + n] = np.where(rng.random(n) < 0.9, rng.choice(letters), r[at:at + n])
        return r.astype(np.uint8)

    reads = [random_read([cu.A, cu.T]) for _ in range(300)] + [random_read([cu.A, cu.C, cu.T, cu.G]) for _ in range(300)]
    assert {int(x) for r in reads[:300] for x in r.tolist()} == {cu.A, cu.T} and min(len(r) for r in reads) == 0 and max(len(r) for r in reads) == 200
    codes, offs = cu.concat(reads)
    with_low = without = ties = 0
    for p in (cu.params(max_score_pct=20, min_len=20), cu.params(max_score_pct=20, max_low_pct=0, flags=cu.TRIM)):
        got = cu.expect_complexity(codes, offs, p)[0]
        for r, read in enumerate(reads):
            want, stretches = by_strings(read, p)
            assert tuple(int(x) for x in got[r].tolist()) == want, f"read {r} under {p}: {read.tolist()}"
            if p["flags"] & cu.TRIM:
                with_low += want[1] > 0
                without += want[1] == 0
                ties += want[5] == cu.CLIPPED and stretches.count(max(stretches)) > 1
        assert {cu.WHOLE, cu.DROPPED} <= set(got["verdict"].tolist())
    assert with_low >= 100 and without >= 100 and ties >= 10, (with_low, without, ties)


def test_restatement_on_the_examples_of_the_rule():
    assert cu.windows_of(150) == [(0, 64), (32, 96), (64, 128), (96, 150)] and cu.windows_of(64) == [(0, 64)]
    assert cu.windows_of(65) == [(0, 64), (32, 65)] and cu.windows_of(0) == [] and cu.windows_of(1) == [(0, 1)] and cu.windows_of(33) == [(0, 33)]
    assert all(e - b > 32 for L in range(65, 400) for b, e in cu.windows_of(L)[-1:])
    # a 12-base read with triplet counts (4, 3, 1, 1, 1): D = 4 * 3 + 3 * 2 = 18 of 10 * 9 = 90: exactly 20 %
    read = [cu.A] * 6 + [cu.C] * 5 + [cu.G]               # AAA x4, AAC, ACC, CCC x3, CCG
    assert cu.window_pairs(read) == (18, 10)
    assert cu.complexity_read(read, cu.params(max_score_pct=20))[:3] == (1, 1, 20) and cu.complexity_read(read, cu.params(max_score_pct=21))[:3] == (1, 0, 20)
    assert cu.complexity_read(read, cu.params(max_score_pct=20)) == (1, 1, 20, 0, 0, cu.DROPPED)
    # repeats of period 1 / 2 / 3 / 4 / 6 in a window of 64 bases
    units = ([cu.A], [cu.A, cu.C], [cu.A, cu.C, cu.G], [cu.A, cu.C, cu.T, cu.G], [cu.A, cu.A, cu.C, cu.T, cu.G, cu.C])
    assert [cu.complexity_read(np.resize(np.array(u, dtype=np.uint8), 64), cu.params())[2] for u in units] == [100, 49, 32, 23, 15]
    # reads too short for two triplets have no score and are never low
    for L in (1, 2, 3):
        assert cu.complexity_read([cu.G] * L, cu.params(max_score_pct=1)) == (1, 0, 0, 0, L, cu.WHOLE)
    assert cu.complexity_read([cu.G] * 4, cu.params(max_score_pct=100)) == (1, 1, 100, 0, 0, cu.DROPPED)
    assert cu.complexity_read([], cu.params()) == (0, 0, 0, 0, 0, cu.DROPPED)
    # min_len; a dropped read's record still says what was found
    clean = cu.debruijn3()[:20]                           # no triplet twice
    assert cu.complexity_read(clean, cu.params(min_len=21)) == (1, 0, 0, 0, 0, cu.DROPPED) and cu.complexity_read(clean, cu.params(min_len=20))[3:] == (0, 20, cu.WHOLE)
    # SDT_COMPLEXITY_TRIM keeps the first of two clean stretches of 32 bases around one low window
    tie = np.concatenate([cu.debruijn3()[:54], np.full(30, cu.A, dtype=np.uint8), cu.debruijn3()[22:]]).astype(np.uint8)      # (the next base is A too: 29 x AAA)
    assert len(tie) == 128 and cu.complexity_read(tie, cu.params(max_low_pct=0, flags=cu.TRIM)) == (3, 1, 21, 0, 32, cu.CLIPPED)


def test_chance_figures_at_a_tenth_of_their_size():
    """20 000 random windows per length: the mean score is 1.56 at both lengths, no 64-base window reaches 10"""
    full, short = cu.random_window_scores(20000, 64, 1), cu.random_window_scores(20000, 33, 1)
    print(f"64 bases: mean {full.mean():.3f} max {full.max():.2f}; 33 bases: mean {short.mean():.3f} max {short.max():.2f}, "
          f"{int((short >= 7).sum())} reach 7, {int((short >= 10).sum())} reach 10")
    assert full.max() < 10


def test_the_case_holds_what_it_says():
    c = cu.case()
    assert len(c["reads"]) == 150 and cu.case_holds() >= 25
    assert max(len(r) for r in c["reads"]) == 2100 and min(len(r) for r in c["reads"]) == 0
    # the other parameter sets of the GPU test change what is found
    strict, lax = cu.case_expect(max_score_pct=1)[0], cu.case_expect(max_score_pct=100)[0]
    assert (strict["low"] > 0).sum() > (cu.case_expect()[0]["low"] > 0).sum() > (lax["low"] > 0).sum() >= 10
    assert (lax["score"][lax["low"] > 0] == 100).all()
    # the texts of the command line tool on the case, by hand on their smallest parts
    cx = cu.case_expect()[0]
    rec, pairs, single, hist = cu.cli_texts(c["codes"], c["offs"], cx, [(0, len(c["reads"]))])
    assert rec.count("\n") == len(c["reads"]) and pairs.count(">") + single.count(">") == int((cx["len"] > 0).sum())
    assert hist.splitlines()[-1] == f"# reads 150 low {int((cx['low'] > 0).sum())} dropped {int((cx['verdict'] == 3).sum())} clipped 0"
    assert hist.splitlines()[-2] == f"100 {int((cx['score'] == 100).sum())}" and sum(int(x.split()[1]) for x in hist.splitlines()[:-1]) == 150
    assert cu.cli_texts(c["codes"][:0], c["offs"][:1], cx[:0], [])[3] == "# reads 0 low 0 dropped 0 clipped 0\n"


# ---- the pure checks of csrc/sdt_read_plan.h --------------------------------------------------------------------------------------------
def test_parameter_checks_and_windows_clean_under_sanitizers(tmp_path):
    """tools/complexity_plan_check.cpp: every refusal, the boundaries 100 / 101, the windows of every L up to 300 against a walk over
    every base; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "complexity_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "complexity_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("complexity_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers complexity` -------------------------------------------------------------------------------------
def test_record_line_and_score_histogram_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "complexity_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "complexity_host_check.c"), os.path.join(host, "cxsplit.c")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "complexity_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_complexity(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("complexity",), ("complexity", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers complexity -s lib.cfg -K k", "--max-score P, default 10", "--max-low Q, default 50", "--trim-low",
                     "--min-len L, default 0", "prefix.readComplexity", "prefix.cx.pairs.fa", "prefix.cx.single.fa", "prefix.scoreHist",
                     "windows low score start len verdict", "# reads R low V dropped D clipped C", "a choice, not a measurement",
                     "has 96 low bases and is dropped"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "clip", "overlap", "query"):
        for opt in (("--max-score", "10"), ("--max-low", "50"), ("--trim-low",)):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to complexity" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    for opt, say in ((("-a", "x.fa"), "-a belongs to clip"), (("--tail3", "A"), "--tail3 belongs to clip"), (("--min-overlap", "9"), "--min-overlap belongs to clip"),
                     (("--max-err", "5"), "--max-err belongs to overlap"), (("--mate-swap",), "--mate-swap belongs to dedup"),
                     (("--target", "5"), "--target belongs to normalize"), (("--min-cov", "5"), "--min-cov belongs to trim")):
        r = subprocess.run([exe, "complexity", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opts, say in ((("--max-score", "0"), "--max-score"), (("--max-score", "101"), "--max-score"), (("--max-score", "x"), "--max-score"),
                      (("--max-low", "101"), "--max-low"), (("--max-low", "-1"), "--max-low"), (("--trim-low", "--max-low", "5"), "--max-low 5"),
                      (("--max-low", "5", "--trim-low"), "--max-low 5"), (("--min-len", "1e3"), "--min-len")):
        r = subprocess.run([exe, "complexity", "-s", cfg, "-K", "31", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    # the options are fine, the library config is not there: refused before the device is touched
    for opts in (("--max-score", "100", "--max-low", "100", "--min-len", "0"), ("--max-score", "1", "--trim-low", "--max-low", "0"), ("--trim-low",)):
        r = subprocess.run([exe, "complexity", "-s", cfg, "-K", "31", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and "belongs to" not in r.stderr and "whole number" not in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
