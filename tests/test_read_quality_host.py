"""CPU: the quality trim exists at every layer (header, library, binding); the numpy restatement of the rule in its scan form
(read_quality_util.py) -- what the GPU tests expect -- against the search over every segment and against a plain loop; the spot values
of the rule; the case of tests/test_read_quality.py holds what it promises; the pure checks the stage adds to csrc/sdt_read_plan.h, the
device-free half of `sdt-kmers qtrim` (csrc/host/qualsplit.c) and the parser's quality bytes (csrc/host/seqio.c) as stand-alone
programs under AddressSanitizer + UBSan; the refusals of the command line that need no device."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_quality_util as qu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_quality_reads", "sdt_gpu_quality_reads_device"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_two_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("q_i = 0 if c_i < phred_offset", "min(c_i - phred_offset, 93)", "s_i = q_i - cut_q", "Mott's rule", "the greatest P_b - P_a",
                  "the smallest a wins", "the greatest b", "all s_i < 0 gives a = b = 0", "cut_q = 0 keeps the whole read",
                  "(P_b - M_b descending, a_b ascending, b descending)", "e[q] = 10^6 * 10^(-q / 10) rounded to the nearest integer",
                  "e[20] = 10 000", "e[60..63] = 1, e[64..93] = 0", "no entry is", "summed in 64 bits", "ee_ppm = floor(E / n), 0 for n = 0",
                  "n < max(min_len, 1)", "100 low > max_low_pct n", "max_ee_ppm != 0 and ee_ppm > max_ee_ppm", "the low-base filter is off",
                  "the expected-error filter is off", "phred_offset 33, cut_q 20, low_q 15, max_low_pct 40, max_ee_ppm 0, min_len 0",
                  "a choice, not a measurement", "NO later stage carries qualities along", "does NOT look at the bases",
                  "4-byte aligned and readable up to offsets[nreads] rounded up to 4", "bytes outside the reads never change a result",
                  "NO limit on the read length", "an array of sdt_read_quality through a pointer cast", "sliding-window cuts", "per-end thresholds",
                  "masking bases", "a kept form", "sdt_gpu_keep_reads is\n * not changed", "pair-aware decisions", "any change to another\n * stage",
                  "phred_offset other than 0, 33 or 64", "cut_q > 93; low_q > 93; max_low_pct > 100; flags != 0; reserved != 0"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert "sdt_gpu_quality_kept_reads" not in declared                  # there is no kept form
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+span,\s*low,\s*ee_ppm,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_quality;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+phred_offset,\s*cut_q,\s*low_q,\s*max_low_pct,\s*max_ee_ppm,\s*min_len,\s*flags,\s*reserved;\s*\}"
                     r"\s*sdt_quality_params;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_quality_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_QUALITY_DTYPE
    assert dt.itemsize == 24 and dt.names == qu.Q_FIELDS and dt == qu.Q_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.QualityParams) == 32
    assert [(f, getattr(pkg.QualityParams, f).offset) for f, _ in pkg.QualityParams._fields_] == [(f, 4 * i) for i, f in enumerate(qu.PARAM_FIELDS)]
    d = pkg.QualityParams()
    assert {f: getattr(d, f) for f in qu.PARAM_FIELDS} == qu.DEFAULTS           # the defaults of the command line
    assert (pkg.QUALITY_WHOLE, pkg.QUALITY_CLIPPED, pkg.QUALITY_DROPPED) == (qu.WHOLE, qu.CLIPPED, qu.DROPPED) == (pkg.TRIM_WHOLE, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED)
    for m in ("quality_reads", "quality_reads_device"):
        assert callable(getattr(pkg.PregraphGPU, m))
    assert not hasattr(pkg.PregraphGPU, "quality_kept_reads")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_scan_form_equals_the_search_over_every_segment():
    """2 400 random reads of 0 .. 40 bases with qualities 0 .. 7 under cut_q 0 .. 7: the scan form picks the segment that the search over
    all (a, b) picks.  Seed 1 was run on the CPU: 1 193 of the reads have more than one segment of the greatest sum, so the two tie rules
    decide in half of them; the floor asked for is two thirds of that."""
    rng = np.random.default_rng(1)
    ties = 0
    lengths = set()
    for _ in range(2400):
        L = int(rng.integers(0, 41))
        q = rng.integers(0, 8, L)
        cut = int(rng.integers(0, 8))
        want = qu.segment_brute(q, cut)
        assert qu.segment_scan(q, cut) == want == qu.segment_loop(q, cut), (q.tolist(), cut)
        ties += qu.optimal_segments(q, cut) > 1
        lengths.add(L)
    print(f"{ties} of 2400 reads have more than one optimal segment")
    assert ties >= 800 and lengths == set(range(41))


def test_scan_form_equals_a_plain_loop_on_longer_reads():
    """800 reads of 0 .. 600 bases with the qualities of a sequencer (a plateau that falls off, low 5' ends, runs of quality 2), under
    the defaults and under cut_q 30: the scan form against a loop over b that keeps the minimum and the best key"""
    rng = np.random.default_rng(2)
    clipped = whole = 0
    for i in range(800):
        L = int(rng.integers(0, 601))
        q = qu.realistic(rng, L, i)
        for cut in (20, 30):
            a, b = qu.segment_scan(q, cut)
            assert (a, b) == qu.segment_loop(q, cut), (i, cut)
            whole += b - a == L
            clipped += 0 < b - a < L
        c = (q + 33).astype(np.uint8)
        p = qu.params(min_len=20, max_ee_ppm=20000)
        rec = qu.quality_read(c, p)
        a, b = qu.segment_loop(q, 20)
        seg = [int(x) for x in q[a:b]]
        low, E = sum(x < 15 for x in seg), sum(int(qu.EE_PPM[x]) for x in seg)
        assert rec[:3] == (b - a, low, E // (b - a) if b > a else 0)
        dropped = b - a < 20 or 100 * low > 40 * (b - a) or rec[2] > 20000
        assert rec[3:] == ((0, 0, qu.DROPPED) if dropped else ((0, L, qu.WHOLE) if b - a == L else (a, b - a, qu.CLIPPED)))
    assert clipped >= 400 and whole >= 100, (clipped, whole)


def test_restatement_on_the_spot_values_of_the_rule():
    assert len(qu.EE_PPM) == 94
    assert [int(qu.EE_PPM[q]) for q in (0, 1, 3, 20, 30, 60, 61, 62, 63, 64, 93)] == [1000000, 794328, 501187, 10000, 1000, 1, 1, 1, 1, 0, 0]
    assert (np.diff(qu.EE_PPM) <= 0).all() and (qu.EE_PPM[64:] == 0).all()
    assert qu.quality_of([0, 32, 33, 34, 126, 127, 255], 33).tolist() == [0, 0, 0, 1, 93, 93, 93]
    assert qu.quality_of([0, 63, 64, 104, 157, 158, 255], 64).tolist() == [0, 0, 0, 40, 93, 93, 93]
    assert qu.quality_of([0, 40, 93, 94, 255], 0).tolist() == [0, 40, 93, 93, 93]
    Q = lambda *q: (np.array(q, dtype=np.int64) + 33).astype(np.uint8)
    p = qu.params()
    # all s_i < 0: a = b = 0, nothing measured, dropped even with min_len 0
    assert qu.quality_read(Q(19, 2, 10), p) == (0, 0, 0, 0, 0, qu.DROPPED)
    assert qu.quality_read(Q(), p) == (0, 0, 0, 0, 0, qu.DROPPED)
    # cut_q 0 keeps the whole read
    assert qu.quality_read(Q(0, 0, 40, 0), qu.params(cut_q=0, max_low_pct=100)) == (4, 3, 750025, 0, 4, qu.WHOLE)
    # every base at cut_q: every segment ties, the whole read wins; a base at cut_q at the edge is kept
    assert qu.quality_read(Q(20, 20, 20), p) == (3, 0, 10000, 0, 3, qu.WHOLE)
    assert qu.quality_read(Q(2, 20, 30, 20, 2), p) == (3, 0, 7000, 1, 3, qu.CLIPPED)
    # two maxima of equal sum: the first a; an extension of equal sum to the right: the greatest b
    assert qu.measures(Q(30, 2, 30), p)[:2] == (0, 1) and qu.measures(Q(30, 10, 30, 2), p)[:2] == (0, 3)
    # the three lines of the verdict, in their order, and the record of a dropped read says what was found
    assert qu.quality_read(Q(*[40] * 9), qu.params(min_len=10)) == (9, 0, 100, 0, 0, qu.DROPPED)
    assert qu.quality_read(Q(*[40, 40, 40, 14, 14]), qu.params(cut_q=10)) == (5, 2, 15984, 0, 5, qu.WHOLE)
    assert qu.quality_read(Q(*[40, 40, 14, 14, 14, 40]), qu.params(cut_q=10)) == (6, 3, 19955, 0, 0, qu.DROPPED)
    assert qu.quality_read(Q(*[40, 40, 14, 14, 14, 40]), qu.params(cut_q=10, low_q=0)) == (6, 0, 19955, 0, 6, qu.WHOLE)
    assert qu.quality_read(Q(*[40, 40, 14, 14, 14, 40]), qu.params(cut_q=10, max_low_pct=100, max_ee_ppm=19954)) == (6, 3, 19955, 0, 0, qu.DROPPED)
    assert qu.quality_read(Q(*[40, 40, 14, 14, 14, 40]), qu.params(cut_q=10, max_low_pct=100, max_ee_ppm=19955))[5] == qu.WHOLE
    assert [qu.drop_cause(9, 9, 10 ** 6, qu.params(min_len=10, max_ee_ppm=1)), qu.drop_cause(10, 5, 10 ** 6, qu.params(min_len=10, max_ee_ppm=1)),
            qu.drop_cause(10, 4, 10 ** 6, qu.params(min_len=10, max_ee_ppm=1)), qu.drop_cause(10, 4, 10 ** 6, qu.params(min_len=10))] == ["short", "low", "errors", None]
    # a run of N: quality 2 at the ends is cut, inside it is counted
    assert qu.quality_read(Q(*[2] * 3 + [38] * 30 + [2] * 2 + [38] * 30 + [2] * 5), p)[:2] + qu.quality_read(Q(*[2] * 3 + [38] * 30 + [2] * 2 + [38] * 30 + [2] * 5), p)[3:] \
        == (62, 2, 3, 62, qu.CLIPPED)


def test_the_case_holds_what_it_says():
    c = qu.case()
    assert len(c["reads"]) == 150 and qu.case_holds() >= 30
    assert max(len(r) for r in c["reads"]) == 5000 and min(len(r) for r in c["reads"]) == 0
    # the other parameter sets of the GPU test change what is found
    base = qu.case_expect()[0]
    assert (qu.case_expect(cut_q=0)[0]["verdict"] != qu.CLIPPED).all() and (qu.case_expect(cut_q=0)[0]["span"] == np.diff(c["offs"].astype(np.int64))).all()
    assert (qu.case_expect(cut_q=93)[0]["len"] > 0).sum() == 1            # the read of bytes 255 alone
    assert (qu.case_expect(phred_offset=0)[0]["verdict"] == qu.WHOLE).sum() >= 100 and (qu.case_expect(phred_offset=64)[0]["len"] > 0).sum() <= 3
    drops = [int((qu.case_expect(max_ee_ppm=m)[0]["verdict"] == qu.DROPPED).sum()) for m in (1000, 10000, 100000)]
    assert drops[0] > drops[1] > drops[2] >= 10
    assert (qu.case_expect(max_low_pct=100)[0]["verdict"] == qu.DROPPED).sum() < (base["verdict"] == qu.DROPPED).sum()
    # the texts of the command line tool on the case, by hand on their smallest parts
    rec, pairs, single, hist = qu.cli_texts(c["codes"], c["offs"], base, [(0, len(c["reads"]))], c["params"])
    assert rec.count("\n") == len(c["reads"]) and pairs.count(">") + single.count(">") == int((base["len"] > 0).sum())
    why = qu.causes(base, c["params"])
    assert hist.splitlines()[-1] == (f"# reads 150 whole {int((base['verdict'] == 0).sum())} clipped {int((base['verdict'] == 2).sum())} "
                                     f"dropped {int((base['verdict'] == 3).sum())} short {why.count('short')} low {why.count('low')} errors {why.count('errors')} "
                                     f"bases_in {int(c['offs'][-1])} bases_out {int(base['len'].sum())}")
    assert sum(int(x.split()[1]) for x in hist.splitlines()[:-1]) == int((base["len"] > 0).sum())
    assert qu.cli_texts(c["codes"][:0], c["offs"][:1], base[:0], [], c["params"])[3] == \
        "# reads 0 whole 0 clipped 0 dropped 0 short 0 low 0 errors 0 bases_in 0 bases_out 0\n"


# ---- the pure checks of csrc/sdt_read_plan.h --------------------------------------------------------------------------------------------
def test_parameter_checks_table_and_byte_pieces_clean_under_sanitizers(tmp_path):
    """tools/quality_plan_check.cpp: every refusal and the values next to it, the table of expected errors against the exact integer
    inequality, the byte pieces as a cover of every read; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "quality_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "quality_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("quality_plan_check: ok"), r.stdout + r.stderr
    # the table of the restatement is the table of the header
    plan = open(os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "sdt_read_plan.h")).read()
    body = re.search(r"QUALITY_EE_PPM\[QUALITY_MAX_Q \+ 1\] = \{(.*?)\};", plan, flags=re.S).group(1)
    assert [int(x) for x in re.findall(r"\d+", body)] == qu.EE_PPM.tolist()


# ---- the device-free half of `sdt-kmers qtrim`, and the parser ----------------------------------------------------------------------------
def test_record_line_length_histogram_and_parser_clean_under_sanitizers(tmp_path):
    """tools/quality_host_check.c: qualsplit.c on synthetic records, and a tiny FASTQ through seqio.c with the qualities switched on;
    once with the AVX2 path of the parser and once without it"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "quality_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "quality_host_check.c"), os.path.join(host, "qualsplit.c"),
                                               os.path.join(host, "seqio.c"), "-lpthread"], check=True)
    for extra in ({}, {"SDT_TEST_HOOKS": "1", "SDT_NO_SIMD": "1"}):
        env = {k: v for k, v in os.environ.items() if k != "SDT_NO_SIMD"}
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(env, **extra))
        assert r.returncode == 0 and "quality_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_qtrim(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("qtrim",), ("qtrim", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers qtrim -s lib.cfg -K k", "--phred 33|64, default 33", "--cut-q Q, default 20", "--low-q Q, default 15",
                     "--max-low-bases PCT, default 40", "--max-ee PPM, default 0", "--min-len L, default 0", "prefix.readQual", "prefix.qtrim.pairs.fa",
                     "prefix.qtrim.single.fa", "prefix.lenHist", "span low ee_ppm start len verdict",
                     "# reads R whole W clipped C dropped D short S low V errors X bases_in I bases_out O", "a choice, not a measurement",
                     "FASTQ libraries only"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "clip", "overlap", "complexity", "query"):
        for opt in (("--phred", "33"), ("--cut-q", "20"), ("--low-q", "15"), ("--max-low-bases", "40"), ("--max-ee", "0")):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"{opt[0]} belongs to qtrim" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    for opt, say in ((("-a", "x.fa"), "-a belongs to clip"), (("--tail3", "A"), "--tail3 belongs to clip"), (("--max-err", "5"), "--max-err belongs to overlap"),
                     (("--mate-swap",), "--mate-swap belongs to dedup"), (("--target", "5"), "--target belongs to normalize"),
                     (("--min-cov", "5"), "--min-cov belongs to trim"), (("--max-score", "5"), "--max-score belongs to complexity"),
                     (("--max-low", "5"), "--max-low belongs to complexity"), (("--trim-low",), "--trim-low belongs to complexity")):
        r = subprocess.run([exe, "qtrim", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opts, say in ((("--phred", "0"), "--phred"), (("--phred", "34"), "--phred"), (("--phred", "65"), "--phred"), (("--phred", "x"), "--phred"),
                      (("--cut-q", "94"), "--cut-q"), (("--cut-q", "-1"), "--cut-q"), (("--low-q", "94"), "--low-q"), (("--max-low-bases", "101"), "--max-low-bases"),
                      (("--max-ee", "4294967296"), "--max-ee"), (("--max-ee", "1e4"), "--max-ee"), (("--min-len", "1e3"), "--min-len")):
        r = subprocess.run([exe, "qtrim", "-s", cfg, "-K", "31", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opts}: {r.returncode} {r.stderr[:200]}"
    # the options are fine, the library config is not there: refused before the device is touched
    for opts in (("--phred", "64", "--cut-q", "93", "--low-q", "93", "--max-low-bases", "100", "--max-ee", "4294967295", "--min-len", "0"),
                 ("--phred", "33", "--cut-q", "0", "--low-q", "0", "--max-low-bases", "0")):
        r = subprocess.run([exe, "qtrim", "-s", cfg, "-K", "31", *opts, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and "belongs to" not in r.stderr and "whole number" not in r.stderr
    # a library with a FASTA file is refused before the device is touched and before anything is written
    (tmp_path / "r.fa").write_text(">a\nACGT\n")
    (tmp_path / "r.fq").write_text("@a\nACGT\n+\nIIII\n")
    for line in ("f", "f1", "p"):
        (tmp_path / "lib.cfg").write_text(f"max_rd_len=100\n[LIB]\navg_ins=200\nasm_flags=1\nq={tmp_path / 'r.fq'}\n{line}={tmp_path / 'r.fa'}\n")
        r = subprocess.run([exe, "qtrim", "-s", str(tmp_path / "lib.cfg"), "-K", "31", "-o", out], capture_output=True, text=True)
        assert r.returncode not in (0, 255) and "qtrim needs base qualities" in r.stderr and "r.fa" in r.stderr, f"{line}=: {r.returncode} {r.stderr[:200]}"
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
