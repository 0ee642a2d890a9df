"""CPU: the merge of overlapping mates and the compaction of quality bytes exist at every layer (header, library, binding); the Python
restatement of the rule (read_merge_util.py) -- what the GPU tests expect -- against a second, independently written brute force over
strings; the error-free property over a grid of mate lengths and inserts; the case of tests/test_read_merge.py holds what it promises;
the pure checks the stage adds to csrc/sdt_read_plan.h and the device-free half of `sdt-kmers merge` (csrc/host/mergesplit.c) as
stand-alone programs under AddressSanitizer + UBSan; the refusals of the command line that need no device."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_merge_util as mu
import read_overlap_util as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_merge_pairs", "sdt_gpu_merge_pairs_device", "sdt_gpu_merge_kept_pairs", "sdt_gpu_compact_quals_trimmed",
           "sdt_gpu_compact_quals_trimmed_device"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_five_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("b'[q] = b[Lb - 1 - q] ^ 2", "Fa == Fb", "1 <= F < La + Lb", "max(min_len, 1) <= F", "max_len == 0 or F <= max_len",
                  "INCONSISTENT", "never reads outside the two mates", "m[p] = a[p]", "m[p] = b'[p - d]", "A tie goes to mate 1", "counts in from_b",
                  "c < phred_offset gives 0, else min(c - phred_offset, 93)", "verdict = 5 (SDT_MERGE_MERGED)",
                  "of the pairs that did not merge", "ascending pair index", "(offsets[nreads] - offsets[0] + 15) /",
                  "16 + 4 words always suffice", "2 048 bases at a time", "min_len 0, max_len 0 (no limit), phred_offset 33",
                  "zero-padded to a multiple of 4 bytes", "are not written", "qualities of the merged read", "merging without an overlap record",
                  "a kept form with", "any change to overlap, quality or the compaction calls",
                  # the two exclusions that went here are still where they were said
                  "merging the mates into one read", "NO later stage carries qualities along", "they went here"):
        assert words in src, f"include/sdt_gpu.h does not say {words!r}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+merged,\s*mismatches,\s*from_b,\s*start,\s*len,\s*verdict;\s*\}\s*sdt_read_merge;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_len,\s*max_len,\s*phred_offset,\s*flags;\s*\}\s*sdt_merge_params;", src)
    assert re.search(r"#define\s+SDT_MERGE_MERGED\s+5u", src)
    assert "#define SDT_ABI_VERSION 8" in src and lib.sdt_gpu_abi_version() == 8


def test_read_merge_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_MERGE_DTYPE
    assert dt.itemsize == 24 and dt.names == mu.MERGE_FIELDS and dt == mu.MERGE_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    # start, len and verdict sit where sdt_read_trim has them: compact_trimmed takes the records as they are
    for f in ("start", "len", "verdict"):
        assert dt.fields[f][1] == pkg.READ_TRIM_DTYPE.fields[f][1] == pkg.READ_OVERLAP_DTYPE.fields[f][1]
    assert dt.itemsize == pkg.READ_TRIM_DTYPE.itemsize
    assert ctypes.sizeof(pkg.MergeParams) == 16
    assert [(f, getattr(pkg.MergeParams, f).offset) for f, _ in pkg.MergeParams._fields_] == [(f, 4 * i) for i, f in enumerate(mu.PARAM_FIELDS)]
    d = pkg.MergeParams()
    assert {f: getattr(d, f) for f in mu.PARAM_FIELDS} == mu.DEFAULTS           # the defaults of the command line
    assert pkg.MERGE_MERGED == mu.MERGED == 5 and mu.MERGED not in (pkg.TRIM_WHOLE, pkg.TRIM_GATED, pkg.TRIM_TRIMMED, pkg.TRIM_DROPPED, pkg.TRIM_SHORT)
    for m in ("merge_pairs", "merge_pairs_device", "merge_kept_pairs", "compact_quals_trimmed", "compact_quals_trimmed_device"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def brute_force(a, b, qa, qb, F, phred):
    """the rule once more, over strings: b' and its qualities are built as text and list, both mates are laid out on a line of F
    positions with gaps, and every position is read off the line -> (the merged read as text, mismatch columns, from_b)"""
    sa = "".join("ACTG"[int(x)] for x in a)
    bp = "".join("ACTG"[int(x)] for x in b)[::-1].translate(str.maketrans("ACTG", "TGAC"))
    d = F - len(bp)
    q = lambda c: 0 if c < phred else min(c - phred, 93)
    row_a = [(sa[p], q(int(qa[p])) if qa is not None else None) if p < len(sa) else None for p in range(F)]
    row_b = [None] * F
    for i, ch in enumerate(bp):
        if 0 <= i + d < F:
            row_b[i + d] = (ch, q(int(qb[::-1][i])) if qb is not None else None)
    out, mism, from_b = [], 0, 0
    for x, y in zip(row_a, row_b):
        assert x or y
        if x and y and x[0] != y[0]:
            mism += 1
            take_b = qa is not None and y[1] > x[1]
            from_b += take_b
            out.append(y[0] if take_b else x[0])
        else:
            out.append((x or y)[0])
    return "".join(out), mism, from_b


def test_restatement_equals_brute_force():
    """the 600 pairs over A and T under the overlap records of the overlap rule, without qualities and with random ones"""
    reads, codes, offs = ro.at_pairs()
    ov = ro.at_expect()[0]
    quals = mu.at_quals()
    for with_quals in (False, True):
        mg, out = mu.at_expect(with_quals)
        j = 0
        for t in range(600):
            a, b = reads[2 * t], reads[2 * t + 1]
            F = int(ov["insert"][2 * t])
            if not F:
                assert mg[2 * t].tolist() == (0, 0, 0) + tuple(ov[2 * t].tolist())[3:] and mg[2 * t + 1].tolist() == (0, 0, 0) + tuple(ov[2 * t + 1].tolist())[3:]
                continue
            qa = quals[int(offs[2 * t]):int(offs[2 * t + 1])] if with_quals else None
            qb = quals[int(offs[2 * t + 1]):int(offs[2 * t + 2])] if with_quals else None
            text, mism, from_b = brute_force(a, b, qa, qb, F, 33)
            assert mg[2 * t].tolist() == mg[2 * t + 1].tolist() == (F, mism, from_b, 0, 0, mu.MERGED), f"pair {t}"
            assert "".join("ACTG"[int(x)] for x in out[j]) == text, f"pair {t}"
            assert mism == int(ov["mismatches"][2 * t])              # recounted by this stage: what the overlap counted
            j += 1
        assert j == len(out) >= 100
    # the limits, on the same pairs: every F below 40 or above 120 stays apart
    lim = mu.params(min_len=40, max_len=120)
    mg, out = mu.expect_merge(codes, offs, ov, lim)
    inserts = ov["insert"][0::2]
    assert [len(m) for m in out] == [int(F) for F in inserts if 40 <= F <= 120] and 0 < len(out) < int((inserts > 0).sum())
    assert ((mg["merged"] == 0) == ~np.isin(mg["verdict"], [mu.MERGED])).all()


def test_error_free_mates_merge_into_their_fragment():
    """mates cut from a random fragment with different adapters behind it: the merged read is the fragment, whatever the qualities say,
    over the grid of mate lengths and every insert that crosses a boundary of them"""
    rng = np.random.default_rng(20250612)
    lens = [L for L in mu.MATE_LENGTHS if L]
    combos = 0
    for La in lens:
        for Lb in lens:
            marks = {1, 2, La - 1, La, La + 1, Lb - 1, Lb, Lb + 1, La + Lb - 2, La + Lb - 1, (La + Lb) // 2, 31, 32, 33, 64}
            for F in sorted(f for f in marks if 1 <= f < La + Lb):
                frag = rng.integers(0, 4, size=F, dtype=np.uint8)
                pad = lambda n: rng.integers(0, 4, size=max(n, 0), dtype=np.uint8)
                a = np.concatenate([frag, pad(La - F)])[:La]
                b = np.concatenate([ro.revcomp(frag), pad(Lb - F)])[:Lb]
                assert mu.merge_decide(La, Lb, F, F, 0, 0) == F
                qa, qb = rng.integers(33, 80, size=La, dtype=np.uint8), rng.integers(33, 80, size=Lb, dtype=np.uint8)
                for q in ((None, None), (qa, qb)):
                    m, mism, from_b = mu.merge_pair(a, b, F, q[0], q[1])
                    assert (m == frag).all() and mism == 0 and from_b == 0, (La, Lb, F)
                assert brute_force(a, b, qa, qb, F, 33) == ("".join("ACTG"[int(x)] for x in frag), 0, 0)
                combos += 1
            assert mu.merge_decide(La, Lb, La + Lb, La + Lb, 0, 0) == mu.INCONSISTENT
    assert combos >= 800, combos


def test_restatement_on_the_examples_of_the_rule():
    A, C, T, G = ro.A, ro.C, ro.T, ro.G
    frag = [C, T, G, C, A, G, T, C, C, A]
    rc = ro.revcomp(frag).tolist()
    # both mates read through a fragment of 10 into different adapters: the fragment comes out
    assert mu.merge_pair(frag + [G, G, A], rc + [T, C, T], 10)[0].tolist() == frag
    # the mates meet in the middle of a fragment of 14
    long = frag + [G, A, T, T]
    m, h, fb = mu.merge_pair(long[:10], ro.revcomp(long[4:]).tolist(), 14)
    assert m.tolist() == long and (h, fb) == (0, 0)
    # one mismatch column, at position 6: b' has C ^ 1 there.  Without qualities and on a tie mate 1 decides; a better mate 2 wins
    bad = list(rc)
    bad[3] ^= 1                                                          # b[3] is b'[6]
    q = lambda v, at, n=10: [v if i == at else 30 + 33 for i in range(n)]
    assert mu.merge_pair(frag, bad, 10)[1:] == (1, 0) and mu.merge_pair(frag, bad, 10)[0].tolist() == frag
    assert mu.merge_pair(frag, bad, 10, q(40 + 33, 6), q(40 + 33, 3))[1:] == (1, 0)
    m, h, fb = mu.merge_pair(frag, bad, 10, q(10 + 33, 6), q(40 + 33, 3))
    assert (h, fb) == (1, 1) and m.tolist() == frag[:6] + [bad[3] ^ 2] + frag[7:] and m[6] != frag[6]
    # a byte below the offset is quality 0, a byte past offset + 93 is 93
    assert (mu.quality_of(20, 33), mu.quality_of(33, 33), mu.quality_of(126, 33), mu.quality_of(255, 33), mu.quality_of(63, 64)) == (0, 0, 93, 93, 0)
    assert mu.merge_pair(frag, bad, 10, q(20, 6), q(34, 3))[2] == 1 and mu.merge_pair(frag, bad, 10, q(200, 6), q(255, 3))[2] == 0
    # the decision
    assert mu.merge_decide(150, 150, 200, 200, 0, 0) == 200 and mu.merge_decide(150, 150, 299, 299, 0, 0) == 299
    assert mu.merge_decide(150, 150, 300, 300, 0, 0) == mu.INCONSISTENT == mu.merge_decide(150, 150, 200, 199, 0, 0)
    assert mu.merge_decide(150, 150, 0, 0, 0, 0) == 0 == mu.merge_decide(150, 150, 200, 200, 201, 0) == mu.merge_decide(150, 150, 200, 200, 0, 199)
    # compact_quals_trimmed by slicing
    quals = np.arange(40, 60, dtype=np.uint8)
    recs = np.zeros(3, dtype=mu.MERGE_DTYPE)
    recs["start"], recs["len"] = [2, 0, 1], [3, 0, 4]
    got, n = mu.compact_bytes(quals, np.array([0, 7, 12, 20], dtype=np.uint64), recs)
    assert n == 7 and got.tolist() == [42, 43, 44, 53, 54, 55, 56, 0]


def test_the_case_holds_what_it_says():
    c = mu.case()
    assert mu.case_holds() >= 25
    assert max(len(r) for r in c["reads"]) == 2100 and min(len(r) for r in c["reads"]) == 0
    plain = mu.case_expect(None)
    n = len(c["reads"])
    rest = mu.rest_reads(c["codes"], c["offs"], plain[0])
    assert sum(len(m) for m in plain[1]) + sum(len(r) for r in rest) < int(c["offs"][-1])       # the overlaps are counted once now
    # the texts of the command line tool on the case
    rec, merged, pairs, single, hist, summary = mu.cli_texts(c["codes"], c["offs"], c["ov"], plain[0], plain[1], [(0, n)])
    assert rec.count("\n") == n and merged.count(">") == len(plain[1]) and pairs.count(">") + single.count(">") == int((plain[0]["len"] > 0).sum())
    assert summary.startswith(f"merge: reads {n} pairs {n // 2} overlapping {sum(1 for F in c['inserts'] if F)} merged {len(plain[1])} mismatch columns ")
    assert hist.splitlines()[-1].startswith(f"# pairs {n // 2} overlapping ")
    assert mu.cli_texts(c["codes"], c["offs"], c["ov"], mu.expect_merge(c["codes"], c["offs"], c["ov"], c["params"], pair_ranges=[],
                                                                         ordinals=range(n))[0], [], [])[5].endswith(f"merged 0 mismatch columns 0 bases in {int(c['offs'][-1])} bases out {int(c['ov']['len'].sum())}")


# ---- the pure checks of csrc/sdt_read_plan.h --------------------------------------------------------------------------------------------
def test_parameter_checks_and_the_decision_clean_under_sanitizers(tmp_path):
    """tools/merge_plan_check.cpp: every refusal, the decision against the rule's four lines, every position of more than 825 mergeable
    combinations covered; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "merge_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "merge_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("merge_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers merge` ----------------------------------------------------------------------------------------
def test_record_line_and_statistics_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "merge_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "merge_host_check.c"), os.path.join(host, "mergesplit.c")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "merge_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_merge(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("merge",), ("merge", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers merge -s lib.cfg -K k", "--min-overlap N, default 30", "--max-err PCT, default 10", "--min-len L, default 0",
                     "--min-merged L, default 0", "--max-merged L, default 0", "prefix.readMerge", "prefix.merge.fa", "prefix.merge.pairs.fa",
                     "prefix.merge.single.fa", "prefix.insertHist", "merged mismatches from_b start len verdict",
                     "merge: reads R pairs P overlapping V merged M mismatch columns C bases in I bases out O"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the options are refused first)
    out = str(tmp_path / "out")
    # --min-merged and --max-merged belong to merge alone
    for sub in ("profile", "correct", "normalize", "trim", "dedup", "clip", "overlap", "complexity", "qtrim", "screen", "query"):
        for opt in ("--min-merged", "--max-merged"):
            r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", opt, "100", "-o", out], capture_output=True, text=True)
            assert r.returncode == 255 and f"sdt-kmers: {opt} belongs to merge\n" in r.stderr, f"{sub} {opt}: {r.returncode} {r.stderr[:200]}"
    # merge takes the options of overlap and its own, and no other stage's
    for opt in (("--min-overlap", "20"), ("--max-err", "5"), ("--min-len", "40"), ("--min-merged", "50"), ("--max-merged", "400")):
        r = subprocess.run([exe, "merge", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and "belongs to" not in r.stderr and "whole number" not in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opt, say in ((("-a", "x.fa"), "-a belongs to clip"), (("--mate-swap",), "--mate-swap belongs to dedup"), (("--target", "5"), "--target belongs to normalize"),
                     (("--min-cov", "5"), "--min-cov belongs to trim"), (("--phred", "64"), "--phred belongs to qtrim"), (("--max-score", "5"), "--max-score belongs to complexity"),
                     (("-r", "x.fa"), "-r belongs to screen")):
        r = subprocess.run([exe, "merge", "-s", cfg, "-K", "31", *opt, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and say in r.stderr, f"{opt}: {r.returncode} {r.stderr[:200]}"
    for opt, bad, say in (("--min-merged", "-1", "whole number"), ("--max-merged", "1e3", "whole number"), ("--max-merged", "4294967296", "whole number"),
                          ("--max-err", "101", "whole number"), ("--min-overlap", "0", "at least 1")):
        r = subprocess.run([exe, "merge", "-s", cfg, "-K", "31", opt, bad, "-o", out], capture_output=True, text=True)
        assert r.returncode == 255 and opt in r.stderr and say in r.stderr, f"{opt} {bad}: {r.returncode} {r.stderr[:200]}"
    r = subprocess.run([exe, "merge", "-s", cfg, "-K", "31", "--min-merged", "100", "--max-merged", "99", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255 and "--max-merged 99 is below --min-merged 100" in r.stderr
    # the options are fine, the library config is not there: refused before the device is touched
    r = subprocess.run([exe, "merge", "-s", cfg, "-K", "31", "--min-merged", "100", "--max-merged", "100", "-o", out], capture_output=True, text=True)
    assert r.returncode == 255
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
