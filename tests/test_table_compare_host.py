"""CPU: the comparison of two counted tables (sdt_gpu_compare_tables, sdt_gpu_compare_select) -- the surface, the restatement of the rule
(table_compare_util.py) against a second one written over strings and against an example worked by hand, its symmetries, the even-K
palindrome on the model, and the device-free half of `sdt-kmers compare` (cmpsplit.c) through tools/cmp_host_check built under
AddressSanitizer + UBSan."""
import collections
import os
import re
import shutil
import subprocess

import numpy as np

import asm_support_util as au
import table_compare_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_compare_tables", "sdt_gpu_compare_select"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_two_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    for words in ("#define SDT_CMP_MAX_CELLS 16384", "typedef struct { uint32_t rows, cols, flags, reserved; } sdt_cmp_params;",
                  "typedef struct { uint32_t min_a, max_a, min_b, max_b; } sdt_cmp_range;", "min(cA, rows - 1) = r", "compare(B, A) is the transpose",
                  "the sum of min(cA, cB) over the shared nodes", "capacity = 0 with NULL", "after B's stream has been drained"):
        assert words in src, words
    assert "#define SDT_ABI_VERSION 8" in re.sub(r"[ \t]+", " ", src)
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(sdt_ctx \*a, sdt_ctx \*b," % s, src), s
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS
    assert pkg.CMP_MAX_CELLS == tu.MAX_CELLS == 16384
    for name in ("compare_tables", "compare_select", "compare_select_count", "CmpParams", "CmpRange"):
        assert hasattr(pkg, name), name
    assert callable(pkg.PregraphGPU.compare) and callable(pkg.PregraphGPU.compare_select)
    assert [f for f, _ in pkg.CmpParams._fields_] == ["rows", "cols", "flags", "reserved"] and (pkg.CmpParams().rows, pkg.CmpParams().cols) == (64, 64)
    r = pkg.CmpRange()
    assert (r.min_a, r.max_a, r.min_b, r.max_b) == (1, 2**32 - 1, 0, 0)


# ---- the restatement against a second one over strings ----------------------------------------------------------------------------------
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
RANK = {c: i for i, c in enumerate(au.LETTERS)}


def string_table(codes, offs, K):
    """canonical k-mer (as letters) -> occurrences, from the reads as text: the smaller strand under A < C < T < G"""
    t = collections.Counter()
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        s = au.text_of(codes[int(a):int(b)])
        for i in range(len(s) - K + 1):
            fw = s[i:i + K]
            rc = "".join(COMP[c] for c in reversed(fw))
            t[min(fw, rc, key=lambda x: [RANK[c] for c in x])] += 1
    return t


def test_the_restatement_against_one_over_strings(synth):
    K = 23
    case = tu.pair_case(synth, K)
    SA, SB = string_table(*case["a"], K), string_table(*case["b"], K)
    assert {tu.kmer_text(k, K): c for k, c in case["A"].items()} == dict(SA)          # (the oracle's table is the reads' k-mers, by occurrence)
    assert {tu.kmer_text(k, K): c for k, c in case["B"].items()} == dict(SB)
    for rows, cols in ((64, 64), (2, 8192), (5, 3)):
        m, t = tu.compare(case["A"], case["B"], rows, cols)
        cells = collections.Counter((min(SA[s], rows - 1), min(SB[s], cols - 1)) for s in set(SA) | set(SB))
        assert {(r, c): int(m[r, c]) for r in range(rows) for c in range(cols) if m[r, c]} == dict(cells)
        both = set(SA) & set(SB)
        assert t.tolist() == [len(SA), len(SB), len(both), sum(SA.values()), sum(SB.values()), sum(min(SA[s], SB[s]) for s in both),
                              sum(SA[s] for s in both), sum(SB[s] for s in both)]
    for rg in ((2, tu.U32, 0, 0), (1, tu.U32, 1, tu.U32), (0, tu.U32, 0, tu.U32), (3, 3, 70000, 70001)):
        want = {(s, SA[s], SB.get(s, 0)) for s in SA if rg[0] <= SA[s] <= rg[1] and rg[2] <= SB.get(s, 0) <= rg[3]}
        assert {(tu.kmer_text(k, K), a, b) for k, a, b in tu.select(case["A"], case["B"], *rg)} == want
    assert tu.select(case["A"], case["B"], 3, 3, 70000, 70001) == set() and len(tu.select(case["A"], case["B"], 2, tu.U32, 0, 0)) > 100


# ---- by hand ------------------------------------------------------------------------------------------------------------------------------
HAND_A = {1: 1, 2: 2, 3: 5, 4: 1, 5: 0}                  # k-mers as small integers; 5 is a node counted 0 times
HAND_B = {1: 1, 2: 0, 3: 7, 6: 2, 7: 1}                  # 2 is a node of B counted 0 times: shared, and in column 0
HAND_MATRIX = [[1, 1, 1], [1, 1, 0], [1, 0, 1]]
HAND_TOTALS = [5, 5, 3, 9, 11, 6, 8, 8]


def test_worked_example():
    """union: 1 -> (1, 1); 2 -> (2, 0); 3 -> (5, 7), capped to (2, 2); 4 -> (1, absent); 5 -> (0, absent); 6 -> (absent, 2); 7 -> (absent, 1)"""
    m, t = tu.compare(HAND_A, HAND_B, 3, 3)
    assert m.tolist() == HAND_MATRIX and t.tolist() == HAND_TOTALS
    assert tu.select(HAND_A, HAND_B) == {(2, 2, 0), (4, 1, 0)}                        # cA >= 1 and cB = 0: a count of 0 in B is as good as absent
    assert tu.select(HAND_A, HAND_B, 0, 0, 0, 0) == {(5, 0, 0)}
    assert tu.select(HAND_B, HAND_A) == {(6, 2, 0), (7, 1, 0)}                        # the k-mers only in B: the tables swapped
    assert tu.select(HAND_A, HAND_B, 1, tu.U32, 1, tu.U32) == {(1, 1, 1), (3, 5, 7)}
    assert tu.summary_fields(t, m, 2) == (5, 5, 3, 2, 2, 1, 4285, 6000, 6000, 4000)
    assert tu.summary_fields(np.zeros(8, dtype=np.uint64), np.zeros((3, 3), dtype=np.uint64), 2) == (0,) * 10
    assert tu.matrix_text(m) == "a\\b 0 1 2+\n0 1 1 1\n1 1 1 0\n2+ 1 0 1\n"


def test_symmetries_on_the_model(synth):
    case = tu.pair_case(synth, 31)
    A, B = case["A"], case["B"]
    for rows, cols in ((64, 64), (3, 9)):
        m, t = tu.compare(A, B, rows, cols)
        mt, tt = tu.compare(B, A, cols, rows)
        assert (mt == m.T).all() and (tt == tu.swapped(t)).all()
        assert int(m.sum()) == int(t[0] + t[1] - t[2]) and int(m[1:, 1:].sum()) <= int(t[2])
    d, t = tu.compare(A, A, 64, 64)
    assert (d == np.diag(np.diag(d))).all() and t[0] == t[1] == t[2] == len(A) and t[3] == t[4] == t[5] == t[6] == t[7]
    assert {k for k, _, _ in tu.select(A, B, 0, tu.U32, 0, tu.U32)} == set(A)


def test_even_k_palindrome_on_the_model():
    """K = 4: ACGT is its own reverse complement (A-T, C-G) and counts once per occurrence; the library takes odd K only, so this is held
    on the restatement alone"""
    K = 4
    pal = au.codes_of("ACGT")
    assert (au.revcomp(pal) == pal).all()
    A = collections.Counter(au.canon_kmers(au.codes_of("ACGTACGT"), K))            # ACGT twice, CGTA twice (TACG is its other strand), GTAC: a palindrome too
    B = collections.Counter(au.canon_kmers(au.codes_of("AACGTT"), K))              # AACG twice (CGTT is its other strand), ACGT once
    k = au.canon_kmers(pal, K)[0]
    assert A[k] == 2 and B[k] == 1
    m, t = tu.compare(A, B, 3, 3)
    assert m[2, 1] == 1 and t[2] == 1 and t[5] == 1 and (t[6], t[7]) == (2, 1)
    assert (k, 2, 1) in tu.select(A, B, 2, 2, 1, 1)


# ---- the device-free half of `sdt-kmers compare` ---------------------------------------------------------------------------------------
def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "cmp_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "cmp_host_check.c"), os.path.join(host, "cmpsplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "cmp_host_check: ok" in r.stdout, r.stdout + r.stderr
    # the texts it wrote for the example by hand are the restatement's
    m, t = np.array(HAND_MATRIX, dtype=np.uint64), np.array(HAND_TOTALS, dtype=np.uint64)
    assert (tmp_path / "hand.cmpMatrix").read_text() == tu.matrix_text(m)
    assert (tmp_path / "hand.summary").read_text() == tu.summary_text(t, m, 2)
    sel = {(0x2A, 1, 0), (0x07, 2, 0), (0x34, 70000, 4000000000), (0x01, 4, 9)}
    assert (tmp_path / "hand.cmpKmers").read_text() == tu.kmers_text(sel, 3)[0] == "AAC 4 9\nACG 2 0\nTTT 1 0\nGCA 70000 4000000000\n"
    assert tu.kmers_text(sel, 3, max_list=3) == (None, "# 4 matched\n")


def test_sdt_kmers_usage_knows_compare(pkg):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "compare"], capture_output=True, text=True)
    assert r.returncode == 255
    for word in ("sdt-kmers compare -s a.cfg --against b.cfg -K k", "[--rows R, default 64]", "[--cols C, default 64]", "[--select MINA:MAXA:MINB:MAXB]",
                 "[--max-list N, default 1000000]", "prefix.cmpMatrix", "prefix.cmpKmers", "# M matched",
                 "compare: nodes_a X nodes_b Y shared S solid_a P", "J = floor(10000 S / (X + Y - S))", "0 when the"):
        assert word in r.stderr, f"the usage text lacks {word!r}"
