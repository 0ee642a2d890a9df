"""CPU: the surface of the bubble list (header, exported symbols, binding), the Python restatement of its rule (bubble_util.py) on the
cases of the GPU tests, its symmetries, the palindromic source, the device-free half of `sdt-kmers bubbles` (bubblesplit.c) through
tools/bubble_host_check built under AddressSanitizer + UBSan as a program of its own, and the option table of the built tool."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CALLS = ("begin", "fetch", "paths", "end")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.load_library()
    for c in CALLS:
        assert re.search(r"\bint sdt_gpu_bubbles_%s\(sdt_ctx \*ctx" % c, code), c
        assert hasattr(lib, f"sdt_gpu_bubbles_{c}") and f"sdt_gpu_bubbles_{c}" in pkg.ABI_SYMBOLS
        assert hasattr(pkg.PregraphGPU, f"bubbles_{c}")
    assert hasattr(pkg.PregraphGPU, "import_nodes")
    assert "typedef struct { uint32_t min_count, max_count, min_link, max_len, flags, reserved; } sdt_bubble_params;" in code
    assert "typedef struct { uint64_t sum_a, sum_b; uint32_t len_a, len_b, min_a, min_b, src_count, snk_count, info, reserved; } sdt_bubble;" in code
    assert "#define SDT_BUBBLE_MAX_LEN (1u << 20)" in code
    assert "#define SDT_ABI_VERSION 8" in re.sub(r"[ \t]+", " ", code) and lib.sdt_gpu_abi_version() == 8
    for word in ("ORIENTED WORDS", "SUCCESSORS", "BRANCH", "REPORTED iff s <= revcomp(t)", "the table changed since sdt_gpu_bubbles_begin",
                 "Nothing is per table slot"):
        assert word in src, word
    p = pkg.BubbleParams()
    assert (p.min_count, p.max_count, p.min_link, p.max_len, p.flags, p.reserved) == (2, 0, 1, 1000, 0, 0) and ctypes.sizeof(p) == 24
    assert pkg.BUBBLE_DTYPE == bu.DTYPE and pkg.BUBBLE_DTYPE.itemsize == 48 and pkg.BUBBLE_DTYPE.names == bu.FIELDS
    assert pkg.BUBBLE_MAX_LEN == 1 << 20


# ---- the restatement on its cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [23, 24, 31, 47, 63, 95, 33, 65, 97])
def test_the_cases_hold_what_they_are_built_for(K):
    """the builder asserts every property on the model (bubble_util.built_case): a case that lost one fails here.  Also: the list is the
    same after every read was reverse-complemented; every reported bubble has s <= revcomp(t), and its mirror is found and dropped"""
    case = bu.built_case(K)
    model = case["model"]
    assert case["L"] == max(100, 2 * K + 10) and len(model.bubbles) == 8 and len(case["model1"].bubbles) == 9
    flipped = bu.bubbles_of_reads(*bu.reverse_complemented(case), K)
    assert flipped.bubbles == model.bubbles and flipped.info == model.info and flipped.records().tolist() == model.records().tolist()
    found = {(f[0], f[1], f[2], f[3]): f for f in model.found}
    for s, ba, bb, t, a, b in model.bubbles:
        assert s <= cu.rc_int(t, K)
        mirror = [f for f in model.found if f[0] == cu.rc_int(t, K) and f[3] == cu.rc_int(s, K)]
        assert mirror and all(f not in model.bubbles for f in mirror)
        # the same two paths, read the other way: lengths, minima and sums agree as sets of sides
        assert sorted((m[4][1:4], m[5][1:4]) for m in mirror)[0] in ((a[1:4], b[1:4]), (b[1:4], a[1:4])) or len(mirror) > 1
    assert len(found) == len(model.found)
    # paths: the allele is s followed by the bases, and ends in t
    for i, (s, _, _, t, a, b) in enumerate(model.bubbles):
        for seq, br in zip(model.alleles(i), (a, b)):
            assert len(seq) == K + br[1] + 1 and seq[:K] == cu.kmer_text(s, K) and seq[-K:] == cu.kmer_text(t, K)


def test_the_palindromic_source_on_the_model():
    """K = 24: the source is its own reverse complement -- one oriented word, whose right counters hold what leaves it on either strand"""
    K = 24
    nodes, s = bu.palindrome_graph(K)
    assert cu.rc_int(s, K) == s
    model = bu.Bubbles(bu.as_model_nodes(nodes), K, **bu.DEFAULTS)
    assert len(model.succ(s, s)) == 3 and model.info[1] == 2 and model.info[2] == 5
    assert len(model.bubbles) == 1 and len(model.found) == 2 and s in {f[0] for f in model.found} and s in {cu.rc_int(f[3], K) for f in model.found}


# ---- the device-free half of `sdt-kmers bubbles` -----------------------------------------------------------------------------------------------
def hand_model():
    m = bu.Bubbles.__new__(bu.Bubbles)
    m.K = 3
    m.bubbles = [(0x07, 0, 2, 0x38, (7, 3, 7, 21, [3, 2, 0]), (2, 3, 2, 9, [3, 2, 0])),
                 (0x12, 1, 3, 0x09, (6, 0, 0, 0, []), (5, 2, 5, 11, [1, 2])),
                 (0x2A, 0, 1, 0x15, (63, 2, 4000000000, 5000000000, [0, 3]), (1, 2, 4, 8, [1, 1]))]
    m.info = [40, 6, 13, 12, 3, 18, 3, 0]
    return m


def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "bubble_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "bubble_host_check.c"), os.path.join(host, "bubblesplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "bubble_host_check: ok" in r.stdout, r.stdout + r.stderr
    # the texts it wrote for the example by hand are the restatement's
    m = hand_model()
    assert (tmp_path / "hand.bubbles").read_text() == bu.bubbles_text(m) == \
        "1 ACG GTA A T 3 3 7 2 21 9 7 2 0\n2 CAT ATC C G 0 2 0 5 0 11 6 5 2\n3 TTT CCC A C 2 2 4000000000 4 5000000000 8 63 1 1\n"
    assert (tmp_path / "hand.bubbles.fa").read_text() == bu.fasta_text(m) == \
        (">1_a len=3 min=7 sum=21\nACGAGTA\n>1_b len=3 min=2 sum=9\nACGTGTA\n>2_a len=0 min=0 sum=0\nCATC\n>2_b len=2 min=5 sum=11\nCATGCT\n"
         ">3_a len=2 min=4000000000 sum=5000000000\nTTTAAG\n>3_b len=2 min=4 sum=8\nTTTCCC\n")
    assert (tmp_path / "hand.summary").read_text() == bu.summary_line(m) + "\n"


# ---- the option table of the built tool ------------------------------------------------------------------------------------------------------------
def test_sdt_kmers_options(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "bubbles"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers bubbles -s lib.cfg" in r.stderr and "--max-branch L" in r.stderr
    out = str(tmp_path / "none")
    for sub in ("profile", "cluster", "evaluate"):
        r = subprocess.run([exe, sub, "-s", "none.cfg", "-o", out, "--max-branch", "5"], capture_output=True, text=True)
        assert r.returncode == 255 and "sdt-kmers: --max-branch belongs to bubbles\n" in r.stderr
    for opt, val in (("--max-count", "5"), ("--min-link", "2")):
        r = subprocess.run([exe, "profile", "-s", "none.cfg", "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode == 255 and f"sdt-kmers: {opt} belongs to cluster\n" in r.stderr
        # bubbles takes them: what stops the run is the config that is not there
        r = subprocess.run([exe, "bubbles", "-s", str(tmp_path / "none.cfg"), "-o", out, opt, val, "--max-branch", "50"], capture_output=True, text=True)
        assert r.returncode != 0 and "belongs to" not in r.stderr and "usage:" not in r.stderr, r.stderr[:300]
    for args in (["--min-link", "0"], ["--min-link", "64"], ["--max-branch", "0"], ["--max-branch", str((1 << 20) + 1)], ["-c", "5", "--max-count", "4"],
                 ["--pick", "1:2"]):
        r = subprocess.run([exe, "bubbles", "-s", "none.cfg", "-o", out] + args, capture_output=True, text=True)
        assert r.returncode == 255 and args[-2] in r.stderr, (args, r.stderr[:200])
    assert os.listdir(tmp_path) == []                     # nothing is written
