"""CPU: the surface of the unitig list (header, exported symbols, binding), the Python restatement of its rule (unitig_util.py) on the
cases of the GPU tests and on hand graphs with a palindromic word, the device-free half of `sdt-kmers unitigs` (unitigsplit.c) through
tools/unitig_host_check built under AddressSanitizer + UBSan as a program of its own, and the option table of the built tool."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_util as uu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CALLS = ("begin", "fetch", "seqs", "links", "end")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.load_library()
    for c in CALLS:
        assert re.search(r"\bint sdt_gpu_unitigs_%s\(sdt_ctx \*ctx" % c, code), c
        assert hasattr(lib, f"sdt_gpu_unitigs_{c}") and f"sdt_gpu_unitigs_{c}" in pkg.ABI_SYMBOLS
        assert hasattr(pkg.PregraphGPU, f"unitigs_{c}")
    assert "typedef struct { uint32_t min_count, max_count, min_link, flags; } sdt_unitig_params;" in code
    assert "typedef struct { uint64_t sum; uint32_t nodes, min, max, info; } sdt_unitig;" in code
    assert "typedef struct { uint32_t from, to, info, reserved; } sdt_unitig_link;" in code
    assert "#define SDT_ABI_VERSION 8" in re.sub(r"[ \t]+", " ", code) and lib.sdt_gpu_abi_version() == 8
    for word in ("JOIN.", "UNITIG.", "SEQUENCE.", "LINKS.", "x0 <= revcomp(x(n-1))", "the table changed since sdt_gpu_unitigs_begin", "ONE BIT PER TABLE SLOT",
                 "quadratic in the length of", "list-ranking"):
        assert word in src, word
    p = pkg.UnitigParams()
    assert (p.min_count, p.max_count, p.min_link, p.flags) == (2, 0, 1, 0) and ctypes.sizeof(p) == 16
    assert pkg.UNITIG_DTYPE == uu.DTYPE and pkg.UNITIG_DTYPE.itemsize == 24 and pkg.UNITIG_DTYPE.names == uu.FIELDS
    assert pkg.UNITIG_LINK_DTYPE == uu.LINK_DTYPE and pkg.UNITIG_LINK_DTYPE.itemsize == 16


# ---- the restatement on its cases ----------------------------------------------------------------------------------------------------------
def check_model(m):
    """what holds for every list: the nodes are covered once (asserted where the model is built), the order, the orientation, the links
    from both sides, the overlaps"""
    K = m.K
    firsts = [t["words"][0] for t in m.unitigs]
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)
    for t in m.unitigs:
        if t["circular"]:
            assert t["words"][0] == min(min(w, cu.rc_int(w, K)) for w in t["words"]) and t["indeg"] == t["outdeg"] == 1
        else:
            assert t["words"][0] <= cu.rc_int(t["words"][-1], K)
    assert m.info[4] == m.info[0] and m.info[5] == sum(len(m.codes(i)) for i in range(len(m.unitigs)))
    assert uu.canonical_kmers(m) == sorted(m.g.live)
    uu.assert_overlaps(m)


@pytest.mark.parametrize("K", [23, 31, 33, 65, 97])
def test_the_cases_hold_what_they_are_built_for(K):
    """the figures of the built cases, so that a case that lost its point fails without a GPU; every link is seen from both sides; every
    inner stretch of a bubble side is exactly one unitig; the list is the same after every read was reverse-complemented"""
    case = bu.built_case(K)
    sides = {2: 15, 1: 17}
    for min_count, n in ((2, 36), (1, 41)):
        m = uu.Unitigs(case["nodes"], K, min_count=min_count)
        check_model(m)
        assert m.info[2] == n and m.info[1] == 2 * n and m.info[3] == 0 and m.dangling == 0
        assert m.info[6] == case["longest"] == {23: 3022, 31: 3030, 33: 3032, 65: 3064, 97: 3096}[K]      # the long side of the detour is one unitig
        seen = {(u, o, v, o2) for u, v, o, o2, _, _ in m.links}
        assert all((v, 1 - o2, u, 1 - o) in seen for u, o, v, o2 in seen)
        # a bubble side with inner nodes: the first of them starts a unitig (or ends its mirror) with the same nodes, min and sum
        by_first = {t["words"][0]: t for t in m.unitigs}
        by_rlast = {cu.rc_int(t["words"][-1], K): t for t in m.unitigs}
        bub = case["model"] if min_count == 2 else case["model1"]
        matched = 0
        for s, ba, bb, _, a, b in bub.bubbles:
            for base, (_, ln, mn, total, _) in ((ba, a), (bb, b)):
                if ln == 0:
                    continue
                y = ((s << 2) | base) & ((1 << (2 * K)) - 1)
                t = by_first.get(y) or by_rlast[y]
                assert (len(t["counts"]), min(t["counts"]), sum(t["counts"])) == (ln, mn, total)
                matched += 1
        assert matched == sides[min_count]
    flipped = uu.Unitigs(cu.oracle_nodes(cu.counted_oracle(*bu.reverse_complemented(case), K)), K)
    m = uu.Unitigs(case["nodes"], K)
    assert flipped.info == m.info and flipped.records().tolist() == m.records().tolist() and flipped.links == m.links
    assert flipped.seqs()[0].tobytes() == m.seqs()[0].tobytes()


def test_cycles_on_the_model():
    """a pure cycle needs c + c[:K]: with c + c[:K - 1] the closing link is missing and the cycle is a path"""
    K = 23
    m = uu.Unitigs(bu.as_model_nodes(uu.cycle_graph(K, 200, 5)), K)
    check_model(m)
    assert m.info == [200, 0, 1, 1, 200, 200 + K - 1, 200, 0]
    assert [(u, v, o, o2) for u, v, o, o2, _, _ in m.links] == [(0, 0, 0, 0), (0, 0, 1, 1)] and len(m.gfa_links()) == 1
    c = np.random.default_rng(5).integers(0, 4, size=200, dtype=np.uint8)
    path = uu.Unitigs(bu.as_model_nodes(bu.hand_graph([np.concatenate([c, c[:K - 1]])], K)), K)
    assert path.info[2:4] == [1, 0] and path.info[1] == 2 and path.links == []


def test_palindromic_words_on_the_model():
    """K = 24 (the device takes odd K only): a word that is its own reverse complement joins nothing, is one oriented word and one start,
    and is reported once"""
    K = 24
    nodes, s = bu.palindrome_graph(K)
    assert cu.rc_int(s, K) == s
    m = uu.Unitigs(bu.as_model_nodes(nodes), K)
    check_model(m)
    (i,) = [j for j, t in enumerate(m.unitigs) if s in t["words"]]
    assert m.unitigs[i]["words"] == [s] and m.unitigs[i]["indeg"] == m.unitigs[i]["outdeg"] == 3
    assert m.info[1] == 2 * m.info[2] - 1                     # every chain is found from both ends but that one
    assert sorted(l[4] for l in m.links if l[0] == i) == [b for b, _, _, _ in m.g.succ(s, s)]
    # alone: one node, no link
    rng = np.random.default_rng(3)
    half = rng.integers(0, 4, size=K // 2, dtype=np.uint8)
    lone = bu.hand_graph([np.concatenate([half, cu.revcomp(half)])], K)
    m = uu.Unitigs(bu.as_model_nodes(lone), K)
    assert m.info == [1, 1, 1, 0, 1, K, 1, 0] and m.links == []


# ---- the device-free half of `sdt-kmers unitigs` -----------------------------------------------------------------------------------------------
def hand_model():
    m = uu.Unitigs.__new__(uu.Unitigs)
    m.K = 3
    unitig = lambda words, bases, counts, circular, indeg, outdeg: dict(words=words, bases=bases, counts=counts, circular=circular, indeg=indeg, outdeg=outdeg)
    m.unitigs = [unitig([0x07], [], [9], 0, 0, 2), unitig([0x1C, 0x32], [2], [4000000000, 3000000000], 0, 1, 0), unitig([0x1E], [], [5], 0, 1, 1),
                 unitig([0x29, 0x26, 0x1A], [2, 2], [3, 4, 5], 1, 1, 1), unitig([0x3F], [], [2], 0, 0, 0)]
    m.links = [(0, 1, 0, 0, 0, 6), (0, 2, 0, 0, 2, 3), (1, 0, 1, 1, 2, 6), (2, 2, 0, 1, 0, 63), (2, 0, 1, 1, 2, 3), (3, 3, 0, 0, 2, 4), (3, 3, 1, 1, 3, 4)]
    m.info = [8, 8, 5, 1, 8, 18, 3, 0]
    return m


def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "unitig_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "unitig_host_check.c"), os.path.join(host, "unitigsplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "unitig_host_check: ok" in r.stdout, r.stdout + r.stderr
    # the texts it wrote for the example by hand are the restatement's
    m = hand_model()
    assert (tmp_path / "hand.unitigs").read_text() == uu.unitigs_text(m) == \
        ("1 ACG ACG 1 3 9 900 9 9 0 2 0\n2 CGA GAT 2 4 7000000000 350000000000 3000000000 4000000000 1 0 0\n3 CGT CGT 1 3 5 500 5 5 1 1 0\n"
         "4 TTC CTT 3 5 12 400 3 5 1 1 1\n5 GGG GGG 1 3 2 200 2 2 0 0 0\n")
    assert (tmp_path / "hand.unitigs.fa").read_text() == uu.fasta_text(m) == \
        (">1 nodes=1 sum=9 min=9 max=9 circular=0\nACG\n>2 nodes=2 sum=7000000000 min=3000000000 max=4000000000 circular=0\nCGAT\n"
         ">3 nodes=1 sum=5 min=5 max=5 circular=0\nCGT\n>4 nodes=3 sum=12 min=3 max=5 circular=1\nTTCTT\n>5 nodes=1 sum=2 min=2 max=2 circular=0\nGGG\n")
    assert (tmp_path / "hand.unitigs.gfa").read_text() == uu.gfa_text(m) == \
        ("H\tVN:Z:1.0\nS\t1\tACG\tLN:i:3\tKC:i:9\nS\t2\tCGAT\tLN:i:4\tKC:i:7000000000\nS\t3\tCGT\tLN:i:3\tKC:i:5\nS\t4\tTTCTT\tLN:i:5\tKC:i:12\n"
         "S\t5\tGGG\tLN:i:3\tKC:i:2\nL\t1\t+\t2\t+\t2M\tlc:i:6\nL\t1\t+\t3\t+\t2M\tlc:i:3\nL\t3\t+\t3\t-\t2M\tlc:i:63\nL\t4\t+\t4\t+\t2M\tlc:i:4\n")
    assert (tmp_path / "hand.summary").read_text() == uu.summary_line(m) + "\n"


# ---- the option table of the built tool ------------------------------------------------------------------------------------------------------------
def test_sdt_kmers_options(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "unitigs"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers unitigs -s lib.cfg" in r.stderr and "prefix.unitigs.gfa" in r.stderr
    out = str(tmp_path / "none")
    r = subprocess.run([exe, "unitigs", "-s", "none.cfg", "-o", out, "--max-branch", "5"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers: --max-branch belongs to bubbles\n" in r.stderr
    for opt, val in (("--max-count", "5"), ("--min-link", "2")):
        # unitigs takes them: what stops the run is the config that is not there
        r = subprocess.run([exe, "unitigs", "-s", str(tmp_path / "none.cfg"), "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode != 0 and "belongs to" not in r.stderr and "usage:" not in r.stderr, r.stderr[:300]
    for args in (["--min-link", "0"], ["--min-link", "64"], ["-c", "5", "--max-count", "4"], ["--pick", "1:2"]):
        r = subprocess.run([exe, "unitigs", "-s", "none.cfg", "-o", out] + args, capture_output=True, text=True)
        assert r.returncode == 255 and args[-2] in r.stderr, (args, r.stderr[:200])
    assert os.listdir(tmp_path) == []                     # nothing is written
