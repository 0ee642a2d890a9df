"""CPU: the duplicate filter exists at every layer (header, library, binding); the Python restatement of the rule (read_dedup_util.py)
-- what the GPU tests expect -- against a pairwise comparison of every unit with every other; the case of tests/test_read_dedup.py
holds what it promises; the pure functions the stage adds to csrc/sdt_read_plan.h and the device-free half of `sdt-kmers dedup`
(csrc/host/dupsplit.c) as stand-alone programs under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np

import read_dedup_util as rd
from read_select_util import dense_units, ranged_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdt_gpu_dedup_reads", "sdt_gpu_dedup_reads_device", "sdt_gpu_dedup_kept_reads"]
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    assert re.search(r"#define\s+SDT_DEDUP_MATE_SWAP\s+1u?\b", src)
    assert "Reverse complements of single reads are NOT" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sdt_[a-z_0-9]+)\s*\(", src))
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/sdt_gpu.h"
        assert hasattr(lib, s), f"{s} is not exported by libsdt_gpu.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+first;\s*uint32_t\s+copies,\s*verdict;\s*\}\s*sdt_read_dup;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+flags,\s*reserved;\s*\}\s*sdt_dedup_params;", src)
    assert "#define SDT_ABI_VERSION 8" in src


def test_read_dup_dtype_and_params_are_the_c_structs(pkg):
    import ctypes
    dt = pkg.READ_DUP_DTYPE
    assert dt.itemsize == 16 and dt.names == ("first", "copies", "verdict") == rd.DUP_FIELDS and dt == rd.DUP_DTYPE
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 12]
    assert ctypes.sizeof(pkg.DedupParams) == 8
    assert [(f, getattr(pkg.DedupParams, f).offset) for f, _ in pkg.DedupParams._fields_] == [("flags", 0), ("reserved", 4)]
    assert (pkg.DUP_KEPT, pkg.DUP_DROPPED, pkg.SDT_DEDUP_MATE_SWAP) == (rd.KEPT, rd.DROPPED, rd.MATE_SWAP)
    for m in ("dedup_reads", "dedup_reads_device", "dedup_kept_reads"):
        assert callable(getattr(pkg.PregraphGPU, m))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def random_units(seed, n_units=200):
    """single reads and pairs over a small alphabet of short reads, so that copies, swapped copies, prefixes and empty reads abound;
    some pairs have one mate only"""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(0, 2, size=int(rng.integers(0, 4)), dtype=np.uint8) for _ in range(12)]
    reads, units, o = {}, [], 0
    for _ in range(n_units):
        kind = int(rng.integers(0, 4))
        if kind < 2:
            reads[o] = pool[int(rng.integers(0, len(pool)))]
            units.append((o, [o]))
            o += 1
        else:
            members = [o, o + 1] if kind == 2 or rng.integers(0, 2) else [o + int(rng.integers(0, 2))]
            for i in members:
                reads[i] = pool[int(rng.integers(0, len(pool)))]
            units.append((o, members))
            o += 2
    return reads, units


def test_restatement_equals_pairwise_comparison():
    seen = set()
    for seed in (1, 2, 3):
        for swap in (False, True):
            reads, units = random_units(seed)
            assert len(units) == 200
            want = rd.brute_force(reads, units, swap)
            classes = rd.classes_of(reads, units, swap)
            got = {u: (ids[0], len(ids), rd.KEPT if u == ids[0] else rd.DROPPED) for ids in classes.values() for u in ids}
            assert got == want
            assert sum(len(ids) for ids in classes.values()) == 200 and len(classes) < 150
            seen |= {kind for kind, _ in classes}
            if swap:
                assert len(classes) < len(rd.classes_of(reads, units, False)), "no pair is a copy only under the flag"
    assert seen == {1, 2}
    # through expect_dedup: records by ordinal, a pair with one mate is a single read and keeps the first mate's ordinal as its id
    codes, offs = rd.concat([[0, 1], [2], [0, 1], [2], [2], [0, 1]])
    dup, keep, kept = rd.expect_dedup(codes, offs, ordinals=[0, 1, 2, 3, 5, 7], units=ranged_units([0, 1, 2, 3, 5, 7], [(0, 8)]))
    assert dup.tolist() == [(0, 2, 0), (0, 2, 0), (0, 2, 1), (0, 2, 1), (0, 0, 0), (4, 1, 0), (0, 0, 0), (6, 1, 0)]
    assert keep.tolist() == [1, 1, 0, 0, 0, 1, 0, 1] and kept == 4
    # (a, b), (b, a), a alone, b alone, (a, a): a single read never equals a pair, the swap is per pair
    a, b = [0, 1, 2], [3]
    codes, offs = rd.concat([a, b, b, a, a, a])
    assert [r[2] for r in rd.expect_dedup(codes, offs, paired=True)[0].tolist()] == [0] * 6
    assert [r[2] for r in rd.expect_dedup(codes, offs, paired=True, flags=rd.MATE_SWAP)[0].tolist()] == [0, 0, 1, 1, 0, 0]
    assert [r[2] for r in rd.expect_dedup(codes, offs)[0].tolist()] == [0, 0, 1, 1, 1, 1]
    assert rd.levels_of(rd.expect_dedup(codes, offs, paired=True, flags=1)[0], dense_units(6, True)) == [(1, 1, 2), (2, 1, 4)]


def test_the_case_holds_what_it_says():
    c = rd.case()
    n = len(c["offs"]) - 1
    assert n % 2 == 0 and 100 < n < 300 and c["nseqs"] == 34
    lens = np.diff(c["offs"].astype(np.int64))
    assert set(rd.LENGTHS) <= set(lens.tolist()) and (lens == 0).sum() == 2
    dup, keep, kept = rd.expect_dedup(c["codes"], c["offs"])
    sizes = {int(x) for x in dup["copies"]}
    assert {1, 2, 3, 7} <= sizes
    assert len(set(dup["first"].tolist())) <= 64, "the round cap of 64 could bind under SDT_DEDUP_FP_BITS=1"
    # no near-miss twin is dropped for the sequence it was made from (the proper prefix is in twice: once to make the count even)
    twins = [i for i, o in enumerate(c["origin"]) if o[0] == "twin"]
    assert {o[2] for o in c["origin"] if o[0] == "twin"} == {"last", "first", "plus", "minus", "base 32"} and len(twins) >= 13
    seq_reads = {i for i, o in enumerate(c["origin"]) if o[0] == "seq"}
    for i in twins:
        assert int(dup["first"][i]) not in seq_reads and int(dup["copies"][i]) <= 2
    # copies of one sequence start at different bases of a word, and behind two copies of one sequence come different bases
    starts = {}
    for i, o in enumerate(c["origin"]):
        if o[0] == "seq":
            starts.setdefault(o[1], []).append(int(c["offs"][i]))
    assert sum(len({s & 15 for s in v}) > 1 for v in starts.values()) >= 15
    assert len({s & 15 for v in starts.values() for s in v}) == 16
    bleed = 0
    for i in range(n - 1):
        j = int(dup["first"][i])
        if j != i and j + 1 < n and int(c["offs"][i + 1]) & 15 and lens[i + 1] and lens[j + 1]:
            bleed += int(c["codes"][int(c["offs"][i + 1])]) != int(c["codes"][int(c["offs"][j + 1])])
    assert bleed >= 10
    # the pairs: a pair that is a copy only under the flag, classes of 1, 2, 3 and 7 (9 under the flag), at most 64 classes
    p = rd.paired_case()
    plain = rd.expect_dedup(p["codes"], p["offs"], paired=True)[0]
    swap = rd.expect_dedup(p["codes"], p["offs"], paired=True, flags=rd.MATE_SWAP)[0]
    assert ((plain["verdict"] == rd.KEPT) & (swap["verdict"] == rd.DROPPED)).sum() >= 2
    assert {1, 2, 3, 7} <= set(plain["copies"].tolist()) and {4, 9} <= set(swap["copies"].tolist())
    assert len(set(plain["first"].tolist())) <= 64
    assert (plain["first"][0::2] == plain["first"][1::2]).all() and (plain["verdict"][0::2] == plain["verdict"][1::2]).all()


# ---- the pure functions of csrc/sdt_read_plan.h -----------------------------------------------------------------------------------------
def test_table_size_and_unit_stretches_clean_under_sanitizers(tmp_path):
    """tools/dedup_plan_check.cpp: the table is a power of two of at least 2 x units, the check of the pair ranges, the stretches of
    units from the pair ranges against a walk over the ordinals; includes sdt_read_plan.h alone"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(ROOT, "tools", "dedup_plan_check.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["../soapdenovo-trans_amd/csrc/sdt_read_plan.h"]
    exe = str(tmp_path / "dedup_plan_check")
    subprocess.run([cxx, "-std=c++17"] + SAN + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("dedup_plan_check: ok"), r.stdout + r.stderr


# ---- the device-free half of `sdt-kmers dedup` ----------------------------------------------------------------------------------------
def test_record_line_and_levels_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "dedup_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "dedup_host_check.c"), os.path.join(host, "dupsplit.c")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dedup_host_check: ok" in r.stdout, r.stdout + r.stderr


def test_sdt_kmers_usage_knows_dedup(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    for args in ((), ("dedup",), ("dedup", "-s", "lib.cfg")):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 255
        for word in ("sdt-kmers dedup -s lib.cfg -K k", "--mate-swap", "prefix.readDup", "prefix.dedup.pairs.fa", "prefix.dedup.single.fa",
                     "prefix.dupLevels", "first copies verdict", "copies classes reads"):
            assert word in r.stderr, f"sdt-kmers {' '.join(args)}: the usage text lacks {word!r}"
    cfg = str(tmp_path / "none.cfg")                    # (never opened: the option is refused first)
    for sub in ("profile", "correct", "normalize", "trim", "query"):
        r = subprocess.run([exe, sub, "-s", cfg, "-K", "31", "--mate-swap", "-o", str(tmp_path / "out")], capture_output=True, text=True)
        assert r.returncode == 255 and "--mate-swap belongs to dedup" in r.stderr
    r = subprocess.run([exe, "dedup", "-s", cfg, "-K", "31", "--target", "5", "-o", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 255 and "--target belongs to normalize" in r.stderr
