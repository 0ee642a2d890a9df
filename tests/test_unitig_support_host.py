"""CPU: the surface of the read support tally (header, exported symbols, binding, subcommand table), the Python restatement of its rule
(unitig_support_util.py) on the cases of the GPU tests -- what follows from the rule, against the threading model's own texts -- and the
device-free half of `sdt-kmers support` (supportsplit.c) through tools/support_host_check built under AddressSanitizer + UBSan as a
program of its own."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_support_util as su
import unitig_thread_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CALLS = ("begin", "add", "add_device", "unitigs", "links", "junctions", "mates", "totals", "end")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_subcommand_agree(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    lib = pkg.load_library()
    for proto in ("int sdt_gpu_unitigs_support_begin(sdt_ctx *ctx, const sdt_support_params *params);",
                  "int sdt_gpu_unitigs_support_add(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, int paired);",
                  "int sdt_gpu_unitigs_support_add_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads, int paired);",
                  "int sdt_gpu_unitigs_support_unitigs(sdt_ctx *ctx, uint64_t first, uint64_t n, sdt_unitig_support *out);",
                  "int sdt_gpu_unitigs_support_links(sdt_ctx *ctx, uint64_t first, uint64_t n, sdt_link_support *out, uint64_t capacity, uint64_t *n_links);",
                  "int sdt_gpu_unitigs_support_junctions(sdt_ctx *ctx, sdt_unitig_junction *out, uint64_t capacity, uint64_t *n);",
                  "int sdt_gpu_unitigs_support_mates(sdt_ctx *ctx, sdt_mate_link *out, uint64_t capacity, uint64_t *n);",
                  "int sdt_gpu_unitigs_support_totals(sdt_ctx *ctx, uint64_t totals[12]);",
                  "int sdt_gpu_unitigs_support_end(sdt_ctx *ctx);"):
        assert proto in code, proto
    for c in CALLS:
        assert hasattr(lib, f"sdt_gpu_unitigs_support_{c}") and f"sdt_gpu_unitigs_support_{c}" in pkg.ABI_SYMBOLS
        assert hasattr(pkg.PregraphGPU, f"unitigs_support_{c}")
    assert "typedef struct { uint64_t junction_capacity, mate_capacity; uint32_t flags, reserved; } sdt_support_params;" in code
    assert "typedef struct { uint64_t segs, kmers; } sdt_unitig_support;" in code
    assert "typedef struct { uint64_t along, against; } sdt_link_support;" in code
    assert "typedef struct { uint32_t from, via, to, reserved; uint64_t count; } sdt_unitig_junction;" in code
    assert "typedef struct { uint32_t from, to; uint64_t pairs; } sdt_mate_link;" in code
    assert "#define SDT_ABI_VERSION 8" in code and lib.sdt_gpu_abi_version() == 8
    for word in ("ORIENTED UNITIG.", "PER UNITIG", "PER LINK", "TRAVERSAL", "MIRROR", "JUNCTIONS", "PASSAGE", "MATE LINKS", "TOTALS", "WHEN A SET FILLS UP",
                 "no sdt_gpu_unitigs_support_begin", "DISTINCT READS", "16 B per unitig", "8 x 8 B per unitig", "insert-size"):
        assert word in src, word
    # what the two blocks above it listed as out of scope is not listed there any more
    assert "accumulating per-unitig support on the device" not in src and "mate links between unitigs;" not in src
    assert pkg.UNITIG_SUPPORT_DTYPE == su.UNITIG_DTYPE and pkg.UNITIG_SUPPORT_DTYPE.itemsize == 16
    assert pkg.LINK_SUPPORT_DTYPE == su.LINK_DTYPE and pkg.LINK_SUPPORT_DTYPE.itemsize == 16
    assert pkg.UNITIG_JUNCTION_DTYPE == su.JUNCTION_DTYPE and pkg.UNITIG_JUNCTION_DTYPE.itemsize == 24
    assert pkg.MATE_LINK_DTYPE == su.MATE_DTYPE and pkg.MATE_LINK_DTYPE.itemsize == 16
    assert pkg.SUPPORT_TOTALS == su.TOTALS and len(su.TOTALS) == 12
    p = pkg.SupportParams(junction_capacity=3, mate_capacity=1 << 33)
    assert bytes(p) == np.array([3, 1 << 33, 0], dtype=np.uint64).tobytes()


def test_sdt_kmers_support_options(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "support"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers support -s lib.cfg" in r.stderr
    for ext in ("unitigSupport", "linkSupport", "junctions"):
        assert f"prefix.{ext}" in r.stderr, ext
    assert "mateLinks" not in r.stderr and "--max-mate-links" not in r.stderr      # (the tool adds single reads: mate links are the library's)
    out = str(tmp_path / "none")
    for opt, val, owner in (("--pick", "1:2", "cluster"), ("--max-branch", "5", "bubbles")):
        r = subprocess.run([exe, "support", "-s", "none.cfg", "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode == 255 and f"sdt-kmers: {opt} belongs to {owner}\n" in r.stderr
    for opt, val in (("--max-count", "5"), ("--min-link", "2"), ("-c", "3"), ("--max-junctions", "100")):
        # support takes them: what stops the run is the config that is not there
        r = subprocess.run([exe, "support", "-s", str(tmp_path / "none.cfg"), "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode != 0 and "belongs to" not in r.stderr and "usage:" not in r.stderr, r.stderr[:300]
    r = subprocess.run([exe, "thread", "-s", "none.cfg", "-o", out, "--max-junctions", "5"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers: --max-junctions belongs to support\n" in r.stderr
    assert os.listdir(tmp_path) == []                     # nothing is written


# ---- the restatement on its cases ----------------------------------------------------------------------------------------------------------
def consequences(sup, rec, offs, segs, reads, paired):
    """what the rule promises on any tally, against the threading model's own records and texts"""
    n = len(sup.segs)
    assert sum(sup.segs) == len(segs) == sup.t["segments"] and sum(sup.kmers) == int(rec["live"].sum()) == sup.t["live"]
    text = tu.unitig_reads_text(n, rec, offs, segs).splitlines()
    assert [tuple(int(x) for x in line.split()[2:]) for line in text] == list(zip(sup.segs, sup.kmers))
    linked = int(tu.summary_line(rec, segs).split(" linked ")[1].split()[0])
    ls = sup.links()
    assert int(ls["along"].sum()) == linked == sup.t["traversals"] and sup.t["no_record"] == 0
    assert int(ls["against"].sum()) == linked                  # (every record is the mirror of exactly one record)
    jn = sup.junction_list()
    assert (jn["via"] & 1 == 0).all() and (jn["count"] > 0).all() and int(jn["count"].sum()) == sup.t["passages"] and (jn["reserved"] == 0).all()
    keys = [(int(j["via"]), int(j["from"]), int(j["to"])) for j in jn]
    assert keys == sorted(set(keys))
    mt = sup.mate_list()
    pairs = [(int(m["from"]), int(m["to"])) for m in mt]
    assert pairs == sorted(set(pairs)) and all((a, b) <= (b ^ 1, a ^ 1) and a != b for a, b in pairs) and int(mt["pairs"].sum()) == sup.t["pairs_linked"]
    assert sup.t["pairs_placed"] == sup.t["pairs_within"] + sup.t["pairs_linked"] and sup.t["pairs"] == (len(reads) // 2 if paired else 0)
    # a read and its reverse complement give the same tallies; a pair and its swapped pair -- the same fragment from its other strand --
    # the same mate link
    other = su.Support(sup.th)
    if paired:
        other.add([r for a, b in zip(reads[0::2], reads[1::2]) for r in (b, a)], True)
    else:
        other.add([cu.revcomp(r) for r in reads])
    assert other.segs == sup.segs and other.kmers == sup.kmers and other.junctions == sup.junctions and other.mates == sup.mates
    assert other.links().tolist() == [(b, a) for a, b in sup.links().tolist()] if not paired else True
    return linked


@pytest.mark.parametrize("K", [23, 33, 65, 97])
def test_bubble_cases_on_the_model(K):
    reads = bu.built_case(K)["counted"]
    for mc in (2, 1):
        assert consequences(su.bubble_support(K, mc, 1), *tu.bubble_records(K, mc, 1), reads, False) > 250
        th = tu.bubble_threading(K, mc, 1)
        consequences(su.bubble_pairs_support(K, mc, 1), *th.records(su.even(reads)), su.even(reads), True)


@pytest.mark.parametrize("K", [23, 33, 65, 97])
def test_cluster_cases_on_the_model(K):
    case = cu.built_case(K)
    for name in cu.PARAM_SETS:
        consequences(su.cluster_support(K, name, True), *tu.cluster_records(K, name), case["query"], True)
        consequences(su.cluster_support(K, name), *tu.cluster_records(K, name), case["query"], False)
    # polyA: every position after the first is a traversal of the self link of A^K and, from the third on, the passage (u, u, u)
    base = su.cluster_support(K, "base")
    n = len(case["query"][case["at"]["polyA"]]) - K + 1
    u = tu.cluster_threading(K, "base").place(0)[0]
    assert base.junctions[(u << 1, u << 1, u << 1)] >= n - 2 and base.along[(u << 1, 0)] >= n - 1


def test_hand_made_cases_on_the_model():
    """the cases of the GPU tests assert their own points when they are made"""
    case = su.boundary_case()
    assert len(case["pairs"]) == 9 and len(case["reads"]) == 6
    sup = su.Support(case["th"]).add(list(case["reads"].values()))
    assert sup.t["no_record"] == 0 and sup.t["passages"] == 12 and len(sup.junctions) == 5
    su.cycle_case()


# ---- the device-free half of `sdt-kmers support` -----------------------------------------------------------------------------------------------
def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "support_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "support_host_check.c"), os.path.join(host, "supportsplit.c")], check=True)
    for name, sup in (("base", su.cluster_support(31, "base")), ("bubble", su.bubble_support(23, 2, 1)), ("cycle", su.Support(su.cycle_case()["th"]).add(su.cycle_case()["reads"])),
                      ("empty", su.Support(tu.cluster_threading(31, "base")))):
        out = tmp_path / name
        out.mkdir()
        su.write_records(str(out / "records.bin"), sup)
        r = subprocess.run([exe, str(out / "records.bin"), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and "support_host_check: ok" in r.stdout, r.stdout + r.stderr
        assert (out / "check.unitigSupport").read_text() == su.unitig_support_text(sup)
        assert (out / "check.linkSupport").read_text() == su.link_support_text(sup)
        assert (out / "check.junctions").read_text() == su.junctions_text(sup)
        assert (out / "check.summary").read_text() == su.summary_line(sup) + "\n"
    text = (tmp_path / "base" / "check.junctions").read_text()
    assert "+" in text and "-" in text and (tmp_path / "empty" / "check.junctions").read_text() == ""
    assert (tmp_path / "cycle" / "check.linkSupport").read_text() == "1 + 1 + 5 4\n"
