"""CPU: the surface of read threading (header, exported symbols, binding), the Python restatement of its rule (unitig_thread_util.py) on
the cases of the GPU tests, on a unitig's own sequence and on a cycle, the device-free half of `sdt-kmers thread` (threadsplit.c) through
tools/thread_host_check built under AddressSanitizer + UBSan as a program of its own, and the option table of the built tool."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bubble_util as bu
import read_cluster_util as cu
import unitig_thread_util as tu
import unitig_util as uu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CALLS = ("index", "lookup", "reads", "reads_device")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    lib = pkg.load_library()
    for proto in ("int sdt_gpu_unitigs_index(sdt_ctx *ctx, uint64_t info[4]);",
                  "int sdt_gpu_unitigs_lookup(sdt_ctx *ctx, const uint64_t *keys, uint64_t n, sdt_unitig_pos *out);",
                  "int sdt_gpu_unitigs_reads(sdt_ctx *ctx, const uint32_t *packed_words, uint64_t nwords, const uint64_t *offsets, uint64_t nreads, "
                  "sdt_read_path *rec, uint64_t *seg_offsets, sdt_path_seg *segs, uint64_t capacity, uint64_t *n_segs);",
                  "int sdt_gpu_unitigs_reads_device(sdt_ctx *ctx, const void *d_packed_words, const void *d_offsets, uint64_t nreads, void *d_rec, "
                  "void *d_seg_offsets, void *d_segs, uint64_t capacity, uint64_t *n_segs);"):
        assert proto in code, proto
    for c in CALLS:
        assert hasattr(lib, f"sdt_gpu_unitigs_{c}") and f"sdt_gpu_unitigs_{c}" in pkg.ABI_SYMBOLS
        assert hasattr(pkg.PregraphGPU, f"unitigs_{c}")
    assert "typedef struct { uint32_t unitig, pos, info, reserved; } sdt_unitig_pos;" in code
    assert "typedef struct { uint32_t kmers, live, segs, breaks, first, last; } sdt_read_path;" in code
    assert "typedef struct { uint32_t unitig, info, read_pos, unitig_pos, kmers, reserved; } sdt_path_seg;" in code
    assert "#define SDT_UNITIG_NONE 0xFFFFFFFFu" in code and pkg.UNITIG_NONE == tu.NONE
    assert "#define SDT_ABI_VERSION 8" in code and lib.sdt_gpu_abi_version() == 8
    for word in ("LABEL.", "PLACEMENT.", "CONTINUES", "no sdt_gpu_unitigs_index", "SEGMENT RECORD", "READ RECORD", "mate links between unitigs"):
        assert word in src, word
    assert pkg.READ_PATH_DTYPE == tu.REC_DTYPE and pkg.READ_PATH_DTYPE.itemsize == 24 and pkg.READ_PATH_DTYPE.names == tu.REC_FIELDS
    assert pkg.PATH_SEG_DTYPE == tu.SEG_DTYPE and pkg.PATH_SEG_DTYPE.itemsize == 24 and pkg.PATH_SEG_DTYPE.names == tu.SEG_FIELDS
    assert pkg.UNITIG_POS_DTYPE == tu.POS_DTYPE and pkg.UNITIG_POS_DTYPE.itemsize == 16


# ---- the restatement on its cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [23, 31, 33, 65, 97])
def test_bubble_cases_on_the_model(K):
    """the counted reads of the bubble case: their segments sum to live, at min_count 1 every k-mer is live, no transition is unlinked,
    every linked one is a link of the list between the ends of two unitigs, and a read has three segments at the most"""
    for mc, ml in ((1, 1), (2, 1), (2, 2)):
        th = tu.bubble_threading(K, mc, ml)
        rec, offs, segs = tu.bubble_records(K, mc, ml)
        assert tu.check_consequences(th, rec, offs, segs) == int((segs["info"] >> 1 == 1).sum())
        assert int((segs["info"] >> 1 == 2).sum()) == 0 and int(rec["segs"].max()) == 3
        assert mc != 1 or (rec["live"] == rec["kmers"]).all()
        if K != 97:
            assert 316 <= int((segs["info"] >> 1 == 1).sum()) <= 415, (K, mc, ml)
        assert (segs["reserved"] == 0).all() and (segs["kmers"] > 0).all()
        assert offs.tolist() == [0] + np.cumsum(rec["segs"]).tolist()


@pytest.mark.parametrize("K", [31, 97])
def test_cluster_cases_on_the_model(K):
    case = cu.built_case(K)
    at, query = case["at"], case["query"]
    of = lambda name, read: (lambda r, o, s: s[int(o[read]):int(o[read + 1])])(*tu.cluster_records(K, name))
    pa = of("base", at["polyA"])
    assert len(pa) == {31: 70, 97: 108}[K] == len(query[at["polyA"]]) - K + 1      # every k-mer is A^K: a segment of one k-mer each ...
    assert (pa["info"][1:] >> 1 == 1).all() and pa["info"][0] >> 1 == 0 and (pa["kmers"] == 1).all()      # ... joined by the self link of A^K
    assert len(set(pa["unitig"].tolist())) == 1 and len(set(pa["unitig_pos"].tolist())) == 1
    assert len(of("hub_cut", at["polyA"])) == 0                                  # (above max_count: not live)
    jn = of("base", at["junction"])
    assert len(jn) == 1 and jn["kmers"][0] == len(query[at["junction"]]) - K + 1
    cut = of("link_cut", at["junction"])
    assert len(cut) == 2 and cut["info"][1] >> 1 == 2 and int(cut["kmers"].sum()) == jn["kmers"][0] and cut["read_pos"][1] == cut["kmers"][0]
    if K == 31:
        assert cut["kmers"].tolist() == [35, 35] and cut["read_pos"].tolist() == [0, 35]
    for name in cu.PARAM_SETS:
        rec, offs, segs = tu.cluster_records(K, name)
        later = np.ones(len(segs), dtype=bool)
        later[offs[:-1][rec["segs"] > 0].astype(np.int64)] = False               # not the first segment of its read
        join = segs["info"] >> 1
        assert int((join == 2).sum()) == (1 if name == "link_cut" else 0), name
        if name == "base":
            assert int((later & (join == 0)).sum()) == 2                         # the gaps: weak_middle, and bridge
        assert (join[~later] == 0).all()
        assert rec["breaks"].tolist() == [int((later & (join != 1))[int(a):int(b)].sum()) for a, b in zip(offs, offs[1:])]
    rec = tu.cluster_records(K, "base")[0]
    assert rec["kmers"][at["short_pair"]] == 0 and rec["first"][at["short_pair"]] == tu.NONE and rec["segs"][at["mate_unassigned"] + 1] == 0


@pytest.mark.parametrize("K", [23, 65])
def test_a_unitig_is_one_segment_of_itself(K):
    th = tu.bubble_threading(K, 2, 1)
    m = th.m
    for i in range(len(m.unitigs)):
        n = len(m.unitigs[i]["words"])
        codes = np.array(m.codes(i), dtype=np.uint8)
        one, segs = th.thread(codes)
        assert one == (n, n, 1, 0, i, i) and segs == [[i, 0, 0, 0, n, 0]]
        one, segs = th.thread(cu.revcomp(codes))
        assert one == (n, n, 1, 0, i, i) and segs == [[i, 1, 0, n - 1, n, 0]]
        assert th.lookup([m.unitigs[i]["words"][0], cu.rc_int(m.unitigs[i]["words"][0], K)]).tolist() == [(i, 0, 0, 0), (i, 0, 1, 0)]


def test_round_a_cycle_on_the_model():
    """going round a circular unitig is no continuation: the closing link is a link"""
    K, n = 23, 40
    c = np.random.default_rng(3).integers(0, 4, size=n, dtype=np.uint8)
    m = uu.Unitigs(bu.as_model_nodes(uu.cycle_graph(K, n, 3)), K, min_count=1)
    assert m.info[:4] == [n, 0, 1, 1]
    th = tu.Threading(m)
    x0 = m.unitigs[0]["words"][0]
    fw = cu.kmer_ints(np.concatenate([c, c[:K]]), K)[0]
    if x0 not in fw:                                          # the cycle is reported on the other strand: read it that way
        c = cu.revcomp(c)
        fw = cu.kmer_ints(np.concatenate([c, c[:K]]), K)[0]
    start = fw.index(x0)
    ring = np.concatenate([c[start:], c[:start]])
    read = np.concatenate([ring, ring, ring])[:85 + K - 1]
    one, segs = th.thread(read)
    assert one == (85, 85, 3, 0, 0, 0) and segs == [[0, 0, 0, 0, 40, 0], [0, 0 | 1 << 1, 40, 0, 40, 0], [0, 0 | 1 << 1, 80, 0, 5, 0]]
    one, segs = th.thread(cu.revcomp(read))
    assert one == (85, 85, 3, 0, 0, 0) and segs == [[0, 1, 0, 4, 5, 0], [0, 1 | 1 << 1, 5, 39, 40, 0], [0, 1 | 1 << 1, 45, 39, 40, 0]]


# ---- the device-free half of `sdt-kmers thread` ----------------------------------------------------------------------------------------------
def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "thread_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "thread_host_check.c"), os.path.join(host, "threadsplit.c")], check=True)
    for K, name in ((31, "base"), (31, "link_cut")):
        rec, offs, segs = tu.cluster_records(K, name)
        n = len(tu.cluster_threading(K, name).m.unitigs)
        out = tmp_path / name
        out.mkdir()
        tu.write_records(str(out / "records.bin"), K, n, rec, offs, segs)
        r = subprocess.run([exe, str(out / "records.bin"), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and "thread_host_check: ok" in r.stdout, r.stdout + r.stderr
        assert (out / "check.readPaths").read_text() == tu.read_paths_text(rec, offs, segs)
        assert (out / "check.unitigReads").read_text() == tu.unitig_reads_text(n, rec, offs, segs)
        assert (out / "check.summary").read_text() == tu.summary_line(rec, segs) + "\n"
    text = (tmp_path / "link_cut" / "check.readPaths").read_text()
    assert "~" in text and "/" in text and "-" in text and "\n0 0 0 0 *\n" in text and "<" in text and ">" in text


# ---- the option table of the built tool ------------------------------------------------------------------------------------------------------------
def test_sdt_kmers_options(pkg, tmp_path):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "thread"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers thread -s lib.cfg" in r.stderr and "prefix.readPaths" in r.stderr and "prefix.unitigReads" in r.stderr
    out = str(tmp_path / "none")
    for opt, val, owner in (("--pick", "1:2", "cluster"), ("--max-branch", "5", "bubbles")):
        r = subprocess.run([exe, "thread", "-s", "none.cfg", "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode == 255 and f"sdt-kmers: {opt} belongs to {owner}\n" in r.stderr
    for opt, val in (("--max-count", "5"), ("--min-link", "2"), ("-c", "3")):
        # thread takes them: what stops the run is the config that is not there
        r = subprocess.run([exe, "thread", "-s", str(tmp_path / "none.cfg"), "-o", out, opt, val], capture_output=True, text=True)
        assert r.returncode != 0 and "belongs to" not in r.stderr and "usage:" not in r.stderr, r.stderr[:300]
    for args in (["--min-link", "0"], ["--min-link", "64"], ["-c", "5", "--max-count", "4"]):
        r = subprocess.run([exe, "thread", "-s", "none.cfg", "-o", out] + args, capture_output=True, text=True)
        assert r.returncode == 255 and args[-2] in r.stderr, (args, r.stderr[:200])
    assert os.listdir(tmp_path) == []                     # nothing is written
