"""CPU: the surface of the read clustering (header, exported symbols, binding), the Python restatement of its rule (read_cluster_util.py)
against a second one that works on strings with a reachability matrix, the symmetries of the rule on the model, the cases of the GPU
tests, and the device-free half of `sdt-kmers cluster` (clustersplit.c) through tools/cluster_host_check built under
AddressSanitizer + UBSan as a program of its own."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import read_cluster_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CALLS = ("begin", "components", "lookup", "reads", "reads_device", "kept_reads", "end")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(pkg):
    src = open(os.path.join(ROOT, "include", "sdt_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.load_library()
    for c in CALLS:
        assert re.search(r"\bint sdt_gpu_cluster_%s\(sdt_ctx \*ctx" % c, code), c
        assert hasattr(lib, f"sdt_gpu_cluster_{c}") and f"sdt_gpu_cluster_{c}" in pkg.ABI_SYMBOLS
        assert hasattr(pkg.PregraphGPU, f"cluster_{c}")
    assert "typedef struct { uint32_t min_count, max_count, min_link, flags; } sdt_cluster_params;" in code
    assert "typedef struct { uint64_t count_sum; uint32_t nodes, reserved; } sdt_cluster_comp;" in code
    assert "typedef struct { uint32_t kmers, live, split, cluster, unit, verdict; } sdt_read_cluster;" in code
    assert "#define SDT_CLUSTER_NONE 0xFFFFFFFFu" in code
    assert "#define SDT_ABI_VERSION 8" in re.sub(r"[ \t]+", " ", code) and lib.sdt_gpu_abi_version() == 8
    for word in ("LIVE NODES", "EDGES", "CLUSTERS", "2^32 - 1 slots", "the table changed since sdt_gpu_cluster_begin", "SDT_EFULL when C > capacity"):
        assert word in src, word
    p = pkg.ClusterParams()
    assert (p.min_count, p.max_count, p.min_link, p.flags) == (2, 0, 1, 0) and ctypes.sizeof(p) == 16
    assert [f for f, _ in pkg.ClusterParams._fields_] == ["min_count", "max_count", "min_link", "flags"]
    assert pkg.CLUSTER_NONE == cu.NONE == 0xFFFFFFFF
    assert pkg.READ_CLUSTER_DTYPE == cu.DTYPE and pkg.READ_CLUSTER_DTYPE.itemsize == 24 and pkg.READ_CLUSTER_DTYPE.names == cu.FIELDS
    assert pkg.CLUSTER_COMP_DTYPE.itemsize == 16 and pkg.CLUSTER_COMP_DTYPE.names == ("count_sum", "nodes", "reserved")
    assert (pkg.CLUSTER_WHOLE, pkg.CLUSTER_NOT_WHOLE, pkg.CLUSTER_THROUGH_MATE, pkg.CLUSTER_UNASSIGNED, pkg.CLUSTER_SHORT) == (0, 1, 2, 3, 4)


def test_sdt_kmers_usage_knows_cluster(pkg):
    exe = os.path.join(pkg.CSRC_DIR, "sdt-kmers")
    if not os.path.exists(exe):
        pkg.build()
    r = subprocess.run([exe, "cluster"], capture_output=True, text=True)
    assert r.returncode == 255 and "sdt-kmers cluster -s lib.cfg" in r.stderr and "--pick LO:HI" in r.stderr
    for opt, val in (("--max-count", "5"), ("--min-link", "2"), ("--pick", "1:2")):
        r = subprocess.run([exe, "profile", "-s", "none.cfg", "-o", "none", opt, val], capture_output=True, text=True)
        assert r.returncode == 255 and f"sdt-kmers: {opt} belongs to cluster\n" in r.stderr
    for args in (["--min-link", "0"], ["--min-link", "64"], ["--pick", "0:3"], ["--pick", "3:2"], ["--pick", "7"], ["-c", "5", "--max-count", "4"]):
        r = subprocess.run([exe, "cluster", "-s", "none.cfg", "-o", "none"] + args, capture_output=True, text=True)
        assert r.returncode == 255 and args[-2] in r.stderr, (args, r.stderr[:200])


# ---- the restatement against one over strings ----------------------------------------------------------------------------------------------
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
ORDER = {c: i for i, c in enumerate("ACTG")}             # the numeric order of the key words: A < C < T < G


def s_rc(s):
    return "".join(COMP[c] for c in reversed(s))


def s_key(s):
    return [ORDER[c] for c in s]


def s_canon(s):
    return min(s, s_rc(s), key=s_key)


def string_nodes(reads, K):
    """canonical k-mer (a string) -> [count, links: 8 counters capped at 63, left A C T G then right A C T G], as pass 1 leaves them"""
    nodes = {}
    for r in reads:
        for i in range(len(r) - K + 1):
            w = r[i:i + K]
            prev, nxt = (r[i - 1] if i else None), (r[i + K] if i + K < len(r) else None)
            if s_canon(w) != w:                           # the node is the other strand: what follows the word precedes the node
                w, prev, nxt = s_rc(w), (COMP[nxt] if nxt else None), (COMP[prev] if prev else None)
            n = nodes.setdefault(w, [0, [0] * 8])
            n[0] += 1
            if prev:
                n[1]["ACTG".index(prev)] = min(63, n[1]["ACTG".index(prev)] + 1)
            if nxt:
                n[1][4 + "ACTG".index(nxt)] = min(63, n[1][4 + "ACTG".index(nxt)] + 1)
    return nodes


def brute_force(nodes, min_count, max_count, min_link):
    """clusters as lists of strings in id order, by a reachability matrix (Warshall) over the live nodes"""
    live = sorted((w for w, (c, _) in nodes.items() if c >= max(min_count, 1) and (max_count == 0 or c <= max_count)), key=s_key)
    at = {w: i for i, w in enumerate(live)}
    n = len(live)
    reach = np.eye(n, dtype=bool)
    ends = 0
    for w in live:
        for q, b in itertools.product(range(2), "ACTG"):
            if nodes[w][1][4 * q + "ACTG".index(b)] >= min_link:
                v = s_canon(b + w[:-1] if q == 0 else w[1:] + b)
                if v in at:
                    ends += 1
                    reach[at[w], at[v]] = reach[at[v], at[w]] = True
    for k in range(n):
        reach |= np.outer(reach[:, k], reach[k, :])
    seen, clusters = set(), []
    for i, w in enumerate(live):                          # (live is in key order: a cluster is met at its smallest k-mer)
        if i not in seen:
            members = [j for j in range(n) if reach[i, j]]
            seen.update(members)
            clusters.append([live[j] for j in members])
    return clusters, len(live), ends


def as_model_nodes(nodes):
    """string nodes in the form the restatement takes: int key -> (links word, count, deleted)"""
    out = {}
    for w, (c, links) in nodes.items():
        word = sum(v << (6 * i) for i, v in enumerate(links[:4])) | sum(v << (24 + 6 * i) for i, v in enumerate(links[4:]))
        out[int("".join(f"{ORDER[ch]:02b}" for ch in w), 2)] = (word, c, 0)
    return out


HAND_K = 5
HAND_READS = ["ACGTTGCA" + "T", "ACGTTGCAT", "GGATCCTAG", "GGATCCTAG", "CTAGGATC", "TTTTTTTT", "TTTTTTTT", "ATGCAACGA", "GATCCTAGA", "GATCCTAGA",
              "CCCGAT", "CCCGAT", "TACAAG", "TACAAG", "CAAGTG", "CAAGTG", "ACAAGT", "GACTTAGCCA", "TGGCTAAGTC", "AGCCATG", "AGCCATG", "CTTAGCCG"]


@pytest.mark.parametrize("prm", [(2, 0, 1), (1, 0, 1), (2, 0, 2), (2, 3, 1), (1, 0, 3), (3, 0, 1)])
def test_the_restatement_against_one_over_strings(prm):
    """a graph of about 20 nodes worked by hand at K = 5: a sequence read on both strands, a second one with a branch, a homopolymer
    whose node links to itself, and a junction whose link is seen once"""
    nodes = string_nodes(HAND_READS, HAND_K)
    assert 15 <= len(nodes) <= 30 and nodes["AAAAA"][0] == 8 and nodes["AAAAA"][1][0] > 0
    clusters, n_live, ends = brute_force(nodes, *prm)
    model = cu.Clustering(as_model_nodes(nodes), HAND_K, *prm)
    assert [[cu.kmer_text(k, HAND_K) for k in sorted(u for u, i in model.label.items() if i == c)] for c in range(len(model.comps))] == \
           [sorted(cl, key=s_key) for cl in clusters]
    assert model.info[:3] == [n_live, ends, len(clusters)] and model.info[5] == len(nodes) - n_live
    assert [cu.kmer_text(c[0], HAND_K) for c in model.comps] == [cl[0] for cl in clusters]
    assert [c[1] for c in model.comps] == [len(cl) for cl in clusters] and [c[2] for c in model.comps] == [sum(nodes[w][0] for w in cl) for cl in clusters]
    # the oracle's pass 1 leaves the same nodes as the strings do
    codes, offs = cu.concat([cu.codes_of(r) for r in HAND_READS])
    import oracle_binding as ob
    o = ob.Oracle(HAND_K, nsets=3)
    o.add_reads(codes, offs)
    assert cu.oracle_nodes(o) == as_model_nodes(nodes)


def test_the_hand_graph_is_what_it_is_meant_to_be():
    """every parameter moves the partition; min_link 2 cuts the one link seen once between nodes seen three times"""
    nodes = string_nodes(HAND_READS, HAND_K)
    parts = {prm: frozenset(frozenset(c) for c in brute_force(nodes, *prm)[0]) for prm in ((2, 0, 1), (1, 0, 1), (2, 0, 2), (2, 3, 1))}
    assert len(set(parts.values())) == 4
    assert len(parts[(2, 0, 2)]) == len(parts[(2, 0, 1)]) + 1 and nodes["ACAAG"][0] == 3 and nodes["ACAAG"][1][4 + "ACTG".index("T")] == 1


# ---- symmetries and the cases of the GPU tests -------------------------------------------------------------------------------------------------
def test_symmetries_on_the_model():
    """reverse-complementing every read, and permuting the reads, change nothing: not the nodes' clusters, not the records"""
    case = cu.built_case(31)
    codes, offs = case["reads"]
    reads = [codes[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(reads))
    variants = {"reverse complements": [cu.revcomp(r) for r in reads], "permuted": [reads[i] for i in order]}
    for name, prm in cu.PARAM_SETS.items():
        base = case["models"][name]
        for what, rs in variants.items():
            m = cu.Clustering(cu.oracle_nodes(cu.counted_oracle(*cu.concat(rs), 31)), 31, **prm)
            assert m.label == base.label and m.comps == base.comps and m.info == base.info, (name, what)
    base = case["models"]["base"]
    q = case["query"]
    rec = base.records(q, paired=True)[0]
    flipped = base.records([cu.revcomp(r) for r in q], paired=True)[0]
    single, sflipped = base.records(q)[0], base.records([cu.revcomp(r) for r in q])[0]
    assert (rec["kmers"] == flipped["kmers"]).all() and (rec["live"] == flipped["live"]).all()
    whole = single["split"] == 0                          # (a split read goes by its FIRST live k-mer, which is the last one of the other strand)
    assert whole.sum() > len(q) - 10 and (single[whole] == sflipped[whole]).all() and (sflipped["split"][~whole] > 0).all()
    perm = rng.permutation(len(q) // 2)
    shuffled = [q[2 * int(t) + m] for t in perm for m in range(2)]
    assert (base.records(shuffled, paired=True)[0] == rec.reshape(-1, 2)[perm].reshape(-1)).all()


@pytest.mark.parametrize("K", [23, 31, 47, 63, 95, 127, 33, 65, 97])
def test_the_cases_hold_what_they_are_built_for(K):
    """the builder asserts every property on the model (read_cluster_util.built_case): a case that lost one fails here"""
    case = cu.built_case(K)
    assert case["L"] == max(100, 2 * K + 10) and len(case["query"]) % 2 == 0


def test_pick_and_units_on_the_model():
    case = cu.built_case(31)
    m, q = case["models"]["base"], case["query"]
    rec, keep, kept = m.records(q, paired=True, pick=(2, 5))
    assert kept == int(((rec["unit"] >= 2) & (rec["unit"] <= 5)).sum()) > 0 and (keep[0::2] == keep[1::2]).all()
    assert m.records(q, paired=True, pick=(0, cu.NONE))[2] == int((rec["unit"] != cu.NONE).sum())      # NONE is never picked
    alone = m.records(q, units=[[0], [3, 2]])[0]
    assert alone["verdict"][1] == cu.NONE and alone["unit"][3] == alone["cluster"][3] and alone["unit"][2] == alone["cluster"][3]


# ---- the device-free half of `sdt-kmers cluster` -----------------------------------------------------------------------------------------------
class HandModel:
    K = 3
    comps = [(0x01, 2, 7), (0x07, 1, 70000), (0x2A, 3, 4000000000)]
    info = [6, 8, 3, 3, 2, 4, 0, 0]


HAND_REC = [(8, 8, 0, 0, 0, 0), (8, 7, 0, 0, 0, 0), (8, 8, 0, 0, 0, 1), (8, 8, 2, 2, 0, 1), (8, 0, 0, cu.NONE, 1, 2), (6, 6, 0, 1, 1, 0),
            (0, 0, 0, cu.NONE, cu.NONE, 4), (9, 0, 0, cu.NONE, cu.NONE, 3)]
HAND_LEN = [10, 10, 10, 10, 10, 8, 2, 11]


def test_files_and_summary_clean_under_sanitizers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "cluster_host_check")
    host = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc", "host")
    subprocess.run([cc, "-std=gnu11"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "cluster_host_check.c"), os.path.join(host, "clustersplit.c")], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "cluster_host_check: ok" in r.stdout, r.stdout + r.stderr
    # the texts it wrote for the example by hand are the restatement's
    rec = np.array(HAND_REC, dtype=cu.DTYPE)
    assert (tmp_path / "hand.readCluster").read_text() == cu.read_cluster_text(rec) == \
        "8 8 0 1 1 0\n8 7 0 1 1 0\n8 8 0 1 1 1\n8 8 2 3 1 1\n8 0 0 0 2 2\n6 6 0 2 2 0\n0 0 0 0 0 4\n9 0 0 0 0 3\n"
    assert (tmp_path / "hand.clusters").read_text() == cu.clusters_text(HandModel, rec, HAND_LEN) == \
        "1 AAC 2 7 4 40\n2 ACG 1 70000 2 18\n3 TTT 3 4000000000 0 0\n# live 6 link_ends 8 clusters 3 largest 3 unassigned 2\n"
    assert (tmp_path / "hand.summary").read_text() == cu.summary_line(HandModel, rec) + "\n"
