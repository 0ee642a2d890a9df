"""The rule of read threading (include/sdt_gpu.h: sdt_gpu_unitigs_index / _lookup / _reads) restated in plain Python over
unitig_util.Unitigs -- what the GPU tests and the command-line test expect -- and the texts of the outputs of `sdt-kmers thread`.  The
nodes come from the oracle or are written by hand, never from the library under test.  All comparisons against it are exact."""
import functools

import numpy as np

import bubble_util as bu
import read_cluster_util as cu
import unitig_util as uu
from read_cluster_util import kmer_ints, rc_int

NONE = 0xFFFFFFFF
POS_FIELDS = ("unitig", "pos", "info", "reserved")
POS_DTYPE = np.dtype([(f, np.uint32) for f in POS_FIELDS])
REC_FIELDS = ("kmers", "live", "segs", "breaks", "first", "last")
REC_DTYPE = np.dtype([(f, np.uint32) for f in REC_FIELDS])
SEG_FIELDS = ("unitig", "info", "read_pos", "unitig_pos", "kmers", "reserved")
SEG_DTYPE = np.dtype([(f, np.uint32) for f in SEG_FIELDS])


class Threading:
    """index: canonical k-mer -> (u, i, s) of LABEL, from the words of the model's unitigs"""

    def __init__(self, model):
        self.m, self.K, self.nodes, self.min_link = model, model.K, model.nodes, model.g.min_link
        self.index = {}
        for u, t in enumerate(model.unitigs):
            for i, x in enumerate(t["words"]):
                c = min(x, rc_int(x, self.K))
                assert c not in self.index, "a node lies in two unitigs"
                self.index[c] = (u, i, 0 if x == c else 1)
        assert len(self.index) == model.info[0]

    def place(self, w):
        """PLACEMENT of the word w as given -> (u, i, o), or None where its node is not live"""
        c = min(w, rc_int(w, self.K))
        if c not in self.index:
            return None
        u, i, s = self.index[c]
        return u, i, s if w == c else s ^ 1

    def thread(self, codes):
        """one read -> ((kmers, live, segs, breaks, first, last), [[unitig, info, read_pos, unitig_pos, kmers, 0]])"""
        K = self.K
        fw = kmer_ints(codes, K)[0] if len(codes) >= K else []
        places = [self.place(w) for w in fw]
        segs = []
        for p, pl in enumerate(places):
            if pl is None:
                continue
            prev = places[p - 1] if p else None
            if prev is not None and prev[0] == pl[0] and prev[2] == pl[2] and pl[1] == prev[1] + (1 if pl[2] == 0 else -1):
                segs[-1][4] += 1                              # CONTINUES: no modular arithmetic, the closing link of a cycle is a link
                continue
            join = 0 if prev is None else 1 if bu.get_link(self.nodes, fw[p - 1], fw[p] & 3, K) >= self.min_link else 2
            segs.append([pl[0], pl[2] | join << 1, p, pl[1], 1, 0])
        live = sum(pl is not None for pl in places)
        assert sum(s[4] for s in segs) == live
        breaks = sum(s[1] >> 1 != 1 for s in segs[1:])
        return (len(fw), live, len(segs), breaks, segs[0][0] if segs else NONE, segs[-1][0] if segs else NONE), segs

    def records(self, reads):
        """-> (REC_DTYPE[n], seg_offsets uint64[n + 1], SEG_DTYPE[total])"""
        rec = np.zeros(len(reads), dtype=REC_DTYPE)
        offs = np.zeros(len(reads) + 1, dtype=np.uint64)
        allsegs = []
        for r, codes in enumerate(reads):
            one, segs = self.thread(codes)
            rec[r] = one
            allsegs += segs
            offs[r + 1] = len(allsegs)
        out = np.zeros(len(allsegs), dtype=SEG_DTYPE)
        for j, s in enumerate(allsegs):
            out[j] = tuple(s)
        return rec, offs, out

    def lookup(self, words):
        out = np.zeros(len(words), dtype=POS_DTYPE)
        for j, w in enumerate(words):
            pl = self.place(w)
            out[j] = (NONE, 0, 0, 0) if pl is None else (pl[0], pl[1], pl[2], 0)
        return out

    def link_set(self):
        """(u, o, v, o', b) of every link of the model"""
        return {(u, o, v, o2, b) for u, v, o, o2, b, _ in self.m.links}


def assert_threading_equal(got, want, what=""):
    """(rec, seg_offsets, segs) against the model's"""
    for name, dtype, fields, g, w in (("rec", REC_DTYPE, REC_FIELDS, got[0], want[0]), ("segs", SEG_DTYPE, SEG_FIELDS, got[2], want[2])):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        for f in fields:
            bad = np.nonzero(g[f] != w[f])[0]
            assert bad.size == 0, f"{what}: {name}.{f} differs at {bad[:8].tolist()}: got {g[f][bad[:8]].tolist()} want {w[f][bad[:8]].tolist()}"
    assert got[1].tolist() == want[1].tolist(), f"{what}: seg_offsets"


def check_consequences(th, rec, offs, segs):
    """what the rule promises for a table that pass 1 counted, on any (rec, seg_offsets, segs): a join-1 segment starts at the in end
    of its oriented unitig, the one before it ends at the out end of its own, the two make a link of the list, and a read's segments sum
    to its live k-mers.  -> the number of join-1 transitions"""
    nodes_of = [len(t["words"]) for t in th.m.unitigs]
    links = {(u, o, v, o2) for u, o, v, o2, _ in th.link_set()}
    linked = 0
    for r in range(len(rec)):
        mine = segs[int(offs[r]):int(offs[r + 1])]
        assert int(mine["kmers"].sum()) == int(rec["live"][r]) and len(mine) == int(rec["segs"][r]), r
        for a, b in zip(mine, mine[1:]):
            if int(b["info"]) >> 1 != 1:
                continue
            linked += 1
            u, o, v, o2 = int(a["unitig"]), int(a["info"]) & 1, int(b["unitig"]), int(b["info"]) & 1
            assert int(b["unitig_pos"]) == (0 if o2 == 0 else nodes_of[v] - 1), (r, "a linked segment starts at the in end")
            end = int(a["unitig_pos"]) + (int(a["kmers"]) - 1) * (1 if o == 0 else -1)
            assert end == (nodes_of[u] - 1 if o == 0 else 0), (r, "the segment before a link ends at the out end")
            assert (u, o, v, o2) in links, (r, u, o, v, o2)
            assert int(b["read_pos"]) == int(a["read_pos"]) + int(a["kmers"])
    return linked


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def path_text(segs):
    if len(segs) == 0:
        return "*"
    out = []
    for j, s in enumerate(segs):
        o, join = int(s["info"]) & 1, int(s["info"]) >> 1
        sep = "" if j == 0 else {0: "/", 1: "-", 2: "~"}[join]
        out.append(f"{sep}{'><'[o]}{int(s['unitig']) + 1}:{int(s['unitig_pos'])}+{int(s['kmers'])}")
    return "".join(out)


def read_paths_text(rec, offs, segs):
    """out.readPaths: kmers live segs breaks path"""
    return "".join(f"{r['kmers']} {r['live']} {r['segs']} {r['breaks']} {path_text(segs[int(offs[i]):int(offs[i + 1])])}\n" for i, r in enumerate(rec))


def unitig_reads_text(n_unitigs, rec, offs, segs):
    """out.unitigReads: id reads segments kmers; reads = the reads with at least one segment in the unitig"""
    reads, nseg, kmers = [0] * n_unitigs, [0] * n_unitigs, [0] * n_unitigs
    for i in range(len(rec)):
        mine = segs[int(offs[i]):int(offs[i + 1])]
        for u in set(mine["unitig"].tolist()):
            reads[u] += 1
        for s in mine:
            nseg[int(s["unitig"])] += 1
            kmers[int(s["unitig"])] += int(s["kmers"])
    return "".join(f"{u + 1} {reads[u]} {nseg[u]} {kmers[u]}\n" for u in range(n_unitigs))


def summary_line(rec, segs):
    placed = rec["segs"] > 0
    whole = placed & (rec["live"] == rec["kmers"]) & (rec["breaks"] == 0)
    short = rec["kmers"] == 0
    join = segs["info"] >> 1
    return (f"thread: reads {len(rec)} placed {int(placed.sum())} whole {int(whole.sum())} broken {int((placed & ~whole).sum())} "
            f"unplaced {int((~placed & ~short).sum())} short {int(short.sum())} segments {len(segs)} linked {int((join == 1).sum())} "
            f"unlinked {int((join == 2).sum())}")


def write_records(path, K, n_unitigs, rec, offs, segs):
    """the binary that tools/thread_host_check reads: K, unitigs, reads, segments as uint64, then rec, seg_offsets, segs"""
    with open(path, "wb") as f:
        f.write(np.array([K, n_unitigs, len(rec), len(segs)], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rec).tobytes())
        f.write(np.ascontiguousarray(offs, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(segs).tobytes())


# ---- the models of the built cases, made once and shared by the tests that need them --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bubble_threading(K, min_count, min_link):
    return Threading(uu.Unitigs(bu.built_case(K)["nodes"], K, min_count=min_count, max_count=0, min_link=min_link))


@functools.lru_cache(maxsize=None)
def bubble_records(K, min_count, min_link):
    """the counted reads of the bubble case through the model -> (rec, seg_offsets, segs)"""
    return bubble_threading(K, min_count, min_link).records(bu.built_case(K)["counted"])


@functools.lru_cache(maxsize=None)
def cluster_threading(K, name):
    return Threading(uu.Unitigs(cu.built_case(K)["nodes"], K, **cu.PARAM_SETS[name]))


@functools.lru_cache(maxsize=None)
def cluster_records(K, name):
    return cluster_threading(K, name).records(cu.built_case(K)["query"])
