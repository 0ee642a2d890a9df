"""The rule of the read support tally (include/sdt_gpu.h: sdt_gpu_unitigs_support_*) restated in plain Python over
unitig_thread_util.Threading -- what the GPU tests and the command-line test expect -- and the texts of the outputs of `sdt-kmers
support` (which adds single reads: no mate links).  It works from the model's own segments, never from the library under test.  All comparisons against it are exact."""
import collections
import functools

import numpy as np

import bubble_util as bu
import read_cluster_util as cu
import unitig_thread_util as tu

UNITIG_DTYPE = np.dtype([("segs", np.uint64), ("kmers", np.uint64)])
LINK_DTYPE = np.dtype([("along", np.uint64), ("against", np.uint64)])
JUNCTION_DTYPE = np.dtype([(f, np.uint32) for f in ("from", "via", "to", "reserved")] + [("count", np.uint64)])
MATE_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("pairs", np.uint64)])
TOTALS = ("reads", "placed", "segments", "live", "traversals", "no_record", "passages", "pairs", "pairs_placed", "pairs_within", "pairs_linked", "dropped")


def fold_passage(f, v, t):
    """the form of a passage whose via has o = 0"""
    return (t ^ 1, v ^ 1, f ^ 1) if v & 1 else (f, v, t)


def fold_mate(a, b):
    """the smaller of a mate link's two forms"""
    return min((a, b), (b ^ 1, a ^ 1))


class Support:
    """the tally of a Threading: add() ADDS, like the library's add calls"""

    def __init__(self, th):
        self.th, self.m, self.K = th, th.m, th.K
        n = len(th.m.unitigs)
        self.segs, self.kmers = [0] * n, [0] * n
        self.along = collections.Counter()                    # (ou, b) -> traversals
        self.junctions = collections.Counter()                # (from, via, to), via with o = 0
        self.mates = collections.Counter()                    # (from, to), the smaller form
        self.t = dict.fromkeys(TOTALS, 0)
        self.slots = {(u << 1 | o, b) for u, _, o, _, b, _ in self.m.links}
        self.mirror_base = {(u, o, v, o2): b for u, v, o, o2, b, _ in self.m.links}

    def add_read(self, codes):
        """-> the oriented unitig of the read's last segment, or None"""
        K, t = self.K, self.t
        one, segs = self.th.thread(codes)
        t["reads"] += 1
        t["placed"] += bool(segs)
        t["segments"] += len(segs)
        t["live"] += one[1]
        ou = [s[0] << 1 | s[1] & 1 for s in segs]
        for j, s in enumerate(segs):
            self.segs[s[0]] += 1
            self.kmers[s[0]] += s[4]
            if s[1] >> 1 != 1:
                continue
            b = int(codes[s[2] + K - 1])                      # the last base of w_p
            self.along[(ou[j - 1], b)] += 1
            t["traversals"] += 1
            t["no_record"] += (ou[j - 1], b) not in self.slots
            if segs[j - 1][1] >> 1 == 1:                       # both joins 1: a passage through the unitig of segment j - 1
                self.junctions[fold_passage(ou[j - 2], ou[j - 1], ou[j])] += 1
                t["passages"] += 1
        return ou[-1] if ou else None

    def add(self, reads, paired=False):
        assert not paired or len(reads) % 2 == 0
        last = [self.add_read(r) for r in reads]
        if paired:
            for a, b in zip(last[0::2], last[1::2]):
                self.t["pairs"] += 1
                if a is None or b is None:
                    continue
                self.t["pairs_placed"] += 1
                frm, to = a, b ^ 1                            # mate 2 is read against the fragment
                if frm == to:
                    self.t["pairs_within"] += 1
                else:
                    self.t["pairs_linked"] += 1
                    self.mates[fold_mate(frm, to)] += 1
        return self

    # ---- what the calls give
    def unitigs(self, first=0, n=None):
        last = len(self.segs) if n is None else first + n
        out = np.zeros(last - first, dtype=UNITIG_DTYPE)
        out["segs"], out["kmers"] = self.segs[first:last], self.kmers[first:last]
        return out

    def links(self, first=0, n=None):
        """parallel to Unitigs.link_records(first, n)"""
        last = len(self.segs) if n is None else first + n
        part = [l for l in self.m.links if first <= l[0] < last]
        out = np.zeros(len(part), dtype=LINK_DTYPE)
        for j, (u, v, o, o2, b, _) in enumerate(part):
            mb = self.mirror_base[(v, o2 ^ 1, u, o ^ 1)]      # the one record that leaves (to, o' ^ 1) for (from, o ^ 1)
            out[j] = (self.along[(u << 1 | o, b)], self.along[(v << 1 | o2 ^ 1, mb)])
        return out

    def junction_list(self):
        out = np.zeros(len(self.junctions), dtype=JUNCTION_DTYPE)
        for j, (f, v, t) in enumerate(sorted(self.junctions, key=lambda k: (k[1], k[0], k[2]))):
            out[j] = (f, v, t, 0, self.junctions[(f, v, t)])
        return out

    def mate_list(self):
        out = np.zeros(len(self.mates), dtype=MATE_DTYPE)
        for j, k in enumerate(sorted(self.mates)):
            out[j] = (k[0], k[1], self.mates[k])
        return out

    def totals(self):
        return np.array([self.t[k] for k in TOTALS], dtype=np.uint64)


def assert_support_equal(g, sup, what="", junctions=True, mates=True, totals=True):
    """every fetch of the context g against the model; the ranges in two pieces where there are two unitigs"""
    n = len(sup.segs)
    cut = n // 2
    for first, k in ((0, n), (0, cut), (cut, n - cut)):
        got, want = g.unitigs_support_unitigs(first, k), sup.unitigs(first, k)
        assert got.dtype == UNITIG_DTYPE and got.tolist() == want.tolist(), f"{what}: unitigs {first} + {k}"
        got, want = g.unitigs_support_links(first, k), sup.links(first, k)
        assert got.dtype == LINK_DTYPE and got.tolist() == want.tolist(), f"{what}: links {first} + {k}"
    if junctions:
        got, want = g.unitigs_support_junctions(), sup.junction_list()
        assert got.dtype == JUNCTION_DTYPE and got.tolist() == want.tolist(), f"{what}: junctions {got.tolist()[:6]} want {want.tolist()[:6]}"
    if mates:
        got, want = g.unitigs_support_mates(), sup.mate_list()
        assert got.dtype == MATE_DTYPE and got.tolist() == want.tolist(), f"{what}: mate links {got.tolist()[:6]} want {want.tolist()[:6]}"
    if totals:
        assert g.unitigs_support_totals().tolist() == sup.totals().tolist(), f"{what}: totals {g.unitigs_support_totals().tolist()} want {sup.totals().tolist()}"


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def ou_text(ou):
    return f"{(int(ou) >> 1) + 1}{'+-'[int(ou) & 1]}"


def unitig_support_text(sup):
    """out.unitigSupport: id segments kmers cov_x100 = 100 x kmers / nodes, a floor"""
    return "".join(f"{u + 1} {sup.segs[u]} {sup.kmers[u]} {100 * sup.kmers[u] // len(t['words'])}\n" for u, t in enumerate(sup.m.unitigs))


def link_support_text(sup):
    """out.linkSupport: the links that the GFA writes (the record that is <= its mirror): from o to o' along against"""
    ls = sup.links()
    return "".join(f"{u + 1} {'+-'[o]} {v + 1} {'+-'[o2]} {int(ls['along'][j])} {int(ls['against'][j])}\n"
                   for j, (u, v, o, o2, _, _) in enumerate(sup.m.links) if (u, o, v, o2) <= (v, 1 - o2, u, 1 - o))


def junctions_text(sup):
    return "".join(f"{ou_text(j['from'])} {ou_text(j['via'])} {ou_text(j['to'])} {int(j['count'])}\n" for j in sup.junction_list())


def summary_line(sup):
    t = sup.t
    return (f"support: reads {t['reads']} placed {t['placed']} segments {t['segments']} kmers {t['live']} traversals {t['traversals']} "
            f"no_record {t['no_record']} passages {t['passages']} junctions {len(sup.junctions)} dropped {t['dropped']}")


def write_records(path, sup):
    """the binary that tools/support_host_check reads: K, unitigs, links, junctions as uint64, the twelve totals, then the unitig records,
    their tallies, the link records, their tallies and the junctions"""
    rec, (links, _) = sup.m.records(), sup.m.link_records()
    with open(path, "wb") as f:
        f.write(np.array([sup.K, len(rec), len(links), len(sup.junctions)], dtype=np.uint64).tobytes())
        f.write(sup.totals().tobytes())
        for a in (rec, sup.unitigs(), links, sup.links(), sup.junction_list()):
            f.write(np.ascontiguousarray(a).tobytes())


# ---- the models of the built cases, made once and shared by the tests that need them --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bubble_support(K, min_count, min_link, paired=False):
    """the counted reads of the bubble case, all in one add"""
    return Support(tu.bubble_threading(K, min_count, min_link)).add(bu.built_case(K)["counted"], paired)


@functools.lru_cache(maxsize=None)
def cluster_support(K, name, paired=False):
    return Support(tu.cluster_threading(K, name)).add(cu.built_case(K)["query"], paired)


def even(reads):
    """a list of reads cut to an even number: reads 2r and 2r + 1 as mates"""
    return list(reads[:len(reads) - len(reads) % 2])


@functools.lru_cache(maxsize=None)
def bubble_pairs_support(K, min_count, min_link):
    return Support(tu.bubble_threading(K, min_count, min_link)).add(even(bu.built_case(K)["counted"]), True)


# ---- graphs written by hand: where the unitigs end is where the test needs it ----------------------------------------------------------------
def forked(main, cuts, K, rng):
    """the sequences of a hand graph: main, and per cut i a fork that leaves k-mer i - 1 of main by another base, so that the k-mers
    i - 1 and i of main lie in different unitigs"""
    seqs = [np.asarray(main, dtype=np.uint8)]
    for i in cuts:
        seqs.append(np.concatenate([main[i - 1:i - 1 + K], [(int(main[i - 1 + K]) + 1) & 3], rng.integers(0, 4, size=6)]).astype(np.uint8))
    return seqs


@functools.lru_cache(maxsize=None)
def boundary_case(K=23):
    """two lines of 140 k-mers.  m1 is cut before its k-mers 63, 64, 127 and 128: a read over it has links at lanes 63 and 0 of consecutive
    steps, so the passage found at lane 0 has its earlier start in the step before.  m2 is cut before 60, 130 and 135: the passage found at
    130 has its earlier start two steps before, behind a unitig of 70 nodes.  -> dict: nodes, th, reads (name -> codes), pairs (name ->
    (mate 1, mate 2))"""
    import unitig_util as uu
    rng = np.random.default_rng(5 + K)
    m1, m2 = (rng.integers(0, 4, size=140 + K - 1, dtype=np.uint8) for _ in range(2))
    nodes = bu.hand_graph(forked(m1, (63, 64, 127, 128), K, rng) + forked(m2, (60, 130, 135), K, rng), K)
    th = tu.Threading(uu.Unitigs(bu.as_model_nodes(nodes), K, min_count=1))
    reads = dict(two_steps=m1[:64 + K], three_steps=m1[:130 + K - 1], long_between=m2)
    starts = lambda r: [(s[2], s[1] >> 1) for s in th.thread(r)[1]]
    assert starts(reads["two_steps"]) == [(0, 0), (63, 1), (64, 1)]
    assert starts(reads["three_steps"]) == [(0, 0), (63, 1), (64, 1), (127, 1), (128, 1)]
    assert starts(reads["long_between"]) == [(0, 0), (60, 1), (130, 1), (135, 1)] and th.thread(m2)[1][1][4] == 70
    for name in list(reads):
        reads[name + "_rc"] = cu.revcomp(reads[name])
    # pairs over m1: its k-mers 0 .. 62 are one unitig (a), 64 .. 126 another (b)
    cut = lambda lo, n: m1[lo:lo + n + K - 1]
    a1, a2, b1 = cut(0, 30), cut(20, 30), cut(70, 30)
    rc = cu.revcomp
    pairs = dict(fr=(a1, rc(b1)), fr_mirror=(rc(b1), a1), both_rc=(rc(a1), b1), same_strand=(a1, b1), unplaced=(a1, rng.integers(0, 4, size=60, dtype=np.uint8)),
                 short=(a1, b1[:K - 1]), within=(a1, rc(a2)), within_rc=(a2, rc(a1)), turn=(a1, a2))
    (ua, _, oa), (ub, _, ob) = th.place(cu.kmer_ints(a1, K)[0][0]), th.place(cu.kmer_ints(b1, K)[0][0])
    assert ua != ub and th.thread(a1)[0][2] == th.thread(a2)[0][2] == th.thread(b1)[0][2] == 1
    A, B = ua << 1 | oa, ub << 1 | ob
    want = dict(fr=fold_mate(A, B), fr_mirror=fold_mate(A, B), both_rc=fold_mate(A ^ 1, B ^ 1), same_strand=fold_mate(A, B ^ 1), unplaced=None, short=None,
                within=None, within_rc=None, turn=fold_mate(A, A ^ 1))
    for name, (x, y) in pairs.items():
        s = Support(th).add([x, y], True)
        assert list(s.mates) == ([want[name]] if want[name] else []), name
        assert s.t["pairs_within"] == (name in ("within", "within_rc")) and s.t["pairs_placed"] == (name not in ("unplaced", "short")), name
    assert fold_mate(A, A ^ 1) == (A, A ^ 1)                   # (its own mirror)
    return dict(K=K, nodes=nodes, th=th, reads=reads, pairs=pairs)


@functools.lru_cache(maxsize=None)
def cycle_case(K=23, n=40):
    """a circular unitig walked more than twice from its x0 and from 7 nodes on, on both strands: the closing link, and the passage
    (u, u, u) -> dict: nodes, th, reads"""
    import unitig_util as uu
    nodes = uu.cycle_graph(K, n, 3)
    m = uu.Unitigs(bu.as_model_nodes(nodes), K, min_count=1)
    th = tu.Threading(m)
    ring = np.array(m.codes(0)[:n], dtype=np.uint8)
    read = np.concatenate([ring, ring, ring])[:85 + K - 1]
    half = np.concatenate([ring, ring])[20:20 + 60 + K - 1]      # one and a half times round: one closing link, no passage
    reads = [read, cu.revcomp(read), read[7:], cu.revcomp(read[7:]), half]
    s = Support(th).add(reads)
    assert dict(s.junctions) == {(0, 0, 0): 4} and s.t["traversals"] == 9 and s.t["no_record"] == 0 and len(m.links) == 2
    assert sorted(s.links().tolist()) == [(4, 5), (5, 4)]
    return dict(K=K, nodes=nodes, th=th, reads=reads)
