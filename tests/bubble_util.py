"""The rule of the bubble list (include/sdt_gpu.h: sdt_gpu_bubbles_*) restated in plain Python -- what the GPU tests and the
command-line test expect -- and the cases they run.  The nodes come from the oracle's export() (read_cluster_util.oracle_nodes), or are
written by hand, never from the library under test; oriented words, successors, the branch walk, the pairing and the order are plain
loops over a dictionary.  All comparisons against it are exact."""
import functools

import numpy as np

from read_cluster_util import (LETTERS, concat, counted_oracle, is_live, key_words, kmer_ints, kmer_text, oracle_nodes, rc_int, read_len_for,
                               revcomp, substituted, tiled)

FIELDS = ("sum_a", "sum_b", "len_a", "len_b", "min_a", "min_b", "src_count", "snk_count", "info", "reserved")
DTYPE = np.dtype([("sum_a", np.uint64), ("sum_b", np.uint64)] + [(f, np.uint32) for f in FIELDS[2:]])
DEFAULTS = dict(min_count=2, max_count=0, min_link=1, max_len=4000)


class Bubbles:
    """found: every (s, base_a, base_b, t, branch a, branch b) with a branch = (link, len, min, sum, bases), whether reported or not;
    bubbles: the reported ones in id order; info as sdt_gpu_bubbles_begin gives it"""

    def __init__(self, nodes, K, min_count=2, max_count=0, min_link=1, max_len=4000):
        self.nodes, self.K = nodes, K
        self.min_count, self.max_count, self.min_link, self.max_len = min_count, max_count, min_link, max_len
        self.mask, self.top = (1 << (2 * K)) - 1, 2 * (K - 1)
        live = [u for u, n in nodes.items() if is_live(n, min_count, max_count)]
        self.live = set(live)
        forks = branches = reached = 0
        self.found = []
        for u in live:
            for s in sorted({u, rc_int(u, K)}):               # (a palindrome is one oriented word)
                sc = self.succ(s, rc_int(s, K))
                if len(sc) < 2:
                    continue
                forks += 1
                branches += len(sc)
                ends = [(b, link, self.branch(y, ry)) for b, y, ry, link in sc]
                ends = [(b, link, r) for b, link, r in ends if r is not None]
                reached += len(ends)
                for i, (ba, la, (ta, *pa)) in enumerate(ends):
                    for bb, lb, (tb, *pb) in ends[i + 1:]:
                        if ta == tb:
                            self.found.append((s, ba, bb, ta, (la, *pa), (lb, *pb)))
        self.bubbles = sorted(f for f in self.found if f[0] <= rc_int(f[3], K))
        lens = [(f[4][1], f[5][1]) for f in self.bubbles]
        self.info = [len(live), forks, branches, reached, len(self.bubbles), sum(a + b + 2 for a, b in lens), max([max(p) for p in lens], default=0), 0]

    def node_of(self, x, rx):
        """(links, count) of the live node of the oriented word x, and whether x is its stored key; None: not live"""
        c = x if x <= rx else rx
        if c not in self.live:
            return None
        return self.nodes[c][0], self.nodes[c][1], x == c

    def succ(self, x, rx):
        """[(b, y, revcomp(y), link)] in ascending b"""
        links, _, fwd = self.node_of(x, rx)
        out = []
        for b in range(4):
            link = (links >> (24 + 6 * b if fwd else 6 * (b ^ 2))) & 63
            if link >= self.min_link:
                y, ry = ((x << 2) | b) & self.mask, (rx >> 2) | ((b ^ 2) << self.top)
                if self.node_of(y, ry) is not None:
                    out.append((b, y, ry, link))
        return out

    def branch(self, cur, rcur):
        """the branch whose first word is cur -> (t, len, min, sum, bases after the first) or None"""
        n, mn, total, bases = 0, None, 0, []
        while True:
            if len(self.succ(rcur, cur)) >= 2:
                return cur, n, mn or 0, total, bases
            sc = self.succ(cur, rcur)
            if len(sc) != 1 or n == self.max_len:
                return None
            count = self.node_of(cur, rcur)[1]
            n, mn, total = n + 1, count if mn is None else min(mn, count), total + count
            b, cur, rcur, _ = sc[0]
            bases.append(b)

    def count_of(self, x):
        return self.node_of(x, rc_int(x, self.K))[1]

    # ---- what the calls give
    def records(self):
        rec = np.zeros(len(self.bubbles), dtype=DTYPE)
        for i, (s, ba, bb, t, a, b) in enumerate(self.bubbles):
            rec[i] = (a[3], b[3], a[1], b[1], a[2], b[2], self.count_of(s), self.count_of(t), ba | bb << 2 | a[0] << 8 | b[0] << 16, 0)
        return rec

    def keys(self, nw):
        return np.array([[key_words(s, nw), key_words(t, nw)] for s, _, _, t, _, _ in self.bubbles], dtype=np.uint64).reshape(len(self.bubbles), 2, nw)

    def paths(self, first=0, n=None):
        """(bases uint8, offsets uint64[2 n + 1]) of bubbles first .. first + n - 1"""
        part = self.bubbles[first:] if n is None else self.bubbles[first:first + n]
        seqs = []
        for _, ba, bb, _, a, b in part:
            seqs += [[ba] + a[4], [bb] + b[4]]
        return concat(seqs)

    def alleles(self, i):
        """the two allele sequences of bubble i as text"""
        s, ba, bb, _, a, b = self.bubbles[i]
        return tuple(kmer_text(s, self.K) + "".join(LETTERS[c] for c in [base] + br[4]) for base, br in ((ba, a), (bb, b)))


def assert_bubbles_equal(g, model, info, what=""):
    """info, records, keys and paths of the whole list"""
    assert [int(x) for x in info] == model.info, (what, [int(x) for x in info], model.info)
    n = len(model.bubbles)
    keys, rec = g.bubbles_fetch(0, n)
    want = model.records()
    assert rec.dtype == DTYPE, rec.dtype
    for f in FIELDS:
        assert rec[f].tolist() == want[f].tolist(), f"{what}: field {f}: got {rec[f].tolist()[:8]} want {want[f].tolist()[:8]}"
    assert keys.tolist() == model.keys(g.nw).tolist(), f"{what}: the source and sink words differ"
    bases, offs = g.bubbles_paths(0, n)
    wb, wo = model.paths()
    assert offs.tolist() == wo.tolist(), f"{what}: path offsets"
    assert bases.tobytes() == wb.tobytes(), f"{what}: path bytes"


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def words_of(seq, K):
    """the canonical k-mers of a sequence, a set"""
    return set(kmer_ints(seq, K)[1])


@functools.lru_cache(maxsize=None)
def built_case(K, seed=0):
    """-> dict: K, L, reads (codes, offs), nodes (from the oracle), kmers_in_reads, node_count, counted (the reads, a list), parts (name ->
    the canonical k-mers of that construct), longest (the inner nodes of the long branch), model (DEFAULTS), model1 (min_count 1).  Every
    property the cases are for is asserted on the model here, so a case that lost its point fails without a GPU."""
    rng = np.random.default_rng(7000 * K + seed)
    L = read_len_for(K)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    other = lambda c, k=1: np.uint8((int(c) + k) & 3)
    flank = max(150, K + 40)
    plain = [rnd(int(rng.integers(max(300, L), 601))) for _ in range(12)]
    sub_ref = rnd(2 * flank + 1)
    sub_alt = substituted(sub_ref, flank)
    tri = [rnd(2 * flank + 1)]
    tri += [np.concatenate([tri[0][:flank], [other(tri[0][flank], k)], tri[0][flank + 1:]]).astype(np.uint8) for k in (1, 2)]
    del_ref = rnd(2 * flank + 5)
    del_alt = np.concatenate([del_ref[:flank], del_ref[flank + 5:]])
    skip_ref = rnd(2 * flank + 3 * K)
    skip_alt = np.concatenate([skip_ref[:flank], skip_ref[flank + 3 * K:]])
    two_ref = rnd(2 * flank + K // 2 + 1)
    two_alt = substituted(substituted(two_ref, flank), flank + K // 2)
    # a long branch against a direct edge: P + Q is counted, and P + X + Q where X ends in the last K - 1 bases of P, so that the k-mer
    # P[-(K - 1):] + Q[0] follows the last k-mer of P directly and closes the detour through X as well
    P, Q, m = rnd(flank), rnd(flank), 3000
    X = np.concatenate([rnd(m), P[-(K - 1):]])
    X[0] = other(Q[0])                                        # the two successors of P's last k-mer differ ...
    X[m - 1] = other(P[-K])                                   # ... and so do the two predecessors of the sink
    long_ref, long_alt = np.concatenate([P, Q]), np.concatenate([P, X, Q])
    longest = m + K - 1
    cut = lambda t, a: t[min(a, len(t) - L):][:L]
    err_read = substituted(cut(plain[0], 50), L // 2)         # an error in the middle: a bubble of count 1
    tip_read = substituted(cut(plain[1], 50), L - 6)          # an error 5 bases from the end: a tip
    counted = []
    constructs = {"plain": plain, "sub": [sub_ref, sub_alt], "tri": tri, "del": [del_ref, del_alt], "skip": [skip_ref, skip_alt], "two": [two_ref, two_alt],
                  "long": [long_ref, long_alt]}
    for seqs in constructs.values():
        for t in seqs:
            counted += tiled(t, L)                            # both strands
    counted += [err_read, tip_read]
    codes, offs = concat(counted)
    o = counted_oracle(codes, offs, K)
    nodes = oracle_nodes(o)
    model, model1 = Bubbles(nodes, K, **DEFAULTS), Bubbles(nodes, K, **dict(DEFAULTS, min_count=1))
    parts = {name: set.union(*[words_of(t, K) for t in seqs]) for name, seqs in constructs.items()}
    case = {"K": K, "L": L, "reads": (codes, offs), "nodes": nodes, "kmers_in_reads": o.kmers_in_reads(), "node_count": o.node_count(), "counted": counted,
            "parts": parts, "longest": longest, "model": model, "model1": model1}

    # ---- what the case is for, on the model
    canon_s = lambda f: min(f[0], rc_int(f[0], K))
    of = lambda mdl, name: [f for f in mdl.bubbles if canon_s(f) in parts[name]]
    lens = lambda f: (f[4][1], f[5][1])
    assert len(model.bubbles) == 8 and not of(model, "plain"), [lens(f) for f in model.bubbles]
    assert [lens(f) for f in of(model, "sub")] == [(K, K)]
    assert [lens(f) for f in of(model, "tri")] == [(K, K)] * 3 and len({(f[0], f[3]) for f in of(model, "tri")}) == 1
    (d,), (sk,), (tw,), (lg,) = of(model, "del"), of(model, "skip"), of(model, "two"), of(model, "long")
    assert abs(lens(d)[0] - lens(d)[1]) == 5 and abs(lens(sk)[0] - lens(sk)[1]) == 3 * K
    assert lens(tw) == (K + K // 2, K + K // 2)
    assert sorted(lens(lg)) == [0, longest] and 0 in (lg[4][2] + lg[4][3], lg[5][2] + lg[5][3])      # the len == 0 side: min 0, sum 0
    assert model.info[6] == longest and model.info[5] == sum(sum(lens(f)) + 2 for f in model.bubbles)
    assert model.info[1] == 2 * 6 and model.info[2] == 2 * (5 * 2 + 3) and model.info[3] == model.info[2]      # six sites, one of them three-way, seen from both ends
    # the read with an error in its middle is a ninth bubble at min_count 1, with a side of count 1, on the transcript it was cut from;
    # the error near the end of a read adds a fork whose branch ends, and no bubble
    extra = [f for f in model1.bubbles if f not in model.bubbles]
    assert len(model1.bubbles) == 9 and len(extra) == 1 and lens(extra[0]) == (K, K) and min(extra[0][4][2], extra[0][5][2]) == 1
    assert canon_s(extra[0]) in words_of(plain[0], K)
    assert model1.info[1] == model.info[1] + 3 and model1.info[2] - model1.info[3] == 2      # (the tip, and the transcript beside it: neither meets a sink)
    # max_len at the longest side and one below it
    assert len(Bubbles(nodes, K, **dict(DEFAULTS, max_len=longest)).bubbles) == 8 and len(Bubbles(nodes, K, **dict(DEFAULTS, max_len=longest - 1)).bubbles) == 7
    # every bubble is found from both of its ends, and reported once
    seen = {(f[0], f[3]) for f in model.found}
    assert len(model.found) == 2 * len(model.bubbles) and all((rc_int(f[3], K), rc_int(f[0], K)) in seen for f in model.bubbles)
    assert all(f[0] <= rc_int(f[3], K) for f in model.bubbles)
    return case


def reverse_complemented(case):
    """(codes, offs) of the case's reads, every one reverse-complemented"""
    return concat([revcomp(r) for r in case["counted"]])


def bubbles_of_reads(codes, offs, K, **params):
    return Bubbles(oracle_nodes(counted_oracle(codes, offs, K)), K, **dict(DEFAULTS, **params))


# ---- graphs written by hand --------------------------------------------------------------------------------------------------------------
def _shift(x, b, K):
    """(canonical key, bit position) of the out counter of the oriented word x towards base b"""
    r = rc_int(x, K)
    return (x, 24 + 6 * b) if x <= r else (r, 6 * (b ^ 2))


def set_link(nodes, x, b, value, K):
    """the out counter of the oriented word x towards base b, at this end of the link only"""
    c, sh = _shift(x, b, K)
    nodes[c][0] = nodes[c][0] & ~(63 << sh) | value << sh


def get_link(nodes, x, b, K):
    c, sh = _shift(x, b, K)
    return nodes[c][0] >> sh & 63


def hand_graph(seqs, K, count=5, link=5):
    """canonical k-mer -> [links, count, deleted]: every sequence adds `count` to its k-mers and `link` to both ends of every adjacency
    (saturating at 63), as counting it `count` times would"""
    nodes, top = {}, 2 * (K - 1)
    for seq in seqs:
        fw, cn = kmer_ints(seq, K)
        for c in cn:
            nodes.setdefault(c, [0, 0, 0])[1] += count
        for x, y in zip(fw, fw[1:]):
            for w, b in ((x, y & 3), (rc_int(y, K), (x >> top & 3) ^ 2)):
                set_link(nodes, w, b, min(63, get_link(nodes, w, b, K) + link), K)
    return nodes


def palindrome_graph(K=24):
    """two alleles behind a source that is its own reverse complement (even K) -> (nodes, the source)"""
    rng = np.random.default_rng(11)
    half = rng.integers(0, 4, size=K // 2, dtype=np.uint8)
    S = np.concatenate([half, revcomp(half)])
    pre, post = rng.integers(0, 4, size=40, dtype=np.uint8), rng.integers(0, 4, size=2 * K, dtype=np.uint8)
    pre[-1] = ((post[0] + 2) & 3) ^ 2                         # (what leads into S leaves it, reversed, by a third base)
    ref = np.concatenate([pre, S, post])
    return hand_graph([ref, substituted(ref, len(pre) + K)], K), kmer_ints(S, K)[0][0]


def node_arrays(nodes, nw):
    """(keys, l_links, r_flags, count) as sdt_gpu_import_nodes takes them"""
    ks = sorted(nodes)
    keys = np.array([key_words(k, nw) for k in ks], dtype=np.uint64).reshape(len(ks), nw)
    l = np.array([nodes[k][0] & 0xFFFFFF for k in ks], dtype=np.uint32)
    rf = np.array([nodes[k][0] >> 24 | nodes[k][2] << 25 for k in ks], dtype=np.uint32)
    return keys, l, rf, np.array([nodes[k][1] for k in ks], dtype=np.uint32)


def as_model_nodes(nodes):
    return {k: tuple(v) for k, v in nodes.items()}


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def kind_of(K, len_a, len_b):
    return 0 if len_a == len_b == K else 1 if len_a == len_b else 2


def bubbles_text(model):
    """out.bubbles: id source sink base_a base_b len_a len_b min_a min_b sum_a sum_b link_a link_b kind"""
    K = model.K
    return "".join(f"{i + 1} {kmer_text(s, K)} {kmer_text(t, K)} {LETTERS[ba]} {LETTERS[bb]} {a[1]} {b[1]} {a[2]} {b[2]} {a[3]} {b[3]} {a[0]} {b[0]} "
                   f"{kind_of(K, a[1], b[1])}\n" for i, (s, ba, bb, t, a, b) in enumerate(model.bubbles))


def fasta_text(model):
    """out.bubbles.fa: the two alleles of every bubble"""
    out = []
    for i, (_, _, _, _, a, b) in enumerate(model.bubbles):
        for tag, br, seq in zip("ab", (a, b), model.alleles(i)):
            out.append(f">{i + 1}_{tag} len={br[1]} min={br[2]} sum={br[3]}\n{seq}\n")
    return "".join(out)


def summary_line(model):
    kinds = [kind_of(model.K, f[4][1], f[5][1]) for f in model.bubbles]
    i = model.info
    return (f"bubbles: live {i[0]} forks {i[1]} branches {i[2]} reached {i[3]} bubbles {i[4]} kind0 {kinds.count(0)} kind1 {kinds.count(1)} "
            f"kind2 {kinds.count(2)} longest {i[6]}")
