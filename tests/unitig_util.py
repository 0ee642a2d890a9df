"""The rule of the unitig list (include/sdt_gpu.h: sdt_gpu_unitigs_*) restated in plain Python over bubble_util.Bubbles.succ / node_of --
what the GPU tests and the command-line test expect -- and the texts of the four outputs of `sdt-kmers unitigs`.  The nodes come from
the oracle or are written by hand, never from the library under test.  All comparisons against it are exact."""
import numpy as np

import bubble_util as bu
from read_cluster_util import LETTERS, concat, is_live, key_words, kmer_ints, kmer_text, rc_int

FIELDS = ("sum", "nodes", "min", "max", "info")
DTYPE = np.dtype([("sum", np.uint64)] + [(f, np.uint32) for f in FIELDS[1:]])
LINK_FIELDS = ("from", "to", "info", "reserved")
LINK_DTYPE = np.dtype([(f, np.uint32) for f in LINK_FIELDS])
DEFAULTS = dict(min_count=2, max_count=0, min_link=1)


class Unitigs:
    """unitigs: the reported ones in id order, each a dict (words: x0 .. x(n-1), counts, bases: the last base of x1 .., circular, indeg,
    outdeg); links: (from, to, o, o', b, link) in the order of the rule; dangling; info as sdt_gpu_unitigs_begin gives it"""

    def __init__(self, nodes, K, min_count=2, max_count=0, min_link=1):
        g = bu.Bubbles.__new__(bu.Bubbles)                    # (its succ and node_of only: no bubble is looked for)
        g.nodes, g.K, g.min_count, g.max_count, g.min_link = nodes, K, min_count, max_count, min_link
        g.mask, g.top = (1 << (2 * K)) - 1, 2 * (K - 1)
        g.live = {u for u, n in nodes.items() if is_live(n, min_count, max_count)}
        self.g, self.K, self.nodes = g, K, nodes
        rc = lambda x: rc_int(x, K)
        covered, found, starts = set(), [], 0
        for u in g.live:
            for x in sorted({u, rc(u)}):                      # (a palindrome is one oriented word)
                if self.join(rc(x)) is not None:              # x has a left join: not the first word of a chain
                    continue
                starts += 1
                words, bases = self.chain(x)
                if x <= rc(words[-1]):
                    found.append(self.unitig(words, bases, 0))
                    canon = [min(w, rc(w)) for w in words]
                    assert not covered & set(canon) and len(set(canon)) == len(canon)
                    covered |= set(canon)
        for u in sorted(g.live):                              # what is left lies on cycles: each from its smallest word
            if u in covered:
                continue
            words, bases = self.chain(u, cycle=True)
            canon = [min(w, rc(w)) for w in words]
            assert min(canon) == u and not covered & set(canon) and len(set(canon)) == len(canon)
            covered |= set(canon)
            found.append(self.unitig(words, bases, 1))
        assert covered == g.live
        self.unitigs = sorted(found, key=lambda t: t["words"][0])
        plus = {t["words"][0]: i for i, t in enumerate(self.unitigs)}
        minus = {rc(t["words"][-1]): i for i, t in enumerate(self.unitigs)}
        self.links, self.dangling_of = [], []
        for i, t in enumerate(self.unitigs):
            dangling = 0
            for o, w in ((0, t["words"][-1]), (1, rc(t["words"][0]))):
                for b, y, _, link in g.succ(w, rc(w)):
                    if y in plus:
                        self.links.append((i, plus[y], o, 0, b, link))
                    elif y in minus:
                        self.links.append((i, minus[y], o, 1, b, link))
                    else:
                        dangling += 1
                if w == rc(w):
                    break                                     # (one oriented word, one side)
            self.dangling_of.append(dangling)
        self.dangling = sum(self.dangling_of)
        n = [len(t["words"]) for t in self.unitigs]
        self.info = [len(g.live), starts, len(n), sum(t["circular"] for t in self.unitigs), sum(n), sum(n) + (K - 1) * len(n), max(n, default=0), 0]

    def join(self, x):
        """(b, y, link) when JOIN(x, y) holds for some y, else None"""
        K, g = self.K, self.g
        rx = rc_int(x, K)
        sc = g.succ(x, rx)
        if len(sc) != 1:
            return None
        b, y, ry, link = sc[0]
        back = g.succ(ry, y)
        if len(back) != 1 or back[0][1] != rx or min(x, rx) == min(y, ry) or x == rx or y == ry:
            return None
        return b, y, link

    def chain(self, x, cycle=False):
        """the words from x on along the right joins, and the bases appended; a cycle stops when it is back at x"""
        words, bases = [x], []
        while True:
            j = self.join(words[-1])
            if j is None:
                assert not cycle, "a node that no chain covers lies on no cycle"
                return words, bases
            if cycle and j[1] == x:
                return words, bases
            words.append(j[1])
            bases.append(j[0])

    def unitig(self, words, bases, circular):
        K, g = self.K, self.g
        counts = [g.node_of(w, rc_int(w, K))[1] for w in words]
        return dict(words=words, bases=bases, counts=counts, circular=circular, indeg=len(g.succ(rc_int(words[0], K), words[0])),
                    outdeg=len(g.succ(words[-1], rc_int(words[-1], K))))

    # ---- what the calls give
    def records(self):
        rec = np.zeros(len(self.unitigs), dtype=DTYPE)
        for i, t in enumerate(self.unitigs):
            c = t["counts"]
            rec[i] = (sum(c), len(c), min(c), max(c), t["circular"] | t["indeg"] << 4 | t["outdeg"] << 8)
        return rec

    def keys(self, nw):
        return np.array([[key_words(t["words"][0], nw), key_words(t["words"][-1], nw)] for t in self.unitigs], dtype=np.uint64).reshape(len(self.unitigs), 2, nw)

    def codes(self, i):
        """the base codes of unitig i: the K bases of x0, then one per further word"""
        t, K = self.unitigs[i], self.K
        x0 = t["words"][0]
        return [x0 >> 2 * (K - 1 - j) & 3 for j in range(K)] + t["bases"]

    def seqs(self, first=0, n=None):
        """(bases uint8, offsets uint64[n + 1]) of unitigs first .. first + n - 1"""
        last = len(self.unitigs) if n is None else first + n
        return concat([self.codes(i) for i in range(first, last)])

    def text(self, i, o=0):
        """the sequence of unitig i in letters; o = 1: its reverse complement"""
        c = self.codes(i)
        return "".join(LETTERS[b] for b in (c if o == 0 else [b ^ 2 for b in reversed(c)]))

    def link_records(self, first=0, n=None):
        last = len(self.unitigs) if n is None else first + n
        part = [l for l in self.links if first <= l[0] < last]
        rec = np.zeros(len(part), dtype=LINK_DTYPE)
        for j, (u, v, o, o2, b, link) in enumerate(part):
            rec[j] = (u, v, o | o2 << 1 | b << 2 | link << 8, 0)
        return rec, sum(self.dangling_of[first:last])

    def gfa_links(self):
        """the links that the GFA writes: the directed record that is <= its mirror"""
        return [(u, o, v, o2, link) for u, v, o, o2, _, link in self.links if (u, o, v, o2) <= (v, 1 - o2, u, 1 - o)]


def assert_overlaps(model):
    """every link's two sequences overlap in K - 1 bases in the stated orientations"""
    for u, v, o, o2, b, _ in model.links:
        a, c = model.text(u, o), model.text(v, o2)
        assert a[-(model.K - 1):] == c[:model.K - 1] and c[model.K - 1] == LETTERS[b], (u, v, o, o2)


def assert_unitigs_equal(g, model, info, what=""):
    """info, records, words, sequences and links of the whole list"""
    assert [int(x) for x in info] == model.info, (what, [int(x) for x in info], model.info)
    n = len(model.unitigs)
    keys, rec = g.unitigs_fetch(0, n)
    want = model.records()
    assert rec.dtype == DTYPE, rec.dtype
    for f in FIELDS:
        assert rec[f].tolist() == want[f].tolist(), f"{what}: field {f}: got {rec[f].tolist()[:8]} want {want[f].tolist()[:8]}"
    assert keys.tolist() == model.keys(g.nw).tolist(), f"{what}: the first and last words differ"
    bases, offs = g.unitigs_seqs(0, n)
    wb, wo = model.seqs()
    assert offs.tolist() == wo.tolist(), f"{what}: sequence offsets"
    assert bases.tobytes() == wb.tobytes(), f"{what}: sequence bytes"
    links, dangling = g.unitigs_links(0, n)
    wl, wd = model.link_records()
    assert links.dtype == LINK_DTYPE, links.dtype
    assert links.tolist() == wl.tolist(), f"{what}: links: got {links.tolist()[:6]} want {wl.tolist()[:6]}"
    assert dangling == wd, (what, dangling, wd)


def canonical_kmers(model):
    """the canonical k-mers of all sequences, a sorted list"""
    out = []
    for i in range(len(model.unitigs)):
        out += kmer_ints(np.array(model.codes(i), dtype=np.uint8), model.K)[1]
    return sorted(out)


# ---- graphs written by hand --------------------------------------------------------------------------------------------------------------
def cycle_graph(K, n, seed, **kw):
    """a pure cycle of n nodes: n random bases read round and round.  Built from c + c[:K] (n + K bases): with K - 1 the k-mer that
    closes the cycle would be there and its link would not"""
    c = np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)
    return bu.hand_graph([np.concatenate([c, c[:K]])], K, **kw)


def merged(*graphs):
    out = {}
    for g in graphs:
        for k, v in g.items():
            assert k not in out, "the graphs share a k-mer"
            out[k] = list(v)
    return out


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def unitigs_text(model):
    """out.unitigs: id first last nodes bases sum mean_x100 min max in out circular"""
    K, out = model.K, []
    for i, t in enumerate(model.unitigs):
        c = t["counts"]
        out.append(f"{i + 1} {kmer_text(t['words'][0], K)} {kmer_text(t['words'][-1], K)} {len(c)} {len(c) + K - 1} {sum(c)} {sum(c) * 100 // len(c)} "
                   f"{min(c)} {max(c)} {t['indeg']} {t['outdeg']} {t['circular']}\n")
    return "".join(out)


def fasta_text(model):
    return "".join(f">{i + 1} nodes={len(t['counts'])} sum={sum(t['counts'])} min={min(t['counts'])} max={max(t['counts'])} circular={t['circular']}\n"
                   f"{model.text(i)}\n" for i, t in enumerate(model.unitigs))


def gfa_text(model):
    out = ["H\tVN:Z:1.0\n"]
    for i, t in enumerate(model.unitigs):
        out.append(f"S\t{i + 1}\t{model.text(i)}\tLN:i:{len(t['counts']) + model.K - 1}\tKC:i:{sum(t['counts'])}\n")
    for u, o, v, o2, link in model.gfa_links():
        out.append(f"L\t{u + 1}\t{'+-'[o]}\t{v + 1}\t{'+-'[o2]}\t{model.K - 1}M\tlc:i:{link}\n")
    return "".join(out)


def n50(lengths):
    total, acc = sum(lengths), 0
    for x in sorted(lengths, reverse=True):
        acc += x
        if 2 * acc >= total:
            return x
    return 0


def summary_line(model):
    i, ts = model.info, model.unitigs
    isolated = sum(t["indeg"] == 0 and t["outdeg"] == 0 for t in ts)
    dead = sum((t["indeg"] == 0) != (t["outdeg"] == 0) for t in ts)
    return (f"unitigs: live {i[0]} unitigs {i[2]} circular {i[3]} isolated {isolated} dead_ends {dead} links {len(model.gfa_links())} bases {i[5]} "
            f"longest {i[6]} n50 {n50([len(t['counts']) + model.K - 1 for t in ts])}")
