"""The rule of the read clustering (include/sdt_gpu.h: sdt_gpu_cluster_*) restated in plain Python -- what the GPU tests and the
command-line test expect -- and the cases they run.  The nodes come from the oracle's export() (keys, l_links, r_links, counts,
flags), never from the library under test; liveness, edges, a dictionary union-find, the ranking by smallest key and the read
records are plain loops.  All comparisons against it are exact."""
import functools

import numpy as np

LETTERS = "ACTG"                                      # the stream's codes: A 0, C 1, T 2, G 3; complement = code ^ 2
NONE = 0xFFFFFFFF
FIELDS = ("kmers", "live", "split", "cluster", "unit", "verdict")
DTYPE = np.dtype([(f, np.uint32) for f in FIELDS])
WHOLE, NOT_WHOLE, THROUGH_MATE, UNASSIGNED, SHORT = range(5)

_REV4 = bytes(((b & 3) << 6) | ((b >> 2 & 3) << 4) | ((b >> 4 & 3) << 2) | (b >> 6) for b in range(256))


def codes_of(text):
    return np.array([LETTERS.index(c) for c in text.upper()], dtype=np.uint8)


def text_of(codes):
    return "".join(LETTERS[int(c)] for c in codes)


def revcomp(codes):
    return (np.asarray(codes, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def rc_int(x, K):
    """the reverse complement of a k-mer held as an integer, first base most significant"""
    nb = (2 * K + 7) // 8
    comp = x ^ (((1 << (2 * K)) - 1) // 3 * 2)            # every base ^ 2
    return int.from_bytes(comp.to_bytes(nb, "little").translate(_REV4), "big") >> (8 * nb - 2 * K)


def canon(x, K):
    r = rc_int(x, K)
    return x if x < r else r


def kmer_ints(codes, K):
    """(forward k-mers, canonical k-mers) of a sequence as integers"""
    mask, top = (1 << (2 * K)) - 1, 2 * (K - 1)
    fw = rc = 0
    f, c = [], []
    for i, b in enumerate(np.asarray(codes).tolist()):
        fw = ((fw << 2) | b) & mask
        rc = (rc >> 2) | ((b ^ 2) << top)
        if i >= K - 1:
            f.append(fw)
            c.append(fw if fw < rc else rc)
    return f, c


def canon_kmers(codes, K):
    return kmer_ints(codes, K)[1]


def concat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    codes = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if seqs else np.zeros(0, dtype=np.uint8)
    return codes.astype(np.uint8), offs


def key_words(x, nw):
    return [(x >> (64 * (nw - 1 - i))) & 0xFFFFFFFFFFFFFFFF for i in range(nw)]


def keys_array(ints, nw):
    return np.array([key_words(x, nw) for x in ints], dtype=np.uint64).reshape(len(ints), nw)


def key_int(row):
    v = 0
    for x in row:
        v = (v << 64) | int(x)
    return v


def oracle_nodes(o):
    """canonical k-mer -> (links = l_links | r_links << 24, count, deleted) from an oracle's table as it stands"""
    keys, l, r, cnt, fl = o.export()
    return {key_int(row): (int(a) | int(b) << 24, int(c), int(f) >> 1 & 1) for row, a, b, c, f in zip(keys.tolist(), l.tolist(), r.tolist(), cnt.tolist(), fl.tolist())}


def counted_oracle(codes, offs, K):
    import oracle_binding as ob
    o = ob.Oracle(K, nsets=5)
    o.add_reads(codes, offs)
    return o


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def is_live(node, min_count, max_count):
    _, count, deleted = node
    return not deleted and count >= max(min_count, 1) and (max_count == 0 or count <= max_count)


def neighbour(u, side, b, K):
    """the canonical k-mer of u's neighbour by base b on the left (side 0) or on the right (side 1)"""
    word = (u >> 2) | (b << (2 * (K - 1))) if side == 0 else ((u << 2) | b) & ((1 << (2 * K)) - 1)
    return canon(word, K)


def edges_of(nodes, K, min_count, max_count, min_link):
    """[(u, v)] for every qualifying link end (u, side, b) that finds a live neighbour, u = v included"""
    out = []
    for u, node in nodes.items():
        if not is_live(node, min_count, max_count):
            continue
        for side in range(2):
            for b in range(4):
                if (node[0] >> (24 * side + 6 * b)) & 63 >= min_link:
                    v = neighbour(u, side, b, K)
                    if v in nodes and is_live(nodes[v], min_count, max_count):
                        out.append((u, v))
    return out


class Clustering:
    """label: canonical k-mer -> id; comps: [(smallest k-mer, nodes, count_sum)] in id order; info as sdt_gpu_cluster_begin gives it"""

    def __init__(self, nodes, K, min_count=2, max_count=0, min_link=1):
        live = [u for u, n in nodes.items() if is_live(n, min_count, max_count)]
        parent = {u: u for u in live}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        ends = edges_of(nodes, K, min_count, max_count, min_link)
        for u, v in ends:
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
        members = {}
        for u in live:
            members.setdefault(find(u), []).append(u)
        roots = sorted(min(m) for m in members.values())
        assert roots == sorted(members)                   # (the smaller root wins every union: a root is its cluster's smallest k-mer)
        self.K = K
        self.label = {}
        self.comps = []
        for i, r in enumerate(roots):
            for u in members[r]:
                self.label[u] = i
            self.comps.append((r, len(members[r]), sum(nodes[u][1] for u in members[r])))
        sizes = [c[1] for c in self.comps]
        big = max(sizes) if sizes else 0
        self.info = [len(live), len(ends), len(roots), big, sizes.index(big) if sizes else 0, len(nodes) - len(live), 0, 0]

    def of_kmer(self, x):
        return self.label.get(canon(x, self.K), NONE)

    def walk(self, codes):
        """(kmers, live, split, cluster) of one read"""
        labs = [self.label.get(k, NONE) for k in canon_kmers(codes, self.K)]
        alive = [x for x in labs if x != NONE]
        first = alive[0] if alive else NONE
        return len(labs), len(alive), sum(x != first for x in alive), first

    def records(self, reads, paired=False, pick=(0, NONE - 1), units=None):
        """-> (DTYPE[len(reads)], keep uint8, reads kept).  units: lists of read indices (default: every read, or reads 2t and 2t + 1);
        a read in no unit keeps a record of 0xFF bytes and keep 0"""
        n = len(reads)
        if units is None:
            assert not paired or n % 2 == 0
            units = [[2 * t, 2 * t + 1] for t in range(n // 2)] if paired else [[i] for i in range(n)]
        rec = np.full(n, NONE, dtype=np.uint32).repeat(6).view(DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        for unit in units:
            w = [self.walk(reads[i]) for i in unit]
            own = [x[3] for x in w]
            u = next((c for c in own if c != NONE), NONE)
            for i, (kmers, live, split, cluster) in zip(unit, w):
                if all(x[0] == 0 for x in w):
                    v = SHORT
                elif all(x[1] == 0 for x in w):
                    v = UNASSIGNED
                elif live == 0:
                    v = THROUGH_MATE
                elif split > 0 or cluster != u:
                    v = NOT_WHOLE
                else:
                    v = WHOLE
                rec[i] = (kmers, live, split, cluster, u, v)
                keep[i] = u != NONE and pick[0] <= u <= pick[1]
        return rec, keep, int(keep.sum())


def assert_records_equal(got, want, what=""):
    assert got.dtype == DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at reads {bad[:8].tolist()}: got {got[f][bad[:8]].tolist()} want {want[f][bad[:8]].tolist()}"


def assert_clustering_equal(pkg, g, model, info, what=""):
    """info, the component list with its keys in strictly ascending order"""
    assert [int(x) for x in info] == model.info, (what, [int(x) for x in info], model.info)
    keys, comp = g.cluster_components()
    got = [key_int(r) for r in keys.tolist()]
    assert got == [c[0] for c in model.comps], f"{what}: the clusters' smallest k-mers differ"
    assert all(a < b for a, b in zip(got, got[1:])), f"{what}: keys not strictly ascending"
    assert comp["nodes"].tolist() == [c[1] for c in model.comps] and comp["count_sum"].tolist() == [c[2] for c in model.comps], what
    assert (comp["reserved"] == 0).all()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def read_len_for(K):
    """reads are 100 bases where such a read can hold a whole k-mer on either side of a junction (2 K + 10 <= 100), and 2 K + 10 bases
    beyond: the bridge and the junction of the case need one read across them"""
    return max(100, 2 * K + 10)


def tiled(seq, L, step=10):
    """reads of L bases over seq every `step` bases and at its end, on both strands"""
    assert len(seq) >= L
    starts = sorted(set(list(range(0, len(seq) - L + 1, step)) + [len(seq) - L]))
    out = []
    for s in starts:
        out.append(np.asarray(seq[s:s + L], dtype=np.uint8))
        out.append(revcomp(seq[s:s + L]))
    return out


def substituted(seq, at):
    s = np.array(seq, dtype=np.uint8)
    s[at] = (s[at] + 1) & 3
    return s


PARAM_SETS = {                                            # what the case is built around
    "base": dict(min_count=2, max_count=70000, min_link=1),
    "bridge": dict(min_count=1, max_count=0, min_link=1),
    "hub_cut": dict(min_count=2, max_count=60000, min_link=1),
    "link_cut": dict(min_count=2, max_count=0, min_link=2),
}


@functools.lru_cache(maxsize=None)
def built_case(K, seed=0):
    """-> dict: K, L, reads (codes, offs) to count, nodes (from the oracle), kmers_in_reads, node_count, query (reads to cluster, an even
    number: reads 2t and 2t + 1 are the pairs), at (name -> index in query), models (name of PARAM_SETS -> Clustering).  Every property
    the issue names is asserted on the model here, so a case that lost one fails without a GPU."""
    rng = np.random.default_rng(1000 * K + seed)
    L = read_len_for(K)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    tr = lambda: rnd(int(rng.integers(300, 601)))
    plain = [tr() for _ in range(12)]                     # >= 12 disjoint transcripts
    # two transcripts that share a stretch of 2K bases
    stretch = rnd(2 * K)
    sh_a, sh_b = np.concatenate([rnd(150), stretch, rnd(150)]), np.concatenate([rnd(200), stretch, rnd(120)])
    # two transcripts joined only by one chimeric read: its K - 1 junction k-mers are seen once
    br_a, br_b = tr(), tr()
    bridge_read = np.concatenate([br_a[-(L // 2):], br_b[:L - L // 2]])
    # three transcripts that end in the same poly-A hub; the base in front of the tail differs, so that nothing but the hub joins them
    hubs = [np.concatenate([tr(), np.array([c], dtype=np.uint8), np.zeros(K + 5, dtype=np.uint8)]) for c in (1, 2, 3)]
    hub_reads = [np.zeros(K + 249, dtype=np.uint8)] * 264   # 264 x 250 = 66 000 occurrences of the node A^K
    # one sequence counted as two halves that overlap by K - 1 bases, so that no counted read holds the adjacency at base m, and one read
    # across it: every k-mer there is seen at least twice, the link counter of the junction once
    jn = rnd(2 * L + 160)
    m = L + 80
    s0 = m - K - (L - K - 1) // 2
    jn_read = jn[s0:s0 + L]                               # holds the K + 1 bases jn[m - K .. m]
    # a read with one substitution in the middle: K weak k-mers between two live stretches of one cluster
    cut = lambda t, a: t[min(a, len(t) - L):][:L]
    err_read = substituted(cut(plain[0], 50), L // 2)
    counted = []
    for t in plain + [sh_a, sh_b, br_a, br_b] + hubs:
        counted += tiled(t, L)
    counted += tiled(jn[:m], L) + tiled(jn[m - K + 1:], L)
    counted += [bridge_read, jn_read, err_read] + hub_reads
    codes, offs = concat(counted)
    o = counted_oracle(codes, offs, K)
    nodes = oracle_nodes(o)
    models = {name: Clustering(nodes, K, **p) for name, p in PARAM_SETS.items()}

    # ---- the reads that are clustered
    query, at = [], {}

    def add(name, a, b):
        at[name] = len(query)
        query.extend([np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)])

    random_read = rnd(L)
    add("whole_pair", plain[1][:L], revcomp(cut(plain[1], 120)))
    add("mates_apart", plain[2][:L], plain[3][:L])                        # mates in different clusters
    add("mate_unassigned", cut(plain[4], 10), random_read)              # a mate without a live k-mer
    add("unassigned_first", random_read, cut(plain[4], 10))
    add("short_pair", plain[5][:K - 1], plain[5][:3])                     # shorter than K, both
    add("short_mate", plain[5][:K - 1], cut(plain[5], 20))
    add("short_and_random", np.zeros(0, dtype=np.uint8), random_read)
    add("bridge", bridge_read, br_a[:L])
    add("junction", jn_read, jn[:L])
    add("weak_middle", err_read, cut(plain[0], 50))
    add("hub", hubs[0][-L:], hubs[1][-L:])
    add("shared", sh_a[:L], sh_b[:L])
    add("polyA", np.zeros(L, dtype=np.uint8), hubs[2][:L])
    for i in range(0, len(counted) - 280, 14):                            # and a sample of the counted reads, consecutive ones as mates
        query.extend([counted[i], counted[i + 1]])
    assert len(query) % 2 == 0

    # ---- what the case is for, on the model
    base, bridge, hub_cut, link_cut = (models[n] for n in ("base", "bridge", "hub_cut", "link_cut"))
    cl = lambda mdl, seq: {mdl.label.get(k, NONE) for k in canon_kmers(seq, K)} - {NONE}
    assert len({next(iter(cl(base, t))) for t in plain}) == 12 and all(len(cl(base, t)) == 1 for t in plain)
    assert cl(base, sh_a) == cl(base, sh_b) and len(cl(base, sh_a)) == 1
    assert len(cl(bridge, br_a) | cl(bridge, br_b)) == 1 and cl(base, br_a).isdisjoint(cl(base, br_b))
    assert bridge.info[2] < base.info[2]
    hub_count = nodes[0][1]                               # the node A^K
    assert 65535 < hub_count <= 70000 and (hub_count & 0xFFFF) < 60000      # (the high half decides)
    assert len(set.union(*[cl(base, h) for h in hubs])) == 1 and len(set.union(*[cl(hub_cut, h) for h in hubs])) == 3
    assert hub_cut.of_kmer(0) == NONE and hub_cut.info[2] == base.info[2] + 2
    assert len(cl(base, jn)) == 1 and len(cl(link_cut, jn)) == 2 and link_cut.info[2] == base.info[2] + 1
    jf, jc = kmer_ints(jn[m - K:m + 1], K)                # the two k-mers at the junction and the counter between them
    side = 1 if jf[0] == jc[0] else 0
    b = int(jn[m]) if side else int(jn[m]) ^ 2
    assert (nodes[jc[0]][0] >> (24 * side + 6 * b)) & 63 == 1 and nodes[jc[0]][1] >= 2 and nodes[jc[1]][1] >= 2
    assert len({mdl.info[2] for mdl in models.values()}) == 4
    rec = base.records(query, paired=True)[0]
    single = base.records(query)[0]
    assert set(rec["verdict"].tolist()) == {WHOLE, NOT_WHOLE, THROUGH_MATE, UNASSIGNED, SHORT}
    assert rec["verdict"][at["mates_apart"] + 1] == NOT_WHOLE and rec["split"][at["mates_apart"] + 1] == 0
    assert rec["verdict"][at["mate_unassigned"] + 1] == THROUGH_MATE and rec["unit"][at["unassigned_first"]] == rec["cluster"][at["unassigned_first"] + 1]
    assert rec["verdict"][at["short_pair"]] == SHORT and rec["verdict"][at["short_and_random"]] == UNASSIGNED and rec["kmers"][at["short_and_random"]] == 0
    w = rec[at["weak_middle"]]
    assert w["split"] == 0 and w["live"] == w["kmers"] - K and w["verdict"] == WHOLE
    assert link_cut.records(query)[0]["split"][at["junction"]] > 0 and single["split"][at["junction"]] == 0
    assert base.records(query)[0]["split"][at["bridge"]] > 0 and bridge.records(query)[0]["split"][at["bridge"]] == 0
    assert hub_cut.records(query)[0]["live"][at["polyA"]] == 0 and single["live"][at["polyA"]] == L - K + 1
    assert (single["verdict"] != THROUGH_MATE).all()
    return {"K": K, "L": L, "reads": (codes, offs), "nodes": nodes, "kmers_in_reads": o.kmers_in_reads(), "node_count": o.node_count(),
            "query": query, "at": at, "models": models, "oracle": o}


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def kmer_text(x, K):
    return "".join(LETTERS[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def read_cluster_text(rec):
    ident = lambda c: 0 if c == NONE else c + 1           # ids are 1-based in the files, 0 = none
    return "".join(f"{r['kmers']} {r['live']} {r['split']} {ident(int(r['cluster']))} {ident(int(r['unit']))} {r['verdict']}\n" for r in rec)


def clusters_text(model, rec, lengths):
    """out.clusters: id kmer nodes count_sum reads bases, then the closing line"""
    reads, bases = [0] * len(model.comps), [0] * len(model.comps)
    for r, n in zip(rec, lengths):
        if r["unit"] != NONE:
            reads[int(r["unit"])] += 1
            bases[int(r["unit"])] += int(n)
    lines = [f"{i + 1} {kmer_text(k, model.K)} {nodes} {total} {reads[i]} {bases[i]}\n" for i, (k, nodes, total) in enumerate(model.comps)]
    unassigned = int((rec["unit"] == NONE).sum())
    lines.append(f"# live {model.info[0]} link_ends {model.info[1]} clusters {model.info[2]} largest {model.info[3]} unassigned {unassigned}\n")
    return "".join(lines)


def summary_line(model, rec):
    v = rec["verdict"]
    assigned = int((rec["unit"] != NONE).sum())
    per = np.bincount(rec["unit"][rec["unit"] != NONE].astype(np.int64), minlength=max(len(model.comps), 1))
    return (f"cluster: reads {len(rec)} assigned {assigned} whole {int((v == WHOLE).sum())} through_mate {int((v == THROUGH_MATE).sum())} "
            f"unassigned {int((v == UNASSIGNED).sum())} short {int((v == SHORT).sum())} clusters {model.info[2]} largest_nodes {model.info[3]} "
            f"largest_reads {int(per.max()) if len(model.comps) else 0}")


def fasta_texts(reads, rec, alive, ranges):
    """(prefix.cluster.pairs.fa, prefix.cluster.single.fa): the reads with alive[i], those of a pair range into the pairs file, named by
    their read number and their unit's id"""
    out = ["", ""]
    parts = [[], []]
    for i, r in enumerate(reads):
        if alive[i]:
            unit = 0 if rec["unit"][i] == NONE else int(rec["unit"][i]) + 1
            parts[0 if any(a <= i < b for a, b in ranges) else 1].append(f">{i + 1} cluster={unit}\n{text_of(r)}\n")
    out[0], out[1] = "".join(parts[0]), "".join(parts[1])
    return out
