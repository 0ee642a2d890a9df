"""Inputs and expectations of the second-read-pass tests (test_read2edge_oracle.py on the CPU, test_read2edge.py on the GPU).

The second read pass (prlRead2edge, prlRead2path.c:817-1335) reads three things of the cleaned graph: per node deleted / linear /
inEdge / edge id / twin, the patch table of (K+1)-mers, and num_ed.  None of them has to come from a real graph: `Scenario` counts
seeded reads in the oracle, gives EVERY node a random class and label, fills the patch table with a random part of the (K+1)-mers the
reads will ask for, and runs the oracle's sdto_read2edge on that -- the expectation.  `walk_reads` is parse1read's pairing written
once more in plain Python: it finds the (K+1)-mers to offer the patch table, says which branches of the state machine the inputs
reach (the preconditions of the tests), and gives the ordinal of every arc's first appearance, which *.preArc only shows as an order.
Nothing here looks at the library under test."""
import os

import numpy as np

import oracle_binding as ob

M64 = (1 << 64) - 1
DELETED, FLOATING, IN_EDGE, VERTEX = 0, 1, 2, 3          # node classes; FLOATING = linear and not inEdge (skipped like DELETED)


def words4_of(v):
    """integer -> 4 words, most significant first"""
    return [(v >> 192) & M64, (v >> 128) & M64, (v >> 64) & M64, v & M64]


def keys4_to_int(keys4):
    k = np.asarray(keys4, dtype=np.uint64).reshape(-1, 4).tolist()
    return [(a << 192) | (b << 128) | (c << 64) | d for a, b, c, d in k]


def make_reads(synth, K, L, seed, n_reads=2500, T=10, err=0.003):
    """ragged reads with errors off a small transcriptome; by hand: reads of K - 1, K, K + 1, K + 2 bases and a copy of a read that
    is long enough to hold a path -> (codes, offs)"""
    tx = synth.make_transcriptome(T, seed=seed)
    codes, offs = synth.sample_reads(*tx, n_reads=n_reads, read_len=L, seed=seed + 100, err=err, ragged=True)
    o = offs.astype(np.int64)
    lens = o[1:] - o[:-1]
    long_ones = np.flatnonzero(lens >= min(K + 30, L))
    assert long_ones.size, "no read can hold a path"
    extra = [tx[0][40 * j + 7: 40 * j + 7 + n].astype(np.uint8) for j, n in enumerate((K - 1, K, K + 1, K + 2))]
    r = int(long_ones[len(long_ones) // 2])
    extra.append(codes[o[r]:o[r + 1]].copy())
    codes = np.concatenate([codes] + extra)
    offs = np.concatenate([offs, offs[-1] + np.cumsum([len(e) for e in extra]).astype(np.uint64)])
    return codes, offs


def take_reads(codes, offs, idx):
    """the reads idx of (codes, offs) as a stream of their own"""
    o = offs.astype(np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    lens = o[idx + 1] - o[idx]
    out_offs = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum(lens, out=out_offs[1:])
    parts = [codes[o[i]:o[i + 1]] for i in idx.tolist()]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), out_offs


def random_states(rng, n_nodes, E, shares=(0.05, 0.05, 0.60, 0.30), zero=0.01, id_lo=1):
    """every node a class (DELETED, FLOATING, IN_EDGE, VERTEX by `shares`) and a label: an edge id in [id_lo, E] and a twin in
    {0, 1, 2} with id + twin - 1 <= E (id + twin - 1 == 0 happens, and is wanted: an item that ends the arcs of its read).  Only an
    IN_EDGE node's label is ever read by the pass; the others carry one all the same, so that reading it shows.
    -> (cls uint8[n], edge_id uint32[n], twin uint8[n])"""
    cls = rng.choice(4, size=n_nodes, p=shares).astype(np.uint8)
    twin = rng.integers(0, 3, size=n_nodes).astype(np.uint8)
    edge_id = rng.integers(id_lo, E + 1, size=n_nodes).astype(np.int64)
    edge_id = np.where(edge_id + twin - 1 > E, E + 1 - twin.astype(np.int64), edge_id)
    zero = rng.random(n_nodes) < zero                    # id + twin - 1 == 0 at any E
    edge_id, twin = np.where(zero, 1, edge_id), np.where(zero, 0, twin).astype(np.uint8)
    assert (edge_id >= 1).all() and (edge_id + twin - 1 <= E).all()
    return cls, edge_id.astype(np.uint32), twin


def path_words(cls, edge_id, twin):
    """include/sdt_gpu.h, "pass 2": skip | linear << 1 | twin << 2 | id << 32.  A deleted node keeps whatever linear bit, twin and id
    it had: skip decides"""
    skip = (cls == DELETED) | (cls == FLOATING)
    linear = (cls == FLOATING) | (cls == IN_EDGE) | ((cls == DELETED) & (edge_id % 2 == 1))
    return (skip.astype(np.uint64) | (linear.astype(np.uint64) << np.uint64(1)) | (twin.astype(np.uint64) << np.uint64(2))
            | (edge_id.astype(np.uint64) << np.uint64(32)))


def walk_reads(codes, offs, K, node_of, cls, edge_id, twin, ordinals=None):
    """parse1read (prlRead2path.c:617-789) over every read with the node classes: -> (paths, stats).  paths: (ordinal, items) of the
    reads that end with two or more items; an item is an int (the edge a linear node stands for on the read's strand) or a pair
    (previous vertex k-mer as read, base): the (K+1)-mer search1kmerPlus will look up -- previous vertex + last base of the next
    vertex, whatever was skipped in between (is_prev survives a reset, :650-657).  stats counts the branches taken."""
    o = offs.astype(np.int64).tolist()
    cl, ids, tw = cls.tolist(), edge_id.tolist(), twin.tolist()
    mask, top = (1 << (2 * K)) - 1, 2 * (K - 1)
    paths = []
    st = dict(reads=0, resets=0, reset_then_vertex=0, zero_linear_items=0, breaks=0, same_item_dropped=0, len_k_plus_1=0)
    allc = codes.tolist()
    for r in range(len(o) - 1):
        seq = allc[o[r]:o[r + 1]]
        if len(seq) < K + 1:
            continue
        st["reads"] += 1
        st["len_k_plus_1"] += len(seq) == K + 1
        fw = rc = 0
        retain = 0
        have_prev = after_reset = False
        prev = 0
        items = []
        for p, b in enumerate(seq):
            fw = ((fw << 2) | b) & mask
            rc = (rc >> 2) | ((b ^ 2) << top)
            if p < K - 1:
                continue
            smaller = fw < rc
            i = node_of[fw if smaller else rc]
            c = cl[i]
            if c == DELETED or c == FLOATING:
                if retain < 2:
                    retain = 0
                    items = []
                    st["resets"] += 1
                    after_reset = have_prev
                    continue
                st["breaks"] += 1
                break
            if c == IN_EDGE:
                item = ids[i] if smaller else ids[i] + tw[i] - 1
                if retain == 0 or have_prev:
                    have_prev = False
                elif item == items[-1]:
                    st["same_item_dropped"] += 1
                    after_reset = False
                    continue
                st["zero_linear_items"] += item == 0
                items.append(item)
                retain += 1
            else:
                if have_prev:
                    st["reset_then_vertex"] += after_reset
                    items.append((prev, b))
                    retain += 1
                have_prev = True
                prev = fw
            after_reset = False
        if retain >= 2:
            paths.append((r if ordinals is None else int(ordinals[r]), items))
    return paths, st


def arcs_of_paths(paths, resolve):
    """the arc counting (:190-241, 415-430) over walked paths; resolve((prev, b)) -> item of a (K+1)-mer, 0 when the patch table does
    not have it.  -> ([(from, to, mult)], [first]) in *.preArc's order (from ascending, first appearance descending), and the number
    of paths of two or more items in which a (K+1)-mer missed"""
    arcs, misses = {}, 0
    for ordinal, items in paths:
        it = [x if isinstance(x, int) else resolve(x) for x in items]
        misses += any(v == 0 and not isinstance(x, int) for v, x in zip(it, items))
        for j in range(len(it) - 1):
            if it[j] == 0 or it[j + 1] == 0:
                break
            key = (it[j], it[j + 1])
            f = (ordinal << 16) | j
            a = arcs.get(key)
            if a is None:
                arcs[key] = [1, f]
            else:
                a[0] += 1
                a[1] = min(a[1], f)
    order = sorted(arcs, key=lambda k: (k[0], -arcs[k][1]))
    return [(k[0], k[1], arcs[k][0]) for k in order], [arcs[k][1] for k in order], misses


class Scenario:
    """reads + random node states + a random patch table, the oracle's *.preArc for them, and what the Python walk says about them"""

    def __init__(self, synth, tmp_dir, K, L, E, seed, n_reads=2500, T=10, shares=(0.05, 0.05, 0.60, 0.30), zero=0.01):
        self.K, self.L, self.E, self.nw = K, L, E, ob.key_words_for(K)
        self.codes, self.offs = make_reads(synth, K, L, seed, n_reads=n_reads, T=T)
        self.nreads = len(self.offs) - 1
        self.words = synth.pack_2bit(self.codes)
        rng = np.random.default_rng(seed + 7)
        o = self.oracle = ob.Oracle(K, nsets=4)
        o.add_reads(self.codes, self.offs)
        self.keys4 = np.ascontiguousarray(o.export()[0])
        n = len(self.keys4)
        self.cls, self.edge_id, self.twin = random_states(rng, n, E, shares=shares, zero=zero)
        self.path_words = path_words(self.cls, self.edge_id, self.twin)
        lin = ((self.path_words >> np.uint64(1)) & np.uint64(1)).astype(np.int64)
        o.set_node_states(self.keys4, lin, (self.cls == DELETED).astype(np.int64), self.edge_id.astype(np.int64),
                          self.twin.astype(np.int64), (self.cls != FLOATING).astype(np.int64))
        o.set_num_ed(E)
        self.node_of = {k: i for i, k in enumerate(keys4_to_int(self.keys4))}
        self.paths, self.stats = walk_reads(self.codes, self.offs, K, self.node_of, self.cls, self.edge_id, self.twin)
        # patch table: ~70 % of the distinct canonical (K+1)-mers the reads ask for, each a random edge and twin
        cand = {}
        for _, items in self.paths:
            for x in items:
                if not isinstance(x, int) and x not in cand:
                    cand[x] = o.canonical_kplus1(words4_of(x[0]), x[1])
        distinct = sorted({k for k, _ in cand.values()})
        chosen = [k for k, u in zip(distinct, rng.random(len(distinct))) if u < 0.7]
        ptwin = rng.integers(0, 3, size=len(chosen))
        pedge = np.minimum(rng.integers(1, E + 1, size=len(chosen)), E + 1 - ptwin)
        self.patch = {k: (int(e), int(t)) for k, e, t in zip(chosen, pedge, ptwin)}
        for k, (e, t) in self.patch.items():
            o.patch_put(k, e, t)
        self.patch_keys = np.array([k[4 - self.nw:] for k in chosen], dtype=np.uint64).reshape(-1, self.nw)
        self.patch_info = np.array([e | t << 32 for e, t in self.patch.values()], dtype=np.uint64)
        self.candidates, self.patch_missing = len(distinct), len(distinct) - len(chosen)
        self._cand = cand
        # the expectation: the oracle's file; the walk only adds the ordinals of the first appearances
        self.pre_arc = os.path.join(str(tmp_dir), f"o_{K}_{L}_{E}_{seed}.preArc")
        self.narcs, self.arcs = o.read2edge_arcs(self.codes, self.offs, self.pre_arc)
        self.walk_arcs, self.first, self.paths_with_miss = arcs_of_paths(self.paths, self.resolve)

    def resolve(self, x):
        key, ps = self._cand[x]
        e = self.patch.get(key)
        return 0 if e is None else (e[0] if ps else e[0] + e[1] - 1)

    def check_preconditions(self, min_occurrences=1000, min_distinct=0):
        """the inputs reach every branch the tests are about -- judged on the oracle's output and on the walk, never on the device's"""
        mult = [m for _, _, m in self.arcs]
        per_from = {}
        for f, _, _ in self.arcs:
            per_from[f] = per_from.get(f, 0) + 1
        assert self.narcs == len(self.arcs)
        assert sum(mult) >= min_occurrences and len(self.arcs) >= min_distinct, (sum(mult), len(self.arcs))
        assert max(mult) >= 2
        assert max(per_from.values()) >= 3
        assert self.paths_with_miss >= 1 and self.patch_missing >= 1
        assert self.stats["reset_then_vertex"] >= 1
        assert self.stats["zero_linear_items"] >= 1
        assert self.stats["len_k_plus_1"] >= 1 and self.stats["breaks"] >= 1
        assert self.stats["same_item_dropped"] >= 1 or self.E > 6      # few ids: runs of one id, and item == last_item

    def device_order(self, dev_keys):
        """dev_keys uint64[n, nw] of the device's table (any order) -> index of each in self.keys4; the key sets must be equal"""
        mine = self.keys4[:, 4 - self.nw:]
        assert dev_keys.shape == mine.shape, (dev_keys.shape, mine.shape)
        pd = np.lexsort(dev_keys.T[::-1])
        po = np.lexsort(mine.T[::-1])
        assert (dev_keys[pd] == mine[po]).all(), "pass 1 on the device and in the oracle hold different k-mers"
        idx = np.zeros(len(mine), dtype=np.int64)
        idx[pd] = po
        return idx
