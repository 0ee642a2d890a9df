"""GPU (-m gpu): what the entry points of the graph unit answer in every state a caller can put them in -- a characterisation,
so that a change of a check, of its place in the order of the checks or of its words shows.

Every case is (return code, exact text of sdt_gpu_last_error); SEEN collects them, EXPECT is the table they are compared with.
The input is 200 reads of 50 bases over one short transcript with 2 % errors (tips and junctions at K = 21, 1-word keys); a
second context at K = 33 (2-word keys) answers for the width refusals.  The calls go to g.lib.sdt_gpu_* with g._ctx where the
Python wrapper would size the arrays itself.

Two kinds of refusal.  Those the host decides (arguments, state, a record array that is too small) leave the context as it was:
the tip walks taken at the end of the main context equal the ones taken before.  Those a kernel counts (a key that is not a node,
an order entry that is no rank, a node index past the last node) leave their count in the context's device counters until
sdt_gpu_reset: each has a context of its own here, and what the next call on it answers is part of the table."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, K_WIDE = 21, 33
P, CUT = 4, 2 * K
THRESHOLD = 0.3
NO_INDEX = "call sdt_gpu_set_node_index first"
NO_NUMBERING = "call sdt_gpu_layout_apply (or sdt_gpu_set_node_index) first"
NO_FIRST = "first-occurrence ordinals were not tracked: init with SDT_FLAG_TRACK_FIRST"


def _reads(synth):
    tx = synth.make_transcriptome(1, seed=5, lo=400, hi=400)
    codes, offs = synth.sample_reads(*tx, n_reads=200, read_len=50, seed=6, err=0.02)
    return synth.pack_2bit(codes), offs


def _counted(pkg, synth, k=K, flags=0):
    g = pkg.PregraphGPU(k, est_distinct=1 << 14, flags=flags)
    g.push_reads(*_reads(synth))
    g.finish_count()
    g.mark_and_hist()
    return g


def _u64(n, fill=0):
    return np.full(max(int(n), 1), fill, dtype=np.uint64)


def _u32(n):
    return np.zeros(max(int(n), 1), dtype=np.uint32)


def _not_a_node(keys):
    have = {int(k) for k in keys[:, 0]}
    bogus = next(int(keys[0, 0]) ^ d for d in range(1, 1 << 20) if int(keys[0, 0]) ^ d not in have)
    out = keys.copy()
    out[0, 0] = np.uint64(bogus)
    return out


class Seen(dict):
    def __init__(self, pkg):
        super().__init__()
        self.names = {getattr(pkg, s): s for s in ("SDT_OK", "SDT_EINVAL", "SDT_ESTATE", "SDT_EFULL", "SDT_ENOMEM", "SDT_EHIP", "SDT_ELIMIT")}

    def ask(self, case, g, fn, *args):
        rc = getattr(g.lib, fn)(g._ctx, *args)
        got = (self.names.get(rc, f"code {rc}"), g.lib.sdt_gpu_last_error().decode() if rc else "")
        print(f"{case}: {got}")
        assert case not in self
        self[case] = got
        return rc


def observe(pkg, synth):
    """-> (what every case answered, what it is expected to answer)"""
    seen, want = Seen(pkg), {}
    ptr, ref = pkg._ptr, ctypes.byref
    n_out, nj, nr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    dbl = ctypes.c_double(THRESHOLD)
    ss = _u64(P + 1)

    # ---- a context without first-occurrence ordinals, never numbered: the layout refuses, everything else asks for an index
    with _counted(pkg, synth) as g:
        n = len(g.export_nodes()[0])
        assert n > 100
        keys, end, info, rec, l, r = np.zeros((n, 1), dtype=np.uint64), _u64(n), np.zeros(n, dtype=np.uint8), _u64(17 * n), _u32(n), _u32(n)
        seen.ask("no first: layout_sorted_keys", g, "sdt_gpu_layout_sorted_keys", P, 1, ptr(keys), n, ptr(ss), ref(n_out))
        seen.ask("no first: layout_on_device", g, "sdt_gpu_layout_on_device", P, 1, 0, ptr(ss), ref(n_out))
        want["no first: layout_sorted_keys"] = want["no first: layout_on_device"] = ("SDT_ESTATE", NO_FIRST)
        seen.ask("no index: layout_apply", g, "sdt_gpu_layout_apply", ptr(_u64(5)), 5)
        want["no index: layout_apply"] = ("SDT_ESTATE", "call sdt_gpu_layout_sorted_keys first (it sorted 0 nodes, the order has 5)")
        seen.ask("no index: export_ordered", g, "sdt_gpu_export_ordered", ptr(keys), ptr(l), ptr(r), ptr(_u32(n)), n)
        want["no index: export_ordered"] = ("SDT_ESTATE", f"call sdt_gpu_layout_apply first (it numbered 0 nodes, the arrays hold {n})")
        seen.ask("no index: update_nodes_by_index", g, "sdt_gpu_update_nodes_by_index", ptr(_u64(1)), ptr(l), ptr(r), 1)
        want["no index: update_nodes_by_index"] = ("SDT_ESTATE", "call sdt_gpu_layout_apply first")
        seen.ask("no index: tip_walks", g, "sdt_gpu_tip_walks", 0, CUT, ptr(end), ptr(info), n)
        seen.ask("no index: tip_walks_compact", g, "sdt_gpu_tip_walks_compact", 0, CUT, ptr(rec), n, ref(nr))
        seen.ask("no index: minor_out_dry", g, "sdt_gpu_minor_out_dry", dbl, ptr(rec), n, ref(nj), ref(nr))
        seen.ask("no index: edge_ports", g, "sdt_gpu_edge_ports", ptr(rec), n, ref(nr))
        seen.ask("no index: build_host_index", g, "sdt_gpu_build_host_index", ptr(_u32(4 * n)), 1 << 20)
        seen.ask("no index: build_host_index64", g, "sdt_gpu_build_host_index64", ptr(_u64(4 * n)), 1 << 20)
        for fn in ("tip_walks", "tip_walks_compact", "minor_out_dry", "edge_ports", "build_host_index", "build_host_index64"):
            want[f"no index: {fn}"] = ("SDT_ESTATE", NO_INDEX)
        seen.ask("no index: tip_walks_labelled", g, "sdt_gpu_tip_walks_labelled", 0, CUT, ref(nr))
        seen.ask("no index: minor_out_labelled", g, "sdt_gpu_minor_out_labelled", dbl, ref(nj), ref(nr))
        want["no index: tip_walks_labelled"] = want["no index: minor_out_labelled"] = ("SDT_ESTATE", NO_NUMBERING)

    # ---- 2-word keys: a variant of fewer words cannot hold them
    with _counted(pkg, synth, K_WIDE, pkg.SDT_FLAG_TRACK_FIRST) as g:
        m = len(g.export_nodes()[0])
        wide = np.zeros((m, 2), dtype=np.uint64)
        seen.ask("wide: layout_sorted_keys nw 1", g, "sdt_gpu_layout_sorted_keys", P, 1, ptr(wide), m, ptr(ss), ref(n_out))
        seen.ask("wide: layout_on_device nw 1", g, "sdt_gpu_layout_on_device", P, 1, 0, ptr(ss), ref(n_out))
        want["wide: layout_sorted_keys nw 1"] = want["wide: layout_on_device nw 1"] = ("SDT_EINVAL", "a 1-word variant cannot hold 2-word keys")

    # ---- the main context: arguments, state, record arrays that are too small; it works as before after all of them
    with _counted(pkg, synth, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        assert len(g.export_nodes()[0]) == n
        for fn, tail in (("layout_sorted_keys", (ptr(keys), n, ptr(ss), ref(n_out))), ("layout_on_device", (0, ptr(ss), ref(n_out)))):
            for p in (0, 257):
                seen.ask(f"{fn} p {p}", g, f"sdt_gpu_{fn}", p, 1, *tail)
                want[f"{fn} p {p}"] = ("SDT_EINVAL", f"layout on the device: 1..256 sets, asked for {p}")
            for nw in (0, 5):
                seen.ask(f"{fn} nw {nw}", g, f"sdt_gpu_{fn}", P, nw, *tail)
                want[f"{fn} nw {nw}"] = ("SDT_EINVAL", f"a {nw}-word variant cannot hold 1-word keys")
            seen.ask(f"{fn} NULL n_out", g, f"sdt_gpu_{fn}", P, 1, *tail[:-1], None)
            want[f"{fn} NULL n_out"] = ("SDT_EINVAL", "NULL argument")
        seen.ask("layout_sorted_keys max_nodes", g, "sdt_gpu_layout_sorted_keys", P, 1, ptr(keys), n - 1, ptr(ss), ref(n_out))
        want["layout_sorted_keys max_nodes"] = ("SDT_EINVAL", f"key array holds {n - 1} nodes, the table has {n}")
        skeys, _ = g.layout_sorted_keys(P, 1)
        order = np.arange(n, dtype=np.uint64)
        seen.ask("layout_apply wrong n", g, "sdt_gpu_layout_apply", ptr(order), n - 1)
        want["layout_apply wrong n"] = ("SDT_ESTATE", f"call sdt_gpu_layout_sorted_keys first (it sorted {n} nodes, the order has {n - 1})")
        g.layout_apply(order)
        seen.ask("export_ordered wrong n", g, "sdt_gpu_export_ordered", ptr(keys), ptr(l), ptr(r), ptr(_u32(n)), n - 1)
        want["export_ordered wrong n"] = ("SDT_ESTATE", f"call sdt_gpu_layout_apply first (it numbered {n} nodes, the arrays hold {n - 1})")
        assert (g.export_ordered()[0] == skeys).all()
        before = g.tip_walks_compact(False, CUT)
        seen.ask("tip_walks wrong n", g, "sdt_gpu_tip_walks", 0, CUT, ptr(end), ptr(info), n - 1)
        want["tip_walks wrong n"] = ("SDT_EINVAL", f"the node index holds {n} nodes, the output arrays {n - 1}")
        pow2 = 1 << (2 * n - 1).bit_length()                      # the smallest power of two >= 2 n
        for fn, idx in (("build_host_index", _u32(pow2 + 1)), ("build_host_index64", _u64(pow2 + 1))):
            for what, slots in (("no power of two", pow2 + 1), ("below 2 x nodes", pow2 // 2)):
                seen.ask(f"{fn} {what}", g, f"sdt_gpu_{fn}", ptr(idx), slots)
                want[f"{fn} {what}"] = ("SDT_EINVAL", "index_slots must be a power of two >= 2 x nodes")
        # a record array of 0 records on a graph that has records: SDT_EFULL and the true counts; with that room the call succeeds
        full = {"tip_walks_compact": ((0, CUT), 2, "nodes have a walk", False), "edge_ports": ((), 17, "the graph has %d non-linear nodes", False),
                "minor_out_dry": ((dbl,), 9, "the pass needs %d", True)}
        for fn, (head, words, text, junctions) in full.items():
            counts = (ref(nj), ref(nr)) if junctions else (ref(nr),)
            nj.value = nr.value = 0
            seen.ask(f"{fn} no room", g, f"sdt_gpu_{fn}", *head, None, 0, *counts)
            need, need_j = nr.value, nj.value
            assert need > 0 and (need_j > 0 or not junctions), (fn, need, need_j)
            want[f"{fn} no room"] = ("SDT_EFULL", "record array holds 0, " + (text % need if "%d" in text else f"{need} {text}"))
            room = np.zeros((need, words), dtype=np.uint64)
            nj.value = nr.value = 0
            seen.ask(f"{fn} with room", g, f"sdt_gpu_{fn}", *head, ptr(room), need, *counts)
            want[f"{fn} with room"] = ("SDT_OK", "")
            assert (nr.value, nj.value) == (need, need_j) and room[:, 0].any(), fn
            if fn == "tip_walks_compact":
                assert sorted(map(tuple, room)) == sorted(map(tuple, before))
        after = g.tip_walks_compact(False, CUT)
        assert len(before) > 0 and sorted(map(tuple, after)) == sorted(map(tuple, before))

    # ---- refusals that a kernel counts, one context each; the call after it
    bogus = _not_a_node(skeys)
    with _counted(pkg, synth) as g:
        seen.ask("set_node_index: not a node", g, "sdt_gpu_set_node_index", ptr(bogus), n)
        want["set_node_index: not a node"] = ("SDT_ESTATE", "sdt_gpu_set_node_index: 1 nodes are not in the table")
        seen.ask("set_node_index: the call after", g, "sdt_gpu_tip_walks_compact", 0, CUT, ptr(rec), n, ref(nr))
        want["set_node_index: the call after"] = ("SDT_ESTATE", NO_INDEX)
    with _counted(pkg, synth) as g:
        g.set_node_index(skeys)
        seen.ask("update_nodes: not a node", g, "sdt_gpu_update_nodes", ptr(bogus), ptr(l), ptr(r), 1)
        want["update_nodes: not a node"] = ("SDT_ESTATE", "sdt_gpu_update_nodes: 1 nodes are not in the table")
        seen.ask("update_nodes: the call after", g, "sdt_gpu_tip_walks_compact", 0, CUT, ptr(rec), n, ref(nr))
        want["update_nodes: the call after"] = ("SDT_ESTATE", "sdt_gpu_tip_walks_compact: 1 walks left the graph")
    with _counted(pkg, synth, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.layout_sorted_keys(P, 1)
        bad = order.copy()
        bad[n // 2] = n
        seen.ask("layout_apply: no rank", g, "sdt_gpu_layout_apply", ptr(bad), n)
        want["layout_apply: no rank"] = ("SDT_EINVAL", f"layout order: 1 entries are not ranks below {n}")
        seen.ask("layout_apply: the call after", g, "sdt_gpu_tip_walks_compact", 0, CUT, ptr(rec), n, ref(nr))
        want["layout_apply: the call after"] = ("SDT_ESTATE", NO_INDEX)
    with _counted(pkg, synth, flags=pkg.SDT_FLAG_TRACK_FIRST) as g:
        g.layout_sorted_keys(P, 1)
        g.layout_apply(order)
        seen.ask("update_nodes_by_index: past the last node", g, "sdt_gpu_update_nodes_by_index", ptr(_u64(1, n)), ptr(l), ptr(r), 1)
        want["update_nodes_by_index: past the last node"] = ("SDT_EINVAL", "sdt_gpu_update_nodes_by_index: 1 indices past the last node")
        seen.ask("update_nodes_by_index: the call after", g, "sdt_gpu_tip_walks_compact", 0, CUT, ptr(rec), n, ref(nr))
        want["update_nodes_by_index: the call after"] = ("SDT_ESTATE", "sdt_gpu_tip_walks_compact: 1 walks left the graph")
    return dict(seen), want


def test_graph_entry_points_answer_every_state_as_recorded(pkg, synth):
    seen, want = observe(pkg, synth)
    assert set(seen) == set(want)
    assert {k: v for k, v in seen.items() if v != want[k]} == {}
    assert seen == want
