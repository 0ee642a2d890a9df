"""Helpers of tests/test_fused_clear.py: the child process that runs its scenarios with the library's knobs in its environment.

SDT_LAZY_CLEAR and SDT_TABLE_SLOT_ROUND are read once per process, so a set of scenarios under one setting runs in one child
(`python fused_clear_util.py spec.json`), the way tests/fullsize_paths_util.py runs its cases.  The parent makes the reads and the
oracle's answers on the CPU and hands them over in an .npz; the child drives the GPU and compares.

Every scenario starts by counting job A (`a`: the reads [a0, a1) of the A stream) and calling reset, so that a slot that reset's
deferred clear misses shows up as a node of A.  Then, by `kind`:
  count    job B is pushed in the pieces of `pushes` and compared with the oracle of B alone (every node, the histogram, `linear`,
           before and after delow(2)); reported: the slots at reset, the pipeline counters, a digest of what was compared
  empty    finish_count + mark_and_hist + export_nodes see an empty table
  search   none of A's keys is found
  import   half of A's nodes are imported and come back, and nothing else
  reset2   a second reset, then as count
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(tmp_path, name, env_knobs, scenarios, arrays, timeout=600):
    npz = os.path.join(str(tmp_path), name + ".npz")
    np.savez(npz, **arrays)
    sp = os.path.join(str(tmp_path), name + ".json")
    with open(sp, "w") as f:
        json.dump({"npz": npz, "scenarios": scenarios}, f)
    env = dict(os.environ, **{k: str(v) for k, v in env_knobs.items()})
    assert env.get("SDT_TEST_HOOKS") == "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), sp], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _piece(synth, codes, offs, r0, r1):
    b0 = int(offs[r0])
    return synth.pack_2bit(codes[b0: int(offs[r1])]), offs[r0: r1 + 1] - offs[r0]


def _digest(fu, g, ans, track):
    """what compare_with_answer has just found equal to the oracle, as the library returned it after delow(2), in one hash"""
    h = hashlib.sha1()
    hist, linear = g.mark_and_hist()
    h.update(np.asarray(hist, dtype=np.int64).tobytes())
    h.update(np.uint64(linear).tobytes())
    for a in fu.gpu_table(g):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _child(spec_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import fullsize_paths_util as fu
    pkg = ge.load_package()
    from soapdenovo_trans_amd import synth
    with open(spec_path) as f:
        spec = json.load(f)
    z = np.load(spec["npz"])
    arr = {k: z[k] for k in z.files}
    out = {}
    for sc in spec["scenarios"]:
        K, flags, name = sc["K"], sc["flags"], sc["name"]
        track = bool(flags & pkg.SDT_FLAG_TRACK_FIRST)
        ans = {k[len(sc["ans"]):]: v for k, v in arr.items() if k.startswith(sc["ans"])}
        ans["K"] = K
        res = {}
        with pkg.PregraphGPU(K, est_distinct=sc["est_distinct"], flags=flags) as g:
            g.push_reads(*_piece(synth, arr["a_codes"], arr["a_offs"], sc["a"][0], sc["a"][1]))
            a_kmers, a_nodes = g.finish_count()
            assert a_nodes > 1000, (name, "job A left no nodes", a_nodes)
            a_table = g.export_nodes() if sc["kind"] in ("search", "import") else None
            g.reset()
            res["slots"] = g.table_slots()
            if sc["kind"] == "reset2":
                g.reset()
            if sc["kind"] in ("count", "reset2"):
                for r0, r1 in sc["pushes"]:
                    g.push_reads(*_piece(synth, arr["b_codes"], arr["b_offs"], r0, r1))
                fu.compare_with_answer(g, ans, track, name)
                ms, res["counters"] = g.stage_times()
                res["direct_ms"], res["scatter_ms"] = ms[0], ms[1]
                res["kmers"] = int(ans["kmers"])
                res["digest"] = _digest(fu, g, ans, track)
            elif sc["kind"] == "empty":
                assert g.finish_count() == (0, 0), (name, "finish_count after reset")
                hist, linear = g.mark_and_hist()
                assert linear == 0 and not np.asarray(hist).any(), (name, "mark_and_hist after reset", linear)
                assert len(g.export_nodes()[0]) == 0, (name, "export_nodes after reset")
                res["counters"] = g.stage_times()[1]
            elif sc["kind"] == "search":
                keys = a_table[0][::3]
                count, l, r, status = g.search_kmers(keys)
                assert not status.any() and not count.any(), (name, "keys of job A found after reset", int(np.count_nonzero(status)))
                res["counters"] = g.stage_times()[1]
            elif sc["kind"] == "import":
                keys, l, rf, cnt = (np.ascontiguousarray(a[::2]) for a in a_table)
                g._check(g.lib.sdt_gpu_import_nodes(g._ctx, pkg._ptr(keys), pkg._ptr(l), pkg._ptr(rf), pkg._ptr(cnt), None, len(keys)))
                assert g.finish_count()[1] == len(keys), (name, "nodes after import")
                got = g.export_nodes()
                o0, o1 = fu.row_order(got[0]), fu.row_order(keys)
                for x, y in zip(got, (keys, l, rf, cnt)):
                    assert (x[o0] == y[o1]).all(), (name, "imported nodes differ")
                res["counters"] = g.stage_times()[1]
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    _child(sys.argv[1])
