"""Helpers of tests/test_fullsize_paths.py: inputs, the oracle's answer as row-sorted numpy arrays, the comparison of a counted context with it,
read placement at high base offsets, and the child process that runs a case with the library's size knobs in its environment.

The size thresholds of the locality pipeline (csrc/sdt_pipeline.hpp) are `static const`: they are read when the library is loaded, so a case
that shrinks one runs in a child process (`python fullsize_paths_util.py spec.json`), the way tests/test_spills.py runs its variant library.
The parent makes the input and the oracle's answer on the CPU and hands both over in an .npz; the child only drives the GPU and compares."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO32 = 1 << 32


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def hot_reads(n, L):
    """the input of test_saturation_and_hot_keys at another size: two thirds poly-A, one third the tandem repeat ACTGGC"""
    na = n * 2 // 3
    codes = np.zeros(n * L, dtype=np.uint8)
    codes[L * na:] = np.tile(np.array([0, 1, 2, 3, 3, 1], dtype=np.uint8), (n - na) * L // 6 + 1)[: (n - na) * L]
    return codes, (np.arange(n + 1, dtype=np.uint64) * L)


def mixed_reads(synth, K, n_hot, L, n_tx=6000):
    """the hot reads + ragged reads with errors off make_transcriptome(12)"""
    hc, ho = hot_reads(n_hot, L)
    tx = synth.make_transcriptome(12, seed=K)
    tc, to = synth.sample_reads(*tx, n_reads=n_tx, read_len=L, seed=K + 1, err=0.01, ragged=True)
    return np.concatenate([hc, tc]), np.concatenate([ho, to[1:] + ho[-1]])


# ---- the oracle's answer ----------------------------------------------------------------------------------------------------------------
def _oracle_flags(fl):
    """oracle flags (bit 0 linear, 1 deleted, 2 single) -> the top byte of r_flags (linear, deleted, checked, single)"""
    fl = fl.astype(np.uint32)
    return (fl & 1) | ((fl >> 1 & 1) << 1) | ((fl >> 2 & 1) << 3)


def row_order(keys):
    """the order that sorts key rows (most significant word first)"""
    order = np.argsort(keys[:, 0], kind="stable")
    first = keys[order, 0]
    if keys.shape[1] > 1 and (first[1:] == first[:-1]).any():           # (rows that share the first word: the full comparison)
        order = np.lexsort(keys.T[::-1])
    return order


def oracle_answer(ob, K, pushes, nsets=4, with_first=True, ds=(0, 2)):
    """the oracle over the pushes [(codes, offs)] in order -> a dict of arrays: k-mers, nodes, and for d = 0 and after delow(2) the
    histogram, the linear count and every node's links, flags and count in key order; the sorted first ordinals"""
    o = ob.Oracle(K, nsets=nsets)
    nw = o.nw
    for codes, offs in pushes:
        o.add_reads(codes, offs)
    ans = {"kmers": np.uint64(o.kmers_in_reads()), "nodes": np.uint64(o.node_count())}
    if with_first:
        ans["first"] = np.sort(o.export_first())
    for d in ds:
        if d:
            ans["removed2"] = np.uint64(o.delow(d))
        hist, linear = o.mark()
        keys, l, r, cnt, fl = o.export()
        assert not keys[:, : 4 - nw].any()
        keys = np.ascontiguousarray(keys[:, 4 - nw:])
        order = row_order(keys)
        ans[f"hist{d}"], ans[f"linear{d}"] = hist, np.uint64(linear)
        ans[f"keys{d}"], ans[f"l{d}"], ans[f"r{d}"], ans[f"cnt{d}"], ans[f"fl{d}"] = keys[order], l[order], r[order], cnt[order], _oracle_flags(fl[order])
    return ans


def gpu_table(g, with_first=False):
    """export_nodes in key order: keys, l_links, r links (24 bits), flags (the top byte), count[, first]"""
    out = g.export_nodes(with_first=with_first)
    order = row_order(out[0])
    keys, l, rf, cnt = (a[order] for a in out[:4])
    return (keys, l, rf & np.uint32(0xFFFFFF), rf >> np.uint32(24), cnt) + ((out[4],) if with_first else ())


def assert_table(got, ans, d, what=""):
    names = ("keys", "l", "r", "fl", "cnt")
    want = tuple(ans[f"{n}{d}"] for n in names)
    assert len(got[0]) == len(want[0]), (what, d, "nodes", len(got[0]), len(want[0]))
    for n, a, b in zip(names, got, want):
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, (what, f"d={d}", n, f"{bad.size} nodes differ, the first", [(int(i), [hex(int(x)) for x in ans[f'keys{d}'][i]],
                                                                                           a[i].tolist(), b[i].tolist()) for i in bad[:5]])


def compare_with_answer(g, ans, track, what=""):
    """what test_node_table_equals_oracle asserts, on arrays: k-mers and nodes, histogram and linear count, every node's links, flags and
    count, -d 2 and the same again; with tracking the sorted first ordinals"""
    kmers, nodes = g.finish_count()
    assert (kmers, nodes) == (int(ans["kmers"]), int(ans["nodes"])), (what, kmers, nodes, int(ans["kmers"]), int(ans["nodes"]))
    for d in (0, 2):
        if d:
            assert g.delow(d) == int(ans["removed2"]), (what, "delow")
        hist, linear = g.mark_and_hist()
        assert linear == int(ans[f"linear{d}"]), (what, d, linear, int(ans[f"linear{d}"]))
        assert (hist == ans[f"hist{d}"]).all(), (what, d, "kmerFreq histogram")
        got = gpu_table(g, with_first=bool(track) and d == 0)
        assert_table(got[:5], ans, d, what)
        if track and d == 0:
            assert (np.sort(got[5]) == ans["first"]).all(), (what, "first ordinals")


def level1_buckets_touched(pkg, ans):
    """the level-1 buckets (of 256) that the oracle's distinct keys fall into"""
    K = int(ans["K"])
    return len({pkg.kmer_bucket(row, K) for row in ans["keys0"]})


def final_buckets_touched(pkg, ans):
    """B of the pigeonhole conditions: the final buckets (of 2^18) that the oracle's distinct keys fall into"""
    K = int(ans["K"])
    return len({pkg.kmer_final_bucket(row, K) for row in ans["keys0"]})


# ---- reads at high base offsets ---------------------------------------------------------------------------------------------------------
def place_reads(codes, offs, S, pad_words=4):
    """the reads packed so that the first one starts at absolute base S of a word buffer -> (words: the piece of the buffer that holds them
    + pad_words zero words, the word index at which the piece lies, the absolute offsets).  Bases of the first word in front of S are zero."""
    codes = np.asarray(codes, dtype=np.uint8)
    lead = S & 15
    n = lead + codes.size
    buf = np.zeros((n + 15) // 16 * 16, dtype=np.uint32)
    buf[lead:n] = codes
    shifts = (30 - 2 * np.arange(16)).astype(np.uint32)
    words = np.bitwise_or.reduce(buf.reshape(-1, 16) << shifts, axis=1).astype(np.uint32)
    return np.concatenate([words, np.zeros(pad_words, dtype=np.uint32)]), S >> 4, np.asarray(offs, dtype=np.uint64) + np.uint64(S)


def unpack_placed(words, w0, abs_offs):
    """the inverse, by the definition of the packed format (include/sdt_gpu.h): base i of the buffer is bits 31 - 2 (i & 15) .. of word i >> 4"""
    lo, hi = int(abs_offs[0]), int(abs_offs[-1])
    i = np.arange(lo, hi, dtype=np.int64)
    return ((words[(i >> 4) - w0] >> (30 - 2 * (i & 15)).astype(np.uint32)) & 3).astype(np.uint8)


# ---- the child ------------------------------------------------------------------------------------------------------------------------
def run_child(tmp_path, name, env_knobs, spec, arrays, timeout):
    """run `spec` in a child process with env_knobs in its environment -> the child's result (a dict); a child that fails, faults or aborts
    fails the test with the end of its output and is not run again"""
    npz = os.path.join(str(tmp_path), name + ".npz")
    np.savez(npz, **arrays)
    spec = dict(spec, npz=npz, name=name)
    sp = os.path.join(str(tmp_path), name + ".json")
    with open(sp, "w") as f:
        json.dump(spec, f)
    env = dict(os.environ, **{k: str(v) for k, v in env_knobs.items()})
    assert env.get("SDT_TEST_HOOKS") == "1"              # (tests/conftest.py: the size knobs are test hooks)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), sp], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _child(spec_path):
    """spec: K, flags (a list: one context per entry and repetition), est_distinct, reps, steps = [["push", r0, r1] | ["device", r0, r1] |
    ["finish"]]; the .npz holds the input (codes, offs) and the oracle's answer (oracle_answer)
    -> prints one JSON line: the pipeline counters of every run"""
    import time
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from soapdenovo_trans_amd import synth
    with open(spec_path) as f:
        spec = json.load(f)
    z = np.load(spec["npz"])
    ans = {k: z[k] for k in z.files}
    codes, offs = ans.pop("codes"), ans.pop("offs")
    K = spec["K"]
    ans["K"] = K
    pieces = {}
    for step in spec["steps"]:
        if step[0] in ("push", "device") and (step[1], step[2]) not in pieces:
            r0, r1 = step[1], step[2]
            b0 = int(offs[r0])
            pieces[(r0, r1)] = (synth.pack_2bit(codes[b0: int(offs[r1])]), offs[r0: r1 + 1] - offs[r0])
    out = {"runs": []}
    t0 = time.time()
    for rep in range(spec.get("reps", 1)):
        for flags in spec["flags"]:
            with pkg.PregraphGPU(K, est_distinct=spec["est_distinct"], flags=flags) as g:
                for step in spec["steps"]:
                    if step[0] == "finish":
                        g.finish_count()                             # (SDT_ESTATE of the conservation check raises here)
                    elif step[0] == "push":
                        g.push_reads(*pieces[(step[1], step[2])])
                    else:
                        import torch
                        w, o = pieces[(step[1], step[2])]
                        d_w = torch.from_numpy(w.view(np.int32)).cuda()
                        d_o = torch.from_numpy(o.astype(np.int64)).cuda()
                        torch.cuda.synchronize()
                        g.count_reads_device(d_w, len(w), d_o, len(o) - 1, int(np.diff(o.astype(np.int64)).max()))
                track = bool(flags & pkg.SDT_FLAG_TRACK_FIRST)
                compare_with_answer(g, ans, track, f"{spec['name']} flags={flags} rep={rep}")
                out["runs"].append(g.stage_times()[1])
    out["gpu_seconds"] = round(time.time() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    _child(sys.argv[1])
