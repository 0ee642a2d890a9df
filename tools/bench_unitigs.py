#!/usr/bin/env python3
"""sdt_gpu_unitigs_begin on a counted table beside sdt_gpu_cluster_begin and sdt_gpu_bubbles_begin on the same table, in one process: the
library of tools/bench_bubbles.py (allele_workload.py: synth.torch_workload's transcriptome and sampling, resident in HBM, with a
substitution allele in the middle of every tenth transcript).
    python tools/bench_unitigs.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 5 --out profiles/unitigs/bench_unitigs_8M_T45000.json
Prints one JSON line.  Every figure is taken after one warm-up call and is the median of --steps (all of them are listed):
  unitigs_begin   the wall clock around the blocking call (the start scan, the walks, the two sorts, the permutation, the waits for
                  counters); the split by kernel comes from a kernel trace, which is a run of its own:
                  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_unitigs.py ... --steps 1
  cluster_begin   the same for the clustering, whose k_cl_unite makes the same probes per live node: the yardstick
  bubbles_begin   the same for the bubble list
  unitigs_fetch, unitigs_seqs and unitigs_links of the whole list: wall clock
What is found is held to itself: the nodes of the list are the live nodes, the sequence bytes are what unitigs_seqs returns, and every
link is there from both sides.  No figure is a gate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from allele_workload import workload_with_alleles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=8_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--K", type=int, default=31)
ap.add_argument("--T", type=int, default=45000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--min-count", type=int, default=2)
ap.add_argument("--max-count", type=int, default=0)
ap.add_argument("--min-link", type=int, default=1)
ap.add_argument("--max-len", type=int, default=1000, help="of bubbles_begin")
ap.add_argument("--every", type=int, default=10, help="one transcript in this many carries an allele")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
est = max(1 << 20, int(1.3 * 2250 * args.T + 0.07 * n * L))
prm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link)
res = {"metric": "sdt_gpu_unitigs_begin beside sdt_gpu_cluster_begin and sdt_gpu_bubbles_begin on the same table (wall ms of the blocking calls): "
                 "medians after one warm-up",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "params": prm, "allele_every": args.every}
med = lambda v: round(statistics.median(v), 3)

words, offsets, nwords, res["sites_planted"] = workload_with_alleles(n, L, args.T, dev, K, args.every, err=args.err)
torch.cuda.synchronize()
with pkg.PregraphGPU(K, est_distinct=est) as g:
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers"], res["nodes"] = g.finish_count()
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    res["library"] = os.path.basename(pkg.LIB_PATH)
    res["slots"] = int(g.table_slots())

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return 1e3 * (time.perf_counter() - t0), out

    def timed(name, call):
        first_ms, info = wall(call)                          # warm-up
        res[name + "_first_ms"] = round(first_ms, 3)
        per = [wall(call)[0] for _ in range(args.steps)]
        res[name + "_wall_ms"], res[name + "_ms"] = [round(x, 3) for x in per], med(per)
        return info

    info = timed("unitigs_begin", lambda: g.unitigs_begin(prm))
    res["info"] = [int(x) for x in info]
    cinfo = timed("cluster_begin", lambda: g.cluster_begin(prm))
    binfo = timed("bubbles_begin", lambda: g.bubbles_begin(dict(prm, max_len=args.max_len)))
    res["unitigs_begin_over_cluster_begin"] = round(res["unitigs_begin_ms"] / res["cluster_begin_ms"], 3)
    res["unitigs_begin_over_bubbles_begin"] = round(res["unitigs_begin_ms"] / res["bubbles_begin_ms"], 3)
    res["same_live_nodes"] = bool(int(info[0]) == int(cinfo[0]) == int(binfo[0]) == int(info[4]))
    g.cluster_end()
    g.bubbles_end()
    nu = int(info[2])
    fetch_ms, (keys, rec) = wall(lambda: g.unitigs_fetch(0, nu))
    seqs_ms, (bases, offs) = wall(lambda: g.unitigs_seqs(0, nu))
    links_ms, (links, dangling) = wall(lambda: g.unitigs_links(0, nu))
    res["unitigs_fetch_ms"], res["unitigs_seqs_ms"], res["unitigs_links_ms"] = round(fetch_ms, 3), round(seqs_ms, 3), round(links_ms, 3)
    res["seq_bytes_agree"] = bool(int(offs[-1]) == int(info[5]) == len(bases))
    res["links"], res["dangling"] = len(links), int(dangling)
    o, o2 = links["info"] & 1, links["info"] >> 1 & 1
    there = np.stack([links["from"], o, links["to"], o2], axis=1)
    back = np.stack([links["to"], 1 - o2, links["from"], 1 - o], axis=1)
    res["links_from_both_sides"] = bool(len(np.unique(there, axis=0)) == len(np.unique(np.concatenate([there, back]), axis=0)))
    nodes = rec["nodes"].astype(np.int64)
    deg_in, deg_out = rec["info"] >> 4 & 15, rec["info"] >> 8 & 15
    res["single_node_unitigs"] = int((nodes == 1).sum())
    res["isolated"] = int(((deg_in == 0) & (deg_out == 0)).sum())
    res["dead_ends"] = int(((deg_in == 0) != (deg_out == 0)).sum())
    res["median_nodes"], res["mean_nodes"] = int(np.median(nodes)) if nu else 0, round(float(nodes.mean()), 2) if nu else 0
    by_len = np.sort(nodes + K - 1)[::-1]
    half = np.searchsorted(np.cumsum(by_len) * 2, int(by_len.sum()))
    res["n50_bases"] = int(by_len[min(half, len(by_len) - 1)]) if nu else 0
    g.unitigs_end()
    res["not_measured"] = ["key widths of 2 and 4 words", "the command line", "a table with a cycle (the bit per slot and the second scan)"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
