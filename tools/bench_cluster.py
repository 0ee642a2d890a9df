#!/usr/bin/env python3
"""sdt_gpu_cluster_begin and sdt_gpu_cluster_reads_device on a counted table, beside two calls that were there before, in one process:
a library of tools/bench_asm.py's kind (torch_workload, resident in HBM) counted into one context.
    python tools/bench_cluster.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 5 --out profiles/read_cluster/bench_cluster_8M_T45000.json
Prints one JSON line.  Every figure is taken after one warm-up call and is the median of --steps (all of them are listed):
  cluster_begin         the wall clock around the blocking call (its kernels, its three waits for counters, the sort of the roots and
                        the component list back to the host); the split by kernel comes from a kernel trace, which is a run of its own:
                        rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_cluster.py ... --steps 1
  cluster_reads_device  the library's events around k_cl_reads (sdt_gpu_kernel_time), the batch that was counted, single reads
  (a) sdt_gpu_profile_reads_device on the same batch: the same probes, and the median on top; the library's events
  (b) sdt_gpu_compare_tables of the table with itself at 64 x 64: two scans with one probe per node, the nearest existing cost of
      "visit every node, probe its neighbours"; the library's events (both passes are booked on the one context)
--limit-s: a cluster_begin that takes longer than this is reported as such and the run ends there (no figure is a gate; a union-find
that needs a better order shows here).  What is clustered is held to the table: live + not live = the nodes, the nodes of all clusters
= live."""
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
from soapdenovo_trans_amd import synth  # noqa: E402
import torch  # noqa: E402

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
ap.add_argument("--limit-s", type=float, default=30.0)
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
est = max(1 << 20, int(1.3 * 2250 * args.T + 0.07 * n * L))
prm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link)
res = {"metric": "sdt_gpu_cluster_begin (wall ms) and sdt_gpu_cluster_reads_device (kernel ms) beside sdt_gpu_profile_reads_device (a) and "
                 "sdt_gpu_compare_tables of the table with itself (b): medians after one warm-up",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "params": prm}
med = lambda v: round(statistics.median(v), 3)


def finish():
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, seed=42, err=args.err)
torch.cuda.synchronize()
with pkg.PregraphGPU(K, est_distinct=est) as g:
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers"], res["nodes"] = g.finish_count()
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    res["library"] = os.path.basename(pkg.LIB_PATH)
    res["slots"] = int(g.table_slots())

    def begin():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = g.cluster_begin(prm)
        return 1e3 * (time.perf_counter() - t0), info

    first_ms, info = begin()                             # warm-up
    res["cluster_begin_first_ms"] = round(first_ms, 3)
    res["info"] = [int(x) for x in info]
    if first_ms > 1e3 * args.limit_s:
        res["cluster_begin_over_limit"] = True
        finish()
        sys.exit(0)
    wall = [begin()[0] for _ in range(args.steps)]
    res["cluster_begin_wall_ms"], res["cluster_begin_ms"] = [round(x, 3) for x in wall], med(wall)
    keys, comp = g.cluster_components()
    res["live_plus_not_live_is_nodes"] = bool(int(info[0]) + int(info[5]) == res["nodes"])
    res["cluster_nodes_sum_to_live"] = bool(int(comp["nodes"].sum()) == int(info[0]) and len(comp) == int(info[2]))
    sizes = sorted(comp["nodes"].tolist(), reverse=True)
    res["largest_clusters"] = sizes[:5]

    d_rec = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)

    def timed(call):
        call()                                           # warm-up
        per = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            g.kernel_time(reset=True)
            call()
            torch.cuda.synchronize()
            per.append(g.kernel_time(reset=True)[0])
        return per

    per = timed(lambda: g.cluster_reads_device(words, offsets, n, d_rec, d_keep))
    res["cluster_reads_kernel_ms"], res["cluster_reads_ms"] = [round(x, 3) for x in per], med(per)
    res["cluster_reads_per_s"] = round(n / (1e-3 * statistics.median(per)))
    rec = d_rec.cpu().numpy().view("uint32")
    res["reads_assigned"] = int((rec[:, 4] != pkg.CLUSTER_NONE).sum())
    res["reads_split"] = int((rec[:, 2] > 0).sum())
    per = timed(lambda: g.profile_reads_device(words, offsets, n, L, args.min_count, d_rec))
    res["a_profile_reads_kernel_ms"], res["a_profile_reads_ms"] = [round(x, 3) for x in per], med(per)
    res["a_profile_reads_per_s"] = round(n / (1e-3 * statistics.median(per)))
    res["cluster_reads_over_profile_reads"] = round(res["cluster_reads_ms"] / res["a_profile_reads_ms"], 3)
    per = timed(lambda: pkg.compare_tables(g, g, 64, 64))
    res["b_compare_self_kernel_ms"], res["b_compare_self_ms"] = [round(x, 3) for x in per], med(per)
    res["cluster_begin_over_compare_self"] = round(res["cluster_begin_ms"] / res["b_compare_self_ms"], 3)
    g.cluster_end()
    res["not_measured"] = ["key widths of 2 and 4 words", "paired batches", "the kept form", "the command line", "a table whose nodes are mostly one cluster"]
finish()
