#!/usr/bin/env python3
"""sdt_gpu_bubbles_begin on a counted table beside sdt_gpu_cluster_begin on the same table, in one process: the library of
tools/bench_cluster.py (synth.torch_workload's transcriptome and sampling, resident in HBM) with a substitution allele in a tenth of the
transcripts -- every tenth transcript has one site in its middle, and half of the reads that cover it carry the other base -- so that
there is something to find.
    python tools/bench_bubbles.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 5 --out profiles/bubbles/bench_bubbles_8M_T45000.json
Prints one JSON line.  Every figure is taken after one warm-up call and is the median of --steps (all of them are listed):
  bubbles_begin   the wall clock around the blocking call (the fork scan, the walks, the sort, the permutation, four waits for counters);
                  the split by kernel comes from a kernel trace, which is a run of its own:
                  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_bubbles.py ... --steps 1
  cluster_begin   the same for the clustering, whose k_cl_unite makes the same probes per live node: the yardstick
  bubbles_fetch + bubbles_paths of the whole list: wall clock
What is found is held to what was planted: the bubbles with K inner nodes on both sides are counted against the planted sites.
No figure is a gate."""
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
ap.add_argument("--max-len", type=int, default=1000)
ap.add_argument("--every", type=int, default=10, help="one transcript in this many carries an allele")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
est = max(1 << 20, int(1.3 * 2250 * args.T + 0.07 * n * L))
prm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link, max_len=args.max_len)
cprm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link)
res = {"metric": "sdt_gpu_bubbles_begin beside sdt_gpu_cluster_begin on the same table (wall ms of the blocking calls): medians after one warm-up",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "params": prm, "allele_every": args.every}
med = lambda v: round(statistics.median(v), 3)


def finish():
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


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

    first_ms, info = wall(lambda: g.bubbles_begin(prm))      # warm-up
    res["bubbles_begin_first_ms"] = round(first_ms, 3)
    res["info"] = [int(x) for x in info]
    per = [wall(lambda: g.bubbles_begin(prm))[0] for _ in range(args.steps)]
    res["bubbles_begin_wall_ms"], res["bubbles_begin_ms"] = [round(x, 3) for x in per], med(per)
    first_ms, cinfo = wall(lambda: g.cluster_begin(cprm))
    res["cluster_begin_first_ms"] = round(first_ms, 3)
    per = [wall(lambda: g.cluster_begin(cprm))[0] for _ in range(args.steps)]
    res["cluster_begin_wall_ms"], res["cluster_begin_ms"] = [round(x, 3) for x in per], med(per)
    res["bubbles_begin_over_cluster_begin"] = round(res["bubbles_begin_ms"] / res["cluster_begin_ms"], 3)
    res["same_live_nodes"] = bool(int(info[0]) == int(cinfo[0]))
    g.cluster_end()
    nb = int(info[4])
    fetch_ms, (keys, rec) = wall(lambda: g.bubbles_fetch(0, nb))
    paths_ms, (bases, offs) = wall(lambda: g.bubbles_paths(0, nb))
    res["bubbles_fetch_ms"], res["bubbles_paths_ms"] = round(fetch_ms, 3), round(paths_ms, 3)
    res["path_bytes_agree"] = bool(int(offs[-1]) == int(info[5]) == len(bases))
    same = rec["len_a"] == rec["len_b"]
    res["kind0"] = int((same & (rec["len_a"] == K)).sum())
    res["kind1"] = int((same & (rec["len_a"] != K)).sum())
    res["kind2"] = int((~same).sum())
    res["kind0_with_both_sides_min_5"] = int((same & (rec["len_a"] == K) & (rec["min_a"] >= 5) & (rec["min_b"] >= 5)).sum())
    g.bubbles_end()
    res["not_measured"] = ["key widths of 2 and 4 words", "the command line", "indels and skipped exons at this size"]
finish()
