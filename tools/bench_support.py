#!/usr/bin/env python3
"""sdt_gpu_unitigs_support_add_device, without and with pairs, beside sdt_gpu_unitigs_reads_device in its size-only and its full form on
the same reads, table, list and index, in one process and alternating: the library of tools/bench_thread.py (allele_workload.py).
    python tools/bench_support.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 5 --out profiles/unitig_support/bench_support_8M_T45000.json
Prints one JSON line.  Every figure is the wall clock around the blocking call, taken after one warm-up call, and is the median of --steps
(all of them are listed):
  support_add_device         k_sp_reads once over the reads as single reads, and the wait for its counters
  support_add_device_paired  the same over reads 2r, 2r + 1 as pairs (one wavefront per pair), with the mate-link set
  unitigs_reads_sizes        THE YARDSTICK: k_th_reads once and the scan -- the same one walk with the same probes and no atomics
  unitigs_reads_device       k_th_reads twice and the scan between, with room for every segment
The tally is begun again before every timed add, outside the clock, so that every add does the same work on empty sets.  The split by
kernel comes from a kernel trace, which is a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_support.py ... --steps 1
What is found is held to the threading call: segments, live k-mers and linked transitions are those of its records.  No figure is a gate."""
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
ap.add_argument("--every", type=int, default=10, help="one transcript in this many carries an allele")
ap.add_argument("--capacity", type=int, default=1 << 24, help="the distinct entries each of the two sets may hold")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads - args.reads % 2
est = max(1 << 20, int(1.3 * 2250 * args.T + 0.07 * n * L))
prm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link)
room = dict(junction_capacity=args.capacity, mate_capacity=args.capacity)
res = {"metric": "sdt_gpu_unitigs_support_add_device beside sdt_gpu_unitigs_reads_device on the same reads, table, list and index (wall ms of the blocking "
                 "calls): medians after one warm-up",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "params": prm, "allele_every": args.every, "room": room}
med = lambda v: round(statistics.median(v), 3)

words, offsets, nwords, res["sites_planted"] = workload_with_alleles(n, L, args.T, dev, K, args.every, err=args.err)
torch.cuda.synchronize()
with pkg.PregraphGPU(K, est_distinct=est) as g:
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers"], res["nodes"] = g.finish_count()
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    res["library"] = os.path.basename(pkg.LIB_PATH)
    res["slots"] = int(g.table_slots())

    def wall(call, before=None):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return 1e3 * (time.perf_counter() - t0), out

    info = g.unitigs_begin(prm)
    res["info"] = [int(x) for x in info]
    g.unitigs_index()
    nu = int(info[2])
    d_rec = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_so = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    total = g.unitigs_reads_device(words, offsets, n, d_rec, d_so)
    d_segs = torch.zeros((max(total, 1), 6), dtype=torch.int32, device=dev)
    begin = lambda: g.unitigs_support_begin(room)
    calls = {"support_add_device": (lambda: g.unitigs_support_add_device(words, offsets, n, False), begin),
             "support_add_device_paired": (lambda: g.unitigs_support_add_device(words, offsets, n, True), begin),
             "unitigs_reads_sizes": (lambda: g.unitigs_reads_device(words, offsets, n, d_rec, d_so), None),
             "unitigs_reads_device": (lambda: g.unitigs_reads_device(words, offsets, n, d_rec, d_so, d_segs, total), None)}
    per = {name: [] for name in calls}
    for name, (call, before) in calls.items():               # warm-up
        res[name + "_first_ms"] = round(wall(call, before)[0], 3)
    for _ in range(args.steps):                              # alternating
        for name, (call, before) in calls.items():
            per[name].append(wall(call, before)[0])
    for name in calls:
        res[name + "_wall_ms"], res[name + "_ms"] = [round(x, 3) for x in per[name]], med(per[name])
    res["support_over_reads_sizes"] = round(res["support_add_device_ms"] / res["unitigs_reads_sizes_ms"], 3)
    res["support_paired_over_reads_sizes"] = round(res["support_add_device_paired_ms"] / res["unitigs_reads_sizes_ms"], 3)
    res["support_over_reads_device"] = round(res["support_add_device_ms"] / res["unitigs_reads_device_ms"], 3)
    res["reads_per_s"] = round(n / (res["support_add_device_ms"] * 1e-3))

    # what the last paired add left, against the records of the threading call
    totals = g.unitigs_support_totals()
    res["totals"] = dict(zip(pkg.SUPPORT_TOTALS, (int(x) for x in totals)))
    us = g.unitigs_support_unitigs(0, nu)
    ls = g.unitigs_support_links(0, nu)
    res["junctions"], res["mate_links"] = len(g.unitigs_support_junctions()), len(g.unitigs_support_mates())
    res["max_segs_of_a_unitig"], res["max_along_of_a_link"] = int(us["segs"].max()), int(ls["along"].max()) if len(ls) else 0
    rec = d_rec.cpu().numpy().view(np.uint32)
    segs = d_segs.cpu().numpy().view(np.uint32)[:total]
    res["same_segments"] = bool(int(totals[2]) == total == int(us["segs"].sum()))
    res["same_live"] = bool(int(totals[3]) == int(rec[:, 1].astype(np.int64).sum()) == int(us["kmers"].sum()))
    res["same_linked"] = bool(int(totals[4]) == int((segs[:, 1] >> 1 == 1).sum()) == int(ls["along"].sum()) + int(totals[5]))
    per_unitig = np.bincount(segs[:, 0], minlength=nu)
    res["same_segs_per_unitig"] = bool((per_unitig == us["segs"].astype(np.int64)).all())
    g.unitigs_support_end()
    g.unitigs_end()
    res["not_measured"] = ["key widths of 2 and 4 words", "the host form (staging)", "the command line", "reads longer than 150 bases",
                           "adds onto sets that are already filled (every timed add starts on empty sets)"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
