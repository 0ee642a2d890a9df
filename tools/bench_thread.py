#!/usr/bin/env python3
"""sdt_gpu_unitigs_index and sdt_gpu_unitigs_reads_device on a counted table beside sdt_gpu_cluster_reads_device on the same reads and
table, in one process and alternating: the library of tools/bench_unitigs.py (allele_workload.py: synth.torch_workload's transcriptome
and sampling, resident in HBM, with a substitution allele in the middle of every tenth transcript).
    python tools/bench_thread.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 5 --out profiles/unitig_thread/bench_thread_8M_T45000.json
Prints one JSON line.  Every figure is taken after one warm-up call and is the median of --steps (all of them are listed):
  unitigs_index          the wall clock around the blocking call (the memset of 8 B per slot, k_th_label, the wait for its counters)
  unitigs_reads_device   the wall clock around the blocking call with room for every segment: k_th_reads twice and the scan between
  unitigs_reads_sizes    the same without segments: k_th_reads once and the scan
  cluster_reads_device   the yardstick: one 16-byte probe and one 4-byte label load per k-mer, where threading makes one probe and one
                         8-byte label load per k-mer, twice over
The split by kernel comes from a kernel trace, which is a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_thread.py ... --steps 1
What is found is held to itself: the segments of every read sum to its live k-mers, the offsets are the prefix sums of the records'
segs, and the live k-mers are those that the clustering sees.  No figure is a gate."""
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
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
est = max(1 << 20, int(1.3 * 2250 * args.T + 0.07 * n * L))
prm = dict(min_count=args.min_count, max_count=args.max_count, min_link=args.min_link)
res = {"metric": "sdt_gpu_unitigs_index and sdt_gpu_unitigs_reads_device beside sdt_gpu_cluster_reads_device on the same reads and table (wall ms of the "
                 "blocking calls): medians after one warm-up",
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

    res["unitigs_begin_ms"], info = wall(lambda: g.unitigs_begin(prm))
    res["unitigs_begin_ms"] = round(res["unitigs_begin_ms"], 3)
    res["info"] = [int(x) for x in info]
    first_ms, iinfo = wall(g.unitigs_index)                  # warm-up
    res["unitigs_index_first_ms"] = round(first_ms, 3)
    per = [wall(g.unitigs_index)[0] for _ in range(args.steps)]
    res["unitigs_index_wall_ms"], res["unitigs_index_ms"] = [round(x, 3) for x in per], med(per)
    res["index_info"] = [int(x) for x in iinfo]
    cinfo = g.cluster_begin(prm)

    d_rec = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_so = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_crec = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    total = g.unitigs_reads_device(words, offsets, n, d_rec, d_so)
    d_segs = torch.zeros((max(total, 1), 6), dtype=torch.int32, device=dev)
    calls = {"unitigs_reads_device": lambda: g.unitigs_reads_device(words, offsets, n, d_rec, d_so, d_segs, total),
             "unitigs_reads_sizes": lambda: g.unitigs_reads_device(words, offsets, n, d_rec, d_so),
             "cluster_reads_device": lambda: g.cluster_reads_device(words, offsets, n, d_crec)}
    per = {name: [] for name in calls}
    for name, call in calls.items():                         # warm-up
        res[name + "_first_ms"] = round(wall(call)[0], 3)
    for _ in range(args.steps):                              # alternating
        for name, call in calls.items():
            per[name].append(wall(call)[0])
    for name in calls:
        res[name + "_wall_ms"], res[name + "_ms"] = [round(x, 3) for x in per[name]], med(per[name])
    res["unitigs_reads_over_cluster_reads"] = round(res["unitigs_reads_device_ms"] / res["cluster_reads_device_ms"], 3)
    res["unitigs_reads_sizes_over_cluster_reads"] = round(res["unitigs_reads_sizes_ms"] / res["cluster_reads_device_ms"], 3)
    res["reads_per_s"] = round(n / (res["unitigs_reads_device_ms"] * 1e-3))

    rec = d_rec.cpu().numpy().view(np.uint32)
    so = d_so.cpu().numpy().view(np.uint64)
    segs = d_segs.cpu().numpy().view(np.uint32)[:total]
    crec = d_crec.cpu().numpy().view(np.uint32)
    kmers, live, nsegs, breaks = (rec[:, j].astype(np.int64) for j in range(4))
    res["segments"] = int(total)
    res["offsets_are_prefix_sums"] = bool((np.diff(so.astype(np.int64)) == nsegs).all() and int(so[-1]) == total)
    upto = np.concatenate([[0], np.cumsum(segs[:, 4].astype(np.int64))])
    res["segments_sum_to_live"] = bool((upto[so[1:].astype(np.int64)] - upto[so[:-1].astype(np.int64)] == live).all())
    res["same_live_as_clustering"] = bool((crec[:, 1] == rec[:, 1]).all() and int(cinfo[0]) == int(iinfo[0]))
    join = segs[:, 1] >> 1
    res["linked"], res["unlinked"], res["after_gap"] = int((join == 1).sum()), int((join == 2).sum()), int((join == 0).sum())
    # a linked segment starts at the in end of its oriented unitig, and the one before it ends at the out end of its own
    unodes = g.unitigs_fetch(0, int(info[2]))[1]["nodes"].astype(np.int64)
    su, so_, sp, sk = segs[:, 0].astype(np.int64), (segs[:, 1] & 1).astype(np.int64), segs[:, 3].astype(np.int64), segs[:, 4].astype(np.int64)
    at = np.nonzero(join == 1)[0]
    res["linked_start_at_in_ends"] = bool((sp[at] == np.where(so_[at] == 0, 0, unodes[su[at]] - 1)).all())
    ends = sp[at - 1] + (sk[at - 1] - 1) * np.where(so_[at - 1] == 0, 1, -1)
    res["linked_leave_from_out_ends"] = bool((ends == np.where(so_[at - 1] == 0, unodes[su[at - 1]] - 1, 0)).all())
    res["placed"] = int((nsegs > 0).sum())
    res["whole"] = int(((nsegs > 0) & (live == kmers) & (breaks == 0)).sum())
    res["mean_segments_per_placed_read"] = round(float(nsegs[nsegs > 0].mean()), 3) if res["placed"] else 0
    res["max_segments"] = int(nsegs.max())
    g.cluster_end()
    g.unitigs_end()
    res["not_measured"] = ["key widths of 2 and 4 words", "the host form (staging and the copies back)", "the command line", "reads longer than 150 bases"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
