#!/usr/bin/env python3
"""k_trim_reads (flag off and on) beside k_profile_reads and k_correct_reads on the same reads and the same table, and the ranged
compaction, on a synthetic workload that is resident in HBM (torch_workload, counted by pass 1 on the device: the workload of
DESIGN.md 4g).
    python tools/bench_trim.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call of each kernel (HIP events inside the library, one warm-up call first), k-mers/s, the ratio to the
profile kernel, the verdict counts, and the compaction's wall clock per call with the bytes it moves."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
from soapdenovo_trans_amd import synth  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--K", type=int, default=31)
ap.add_argument("--T", type=int, default=2000)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--min-count", type=int, default=2)
ap.add_argument("--min-len", type=int, default=0)
ap.add_argument("--est-distinct", type=int, default=0, help="default: one slot estimate per k-mer occurrence, as the run of DESIGN.md 4g")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
kmers = n * (L - K + 1)
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
torch.cuda.synchronize()
res = {"metric": "k_trim_reads beside k_profile_reads: ms per call", "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err,
       "kmers": kmers, "min_count": args.min_count, "min_len": args.min_len, "steps": args.steps}
with pkg.PregraphGPU(K, est_distinct=args.est_distinct or kmers) as g:
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers_counted"], res["nodes"] = g.finish_count()
    res["table_slots"] = g.table_slots() if hasattr(g, "table_slots") else None
    d_cov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_fix = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    d_trim = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(name, call):
        call()                                          # warm-up (the first profile of a table state also scans aux once)
        per = []
        for _ in range(args.steps):
            g.kernel_time(reset=True)
            call()
            per.append(g.kernel_time(reset=True)[0])
        res[name + "_ms"] = [round(x, 3) for x in per]
        return min(per)

    prof = timed("k_profile_reads", lambda: g.profile_reads_device(words, offsets, n, L, args.min_count, d_cov))
    corr = timed("k_correct_reads", lambda: g.correct_reads_device(words, nwords, offsets, n, L, args.min_count, d_fix))
    off = timed("k_trim_reads", lambda: g.trim_reads_device(words, offsets, n, L, d_trim, d_keep, args.min_count, 0, args.min_len, 0))
    verdicts_off = torch.bincount(d_trim[:, 5], minlength=5).tolist()
    on = timed("k_trim_reads_corrected", lambda: g.trim_reads_device(words, offsets, n, L, d_trim, d_keep, args.min_count, 0, args.min_len,
                                                                     pkg.TRIM_CORRECTED))
    verdicts_on = torch.bincount(d_trim[:, 5], minlength=5).tolist()
    fix = d_fix.cpu().numpy()
    res.update({"profile_kmers_per_s": round(kmers / (prof * 1e-3)), "trim_kmers_per_s": round(kmers / (off * 1e-3)),
                "trim_corrected_kmers_per_s": round(kmers / (on * 1e-3)), "trim_over_profile": round(off / prof, 3),
                "trim_corrected_over_profile": round(on / prof, 3), "correct_over_profile": round(corr / prof, 3),
                "trim_corrected_over_correct": round(on / corr, 3), "runs": int(fix[:, 2].sum()), "weak_kmers": int(fix[:, 1].sum()),
                "fixed": int(fix[:, 3].sum()), "verdicts_whole_gated_trimmed_dropped_short": verdicts_off,
                "verdicts_corrected": verdicts_on})
    # the ranged compaction of the records of the last call (wall clock: two scans, the placement, the word kernel, four allocations)
    d_ow = torch.zeros((nwords,), dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    nr, nw = g.compact_trimmed_device(words, offsets, n, d_trim, d_ow, nwords, d_oo)
    per = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.time()
        g.compact_trimmed_device(words, offsets, n, d_trim, d_ow, nwords, d_oo)
        per.append((time.time() - t0) * 1e3)
    moved = 4 * (nwords + nw) + 24 * n + 8 * n + 3 * 8 * n + 8 * nr     # words in and out, records, offsets, the three work arrays, new offsets
    res.update({"compact_trimmed_ms": [round(x, 3) for x in per], "compact_out_reads": nr, "compact_out_words": nw,
                "compact_bytes_moved_estimate": moved, "compact_GB_per_s": round(moved / (min(per) * 1e-3) / 1e9, 1)})
print(json.dumps(res))
