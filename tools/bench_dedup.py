#!/usr/bin/env python3
"""sdt_gpu_dedup_reads_device beside k_profile_reads on the same reads, on a synthetic workload that is resident in HBM
(torch_workload: the workload of DESIGN.md 4g), and on the same stream with every read present twice.
    python tools/bench_dedup.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call (HIP events inside the library around the fingerprints and the rounds, one warm-up call first), reads
per second, the reads kept, and the yardstick: the bytes the stage must move at the least -- the stream read twice (once for the
fingerprints, once for the comparison), the table once -- and the rate that they make of the time."""
import argparse
import json
import os
import sys

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
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert (n * L) % 16 == 0, "the doubled stream is made of whole words"
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
body = n * L // 16
words2 = torch.cat([words[:body], words[:body], torch.zeros(4, dtype=words.dtype, device=dev)])
offsets2 = torch.cat([offsets, offsets[1:] + n * L])
torch.cuda.synchronize()
res = {"metric": "sdt_gpu_dedup_reads_device beside k_profile_reads: ms per call", "reads": n, "read_len": L, "K": K, "T": args.T,
       "err": args.err, "steps": args.steps}


def slots_for(units):
    s = 2
    while s < 2 * units:
        s *= 2
    return s


with pkg.PregraphGPU(K, est_distinct=n * (L - K + 1)) as g:

    def timed(name, call):
        call()                                          # warm-up
        per = []
        for _ in range(args.steps):
            g.kernel_time(reset=True)
            call()
            per.append(g.kernel_time(reset=True)[0])
        res[name + "_ms"] = [round(x, 3) for x in per]
        return min(per)

    for name, w, o, m, paired in (("dedup", words, offsets, n, False), ("dedup_twice", words2, offsets2, 2 * n, False)):
        d_dup = torch.zeros((m, 2), dtype=torch.int64, device=dev)
        d_keep = torch.zeros((m,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        kept = []
        best = timed(name, lambda: kept.append(g.dedup_reads_device(w, o, m, d_dup, d_keep, paired=paired)))
        units = m // 2 if paired else m
        moved = 2 * (m * L // 4) + 24 * slots_for(units)                # the stream twice, the table once
        res.update({name + "_reads_per_s": round(m / (best * 1e-3)), name + "_kept": kept[-1], name + "_table_slots": slots_for(units),
                    name + "_yardstick_bytes": moved, name + "_yardstick_GB_per_s": round(moved / (best * 1e-3) / 1e9, 1)})
        del d_dup, d_keep
    # the yardstick of the other read stages: the profile of the same reads against their counted table
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers_counted"], res["nodes"] = g.finish_count()
    d_cov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prof = timed("k_profile_reads", lambda: g.profile_reads_device(words, offsets, n, L, 0, d_cov))
    res["dedup_over_profile"] = round(min(res["dedup_ms"]) / prof, 3)
print(json.dumps(res))
