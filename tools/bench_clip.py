#!/usr/bin/env python3
"""sdt_gpu_clip_reads_device beside k_profile_reads and sdt_gpu_dedup_reads_device on the same reads, on a synthetic workload that is
resident in HBM (torch_workload: the workload of DESIGN.md 4g) into which a 33-base adapter is read through in a share of the reads
(the fragment ends 5 .. 64 bases before the read does) and an A tail of 10 .. 39 bases is put at the end of another share.
    python tools/bench_clip.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: per adapter set (1, 6 and 64 adapters; the planted one is the first of each) ms per call (HIP events inside the
library around the kernel, one warm-up call first), reads per second, the reads by verdict, and the yardstick: the bytes the stage
must move at the least -- the stream read once and 25 B written per read (the record and the keep byte) -- and the rate that they
make of the time.  The other two stages run in the same process on the same reads."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
from soapdenovo_trans_amd import synth  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--K", type=int, default=31)
ap.add_argument("--T", type=int, default=2000)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--adapter-every", type=int, default=10, help="one read in this many carries the read-through adapter")
ap.add_argument("--tail-every", type=int, default=10, help="one read in this many carries an A tail")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert L > 64
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
rng = np.random.default_rng(33)
sets = {m: [(rng.integers(0, 4, size=33 if i == 0 else int(rng.integers(30, 61)), dtype=np.uint8), 0 if i == 0 or i % 3 else 1) for i in range(m)]
        for m in (1, 6, 64)}
planted = sets[1][0][0]
for m in (6, 64):
    sets[m][0] = (planted, 0)

# the adapter and the tails into the packed stream, a million reads at a time (a chunk starts on a word boundary)
shifts = 30 - 2 * torch.arange(16, device=dev, dtype=torch.int64)
ad = torch.from_numpy(planted).to(dev)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
chunk = 1 << 20
assert (chunk * L) % 16 == 0
for c0 in range(0, n, chunk):
    m = min(chunk, n - c0)
    w0, w1 = c0 * L // 16, ((c0 + m) * L + 15) // 16
    w = words[w0:w1].long() & 0xFFFFFFFF
    codes = ((w[:, None] >> shifts[None, :]) & 3).reshape(-1)[: m * L].reshape(m, L)
    i = torch.arange(c0, c0 + m, device=dev, dtype=torch.int64)
    through = (5 + (i * 2654435761 >> 7) % 60)[:, None]                   # bases of the read behind the fragment's end
    k = col - (L - through)
    codes = torch.where((i % args.adapter_every == 0)[:, None] & (k >= 0) & (k < 33), ad[k.clamp(0, 32)].long(), codes)
    tail = (10 + (i * 40503 >> 5) % 30)[:, None]
    codes = torch.where((i % args.tail_every == args.tail_every // 2)[:, None] & (col >= L - tail), torch.zeros_like(codes), codes)
    flat = codes.reshape(-1)
    pad = (-flat.numel()) % 16
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64, device=dev)])
    w = (flat.view(-1, 16) << shifts).sum(dim=1)
    words[w0:w1] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    del w, codes, flat, k
torch.cuda.synchronize()

res = {"metric": "sdt_gpu_clip_reads_device beside k_profile_reads and sdt_gpu_dedup_reads_device: ms per call", "reads": n, "read_len": L, "K": K,
       "T": args.T, "err": args.err, "steps": args.steps, "adapter_share": round(1 / args.adapter_every, 4), "tail_share": round(1 / args.tail_every, 4)}
params = dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=1, tail5_bases=4, flags=0)
res["params"] = params

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

    d_clip = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    moved = n * L // 4 + 25 * n                            # the stream once, 24 + 1 B written per read
    for m, adapters in sets.items():
        name = f"clip_{m}"
        aset = pkg.pack_adapters(adapters)
        kept = []
        best = timed(name, lambda: kept.append(g.clip_reads_device(words, offsets, n, d_clip, d_keep, aset, params)))
        v = d_clip[:, 5]
        res.update({name + "_reads_per_s": round(n / (best * 1e-3)), name + "_kept": kept[-1], name + "_whole": int((v == 0).sum()),
                    name + "_clipped": int((v == 2).sum()), name + "_dropped": int((v == 3).sum()),
                    name + "_by_planted_adapter": int(((d_clip[:, 0] & 0xFFFF) == 1).sum()), name + "_tails3": int((d_clip[:, 1] > 0).sum()),
                    name + "_yardstick_bytes": moved, name + "_yardstick_GB_per_s": round(moved / (best * 1e-3) / 1e9, 1)})
    res["clip_64_over_clip_6"] = round(min(res["clip_64_ms"]) / min(res["clip_6_ms"]), 3)
    del d_clip, d_keep
    # the yardsticks of the parent commit's stages, in the same run on the same reads: one dedup, and the profile against the counted table
    d_dup = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dedup = timed("dedup", lambda: g.dedup_reads_device(words, offsets, n, d_dup, d_keep))
    del d_dup, d_keep
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers_counted"], res["nodes"] = g.finish_count()
    d_cov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prof = timed("k_profile_reads", lambda: g.profile_reads_device(words, offsets, n, L, 0, d_cov))
    for m in sets:
        res[f"clip_{m}_over_profile"] = round(min(res[f"clip_{m}_ms"]) / prof, 3)
        res[f"clip_{m}_over_dedup"] = round(min(res[f"clip_{m}_ms"]) / dedup, 3)
print(json.dumps(res))
