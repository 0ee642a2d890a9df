#!/usr/bin/env python3
"""sdt_gpu_complexity_reads_device beside sdt_gpu_clip_reads_device with one adapter and one sdt_gpu_dedup_reads_device on the same
reads, on a synthetic workload that is resident in HBM (torch_workload: the workload of DESIGN.md 4g) into which, in one read in ten,
a run of 30 .. 150 bases is planted at a random position: poly-A, poly-G (what a run of N becomes) or (AC)n, a third each.
    python tools/bench_complexity.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first), reads per second, the
reads by verdict, the planted reads that were found (a LOW window) and the unplanted reads that were flagged, and the yardstick: the
bytes the stage must move at the least -- the stream read once and 25 B written per read (the record and the keep byte) -- and the
rate that they make of the time.  The records of every --check-every-th read are held to the rule restated in numpy on the CPU
(triplet counts per window, vectorised over reads of one length), and the two counts are given for that sample from both sides.  The
other two stages run in the same process on the same reads."""
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
ap.add_argument("--run-every", type=int, default=10, help="one read in this many carries a planted run")
ap.add_argument("--check-every", type=int, default=16, help="one read in this many is held to the rule on the CPU")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert L > 64
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)

# the runs into the packed stream, a million reads at a time (a chunk starts on a word boundary); the sample's bases go to the host
shifts = 30 - 2 * torch.arange(16, device=dev, dtype=torch.int64)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
chunk = 1 << 20
assert (chunk * L) % 16 == 0 and chunk % args.check_every == 0
sample = []
for c0 in range(0, n, chunk):
    m = min(chunk, n - c0)
    w0, w1 = c0 * L // 16, ((c0 + m) * L + 15) // 16
    w = words[w0:w1].long() & 0xFFFFFFFF
    codes = ((w[:, None] >> shifts[None, :]) & 3).reshape(-1)[: m * L].reshape(m, L)
    i = torch.arange(c0, c0 + m, device=dev, dtype=torch.int64)
    run = (30 + (i * 2654435761 >> 7) % (min(L, 150) - 29))[:, None]       # 30 .. 150 bases
    at = ((i * 40503 >> 3) % (L - run[:, 0] + 1))[:, None]
    kind = ((i // args.run_every) % 3)[:, None]
    value = torch.where(kind == 0, torch.zeros_like(codes), torch.where(kind == 1, torch.full_like(codes, 3), (col - at) & 1))
    codes = torch.where((i % args.run_every == 0)[:, None] & (col >= at) & (col < at + run), value, codes)
    sample.append(codes[:: args.check_every].to(torch.uint8).cpu().numpy())
    flat = codes.reshape(-1)
    pad = (-flat.numel()) % 16
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64, device=dev)])
    w = (flat.view(-1, 16) << shifts).sum(dim=1)
    words[w0:w1] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    del w, codes, flat, value
torch.cuda.synchronize()
sample = np.concatenate(sample)
planted = torch.arange(n, device=dev) % args.run_every == 0

params = dict(max_score_pct=10, max_low_pct=50, min_len=0, flags=0)


def rule(reads, p):
    """the rule of include/sdt_gpu.h for reads of one length, restated in numpy -> (windows, low, score, start, len, verdict) per read"""
    m, length = reads.shape
    W = max(1, -(-length // 32) - 1)
    r = reads.astype(np.int64)
    low_base = np.zeros((m, length), dtype=bool)
    nlow, score = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for j in range(W):
        b, e = 32 * j, min(32 * j + 64, length)
        l = e - b - 2
        if l < 2:
            continue
        t = 16 * r[:, b:e - 2] + 4 * r[:, b + 1:e - 1] + r[:, b + 2:e]
        c = np.bincount((t + 64 * np.arange(m)[:, None]).reshape(-1), minlength=64 * m).reshape(m, 64)
        D = (c * (c - 1)).sum(axis=1)
        score = np.maximum(score, 100 * D // (l * (l - 1)))
        is_low = 100 * D >= p["max_score_pct"] * l * (l - 1)
        nlow += is_low
        low_base[:, b:e] |= is_low[:, None]
    ln = np.where(100 * low_base.sum(axis=1) > p["max_low_pct"] * length, 0, length)
    dropped = ln < max(p["min_len"], 1)
    rec = np.zeros(m, dtype=pkg.READ_COMPLEXITY_DTYPE)
    rec["windows"], rec["low"], rec["score"], rec["len"], rec["verdict"] = W, nlow, score, np.where(dropped, 0, ln), np.where(dropped, 3, 0)
    return rec


res = {"metric": "sdt_gpu_complexity_reads_device beside sdt_gpu_clip_reads_device (one adapter) and sdt_gpu_dedup_reads_device: ms per call",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "run_share": round(1 / args.run_every, 4),
       "params": params}

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

    d_cx = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    moved = n * L // 4 + 25 * n                            # the stream once, 24 + 1 B written per read
    kept = []
    best = timed("complexity", lambda: kept.append(g.complexity_reads_device(words, offsets, n, d_cx, d_keep, params)))
    v, low = d_cx[:, 5], d_cx[:, 1] > 0
    res.update({"complexity_reads_per_s": round(n / (best * 1e-3)), "complexity_kept": kept[-1], "complexity_whole": int((v == 0).sum()),
                "complexity_dropped": int((v == 3).sum()), "planted_reads": int(planted.sum()), "planted_found": int((low & planted).sum()),
                "planted_dropped": int(((v == 3) & planted).sum()), "unplanted_flagged": int((low & ~planted).sum()),
                "unplanted_dropped": int(((v == 3) & ~planted).sum()), "complexity_yardstick_bytes": moved,
                "complexity_yardstick_GB_per_s": round(moved / (best * 1e-3) / 1e9, 1)})
    # the sample against the rule on the CPU
    got = d_cx[:: args.check_every].cpu().numpy().view(np.uint8).copy().view(pkg.READ_COMPLEXITY_DTYPE).reshape(-1)
    want = rule(sample, params)
    is_planted = (np.arange(len(sample)) * args.check_every) % args.run_every == 0
    res.update({"sample_reads": len(sample), "sample_records_equal_the_rule": bool((got == want).all()),
                "sample_planted_found": [int(((got["low"] > 0) & is_planted).sum()), int(((want["low"] > 0) & is_planted).sum())],
                "sample_unplanted_flagged": [int(((got["low"] > 0) & ~is_planted).sum()), int(((want["low"] > 0) & ~is_planted).sum())]})
    del d_cx
    # the yardsticks of the stages next to it, in the same run on the same reads: the clip with one adapter and one dedup
    rng = np.random.default_rng(33)
    aset = pkg.pack_adapters([(rng.integers(0, 4, size=33, dtype=np.uint8), 0)])
    d_clip = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    clip = timed("clip_1", lambda: g.clip_reads_device(words, offsets, n, d_clip, d_keep, aset,
                                                       dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=1,
                                                            tail5_bases=4, flags=0)))
    del d_clip
    d_dup = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dedup = timed("dedup", lambda: g.dedup_reads_device(words, offsets, n, d_dup, d_keep))
    res["complexity_over_clip_1"] = round(best / clip, 3)
    res["complexity_over_dedup"] = round(best / dedup, 3)
    res["not_measured"] = ["the kept form", "the host form", "long reads", "a stream that is mostly low"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
