#!/usr/bin/env python3
"""sdt_gpu_quality_reads_device beside sdt_gpu_clip_reads_device with one adapter and one sdt_gpu_complexity_reads_device on the same
reads, on a synthetic workload that is resident in HBM (torch_workload: the workload of DESIGN.md 4g) with one quality byte per base
(offset 33), drawn on the device from a fixed seed: a plateau of 30 .. 40 (less 6 to plus 2 per base) that falls to 2 .. 15 from a
random base on; in one read in seven the first 1 .. 7 bases have quality 2, in one read in eleven a run of 1 .. 9 bases inside has.
    python tools/bench_quality.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first), reads per second, the
reads by verdict, and the yardstick: the bytes the stage must move at the least -- the quality bytes read once, 8 B of offset read and
25 B written per read (the record and the keep byte) -- and the rate that they make of the time.  The records of every
--check-every-th read are held to the rule restated in numpy on the CPU (prefix sums and a running minimum, vectorised over reads of
one length).  The other two stages run in the same process on the same reads."""
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
ap.add_argument("--seed", type=int, default=20261019)
ap.add_argument("--check-every", type=int, default=16, help="one read in this many is held to the rule on the CPU")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert L > 20 and (n * L) % 4 == 0
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)

# the qualities, a million reads at a time; the sample's bytes go to the host
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=gen, device=dev, dtype=torch.int64)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
quals = torch.empty(n * L, dtype=torch.uint8, device=dev)
chunk = 1 << 20
assert chunk % args.check_every == 0
sample = []
for c0 in range(0, n, chunk):
    m = min(chunk, n - c0)
    i = torch.arange(c0, c0 + m, device=dev, dtype=torch.int64)[:, None]
    q = torch.where(col < ri(L // 3, L + 40, (m, 1)), ri(30, 41, (m, 1)) + ri(-6, 3, (m, L)), ri(2, 16, (m, L)))
    q = torch.where((i % 7 == 0) & (col < ri(1, 8, (m, 1))), torch.full_like(q, 2), q)
    at = ri(0, L - 10, (m, 1))
    q = torch.where((i % 11 == 0) & (col >= at) & (col < at + ri(1, 10, (m, 1))), torch.full_like(q, 2), q)
    q = (q.clamp(0, 41) + 33).to(torch.uint8)
    quals[c0 * L:(c0 + m) * L] = q.reshape(-1)
    sample.append(q[:: args.check_every].cpu().numpy())
    del q, at, i
torch.cuda.synchronize()
sample = np.concatenate(sample)
assert quals.data_ptr() % 4 == 0

params = dict(phred_offset=33, cut_q=20, low_q=15, max_low_pct=40, max_ee_ppm=0, min_len=0, flags=0, reserved=0)


def ee_table():
    """10^6 * 10^(-q / 10) rounded to the nearest integer, in exact integers"""
    top, out = (2 * 10 ** 6) ** 10, []
    for q in range(94):
        t = int(round(1e6 * 10 ** (-q / 10)))
        while (2 * t + 1) ** 10 * 10 ** q <= top:
            t += 1
        while t > 0 and (2 * t - 1) ** 10 * 10 ** q > top:
            t -= 1
        out.append(t)
    return np.array(out, dtype=np.int64)


def rule(c, p):
    """the rule of include/sdt_gpu.h for reads of one length, restated in numpy -> (span, low, ee_ppm, start, len, verdict) per read"""
    m, length = c.shape
    c = c.astype(np.int64)
    q = np.where(c < p["phred_offset"], 0, np.minimum(c - p["phred_offset"], 93))
    P = np.concatenate([np.zeros((m, 1), dtype=np.int64), np.cumsum(q - p["cut_q"], axis=1)], axis=1)
    M = np.minimum.accumulate(P, axis=1)
    idx = np.arange(length + 1)[None, :]
    new = np.concatenate([np.ones((m, 1), dtype=bool), P[:, 1:] < M[:, :-1]], axis=1)
    a_b = np.maximum.accumulate(np.where(new, idx, 0), axis=1)
    key = ((P - M) * (length + 1) + (length - a_b)) * (length + 1) + idx        # gain descending, a ascending, b descending
    b = key.argmax(axis=1)
    a = a_b[np.arange(m), b]
    inside = (idx[:, :-1] >= a[:, None]) & (idx[:, :-1] < b[:, None])
    span = b - a
    low = (inside & (q < p["low_q"])).sum(axis=1)
    ee = np.where(span > 0, (np.where(inside, ee_table()[q], 0)).sum(axis=1) // np.maximum(span, 1), 0)
    dropped = (span < max(p["min_len"], 1)) | (100 * low > p["max_low_pct"] * span) | ((p["max_ee_ppm"] != 0) & (ee > p["max_ee_ppm"]))
    rec = np.zeros(m, dtype=pkg.READ_QUALITY_DTYPE)
    rec["span"], rec["low"], rec["ee_ppm"] = span, low, ee
    rec["start"] = np.where(dropped | (span == length), 0, a)
    rec["len"] = np.where(dropped, 0, span)
    rec["verdict"] = np.where(dropped, 3, np.where(span == length, 0, 2))
    return rec


res = {"metric": "sdt_gpu_quality_reads_device beside sdt_gpu_clip_reads_device (one adapter) and sdt_gpu_complexity_reads_device: ms per call",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "seed": args.seed, "params": params}

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

    d_out = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    moved = n * L + 8 * n + 25 * n                         # the quality bytes once, 8 B of offset, 24 + 1 B written per read
    kept = []
    best = timed("quality", lambda: kept.append(g.quality_reads_device(quals, offsets, n, d_out, d_keep, params)))
    v = d_out[:, 5]
    res.update({"quality_reads_per_s": round(n / (best * 1e-3)), "quality_kept": kept[-1], "quality_whole": int((v == 0).sum()),
                "quality_clipped": int((v == 2).sum()), "quality_dropped": int((v == 3).sum()), "bases_in": n * L,
                "bases_out": int(d_out[:, 4].long().sum()), "quality_yardstick_bytes": moved,
                "quality_yardstick_GB_per_s": round(moved / (best * 1e-3) / 1e9, 1)})
    # the sample against the rule on the CPU
    got = d_out[:: args.check_every].cpu().numpy().view(np.uint8).copy().view(pkg.READ_QUALITY_DTYPE).reshape(-1)
    want = rule(sample, params)
    res.update({"sample_reads": len(sample), "sample_records_equal_the_rule": bool((got == want).all()),
                "sample_by_verdict": [[int((r["verdict"] == x).sum()) for x in (0, 2, 3)] for r in (got, want)]})
    del d_out
    # the yardsticks of the stages next to it, in the same run on the same reads: the clip with one adapter and one complexity filter
    rng = np.random.default_rng(33)
    aset = pkg.pack_adapters([(rng.integers(0, 4, size=33, dtype=np.uint8), 0)])
    d_clip = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    clip = timed("clip_1", lambda: g.clip_reads_device(words, offsets, n, d_clip, d_keep, aset,
                                                       dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=1,
                                                            tail5_bases=4, flags=0)))
    torch.cuda.synchronize()
    cx = timed("complexity", lambda: g.complexity_reads_device(words, offsets, n, d_clip, d_keep, dict(max_score_pct=10, max_low_pct=50, min_len=0, flags=0)))
    res["quality_over_clip_1"] = round(best / clip, 3)
    res["quality_over_complexity"] = round(best / cx, 3)
    res["not_measured"] = ["the host form", "long reads", "the command line"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
