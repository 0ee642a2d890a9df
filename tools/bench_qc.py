#!/usr/bin/env python3
"""sdt_gpu_qc_reads_device with qualities at --cycles 150 and 1024, beside one sdt_gpu_quality_reads_device and one
sdt_gpu_clip_reads_device with one adapter on the same reads, in one process: the workload of tools/bench_quality.py (torch_workload,
resident in HBM; one quality byte per base at offset 33, drawn on the device from the same seed).
    python tools/bench_qc.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4 --out profiles/read_qc/bench_qc_4M_T2000.json
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first, the best of --steps), and
the bar: the QC report at 150 cycles over the quality stage, 2 at most.  The quality stage and the clip are existing code: they are the
yardstick.  The report of every --check-every-th read (a call of its own, which picks them by a class byte) is held to the rule
restated in numpy on the CPU, in both directions."""
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
ap.add_argument("--cycles", type=int, nargs="+", default=[150, 1024], help="the first is the one the bar is about")
ap.add_argument("--check-every", type=int, default=16, help="one read in this many is held to the rule on the CPU")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert L > 20 and (n * L) % 4 == 0
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)

# the qualities of tools/bench_quality.py, a million reads at a time; the sample's bytes go to the host
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=gen, device=dev, dtype=torch.int64)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
quals = torch.empty(n * L, dtype=torch.uint8, device=dev)
chunk = 1 << 20
assert chunk % args.check_every == 0
sample_q = []
for c0 in range(0, n, chunk):
    m = min(chunk, n - c0)
    i = torch.arange(c0, c0 + m, device=dev, dtype=torch.int64)[:, None]
    q = torch.where(col < ri(L // 3, L + 40, (m, 1)), ri(30, 41, (m, 1)) + ri(-6, 3, (m, L)), ri(2, 16, (m, L)))
    q = torch.where((i % 7 == 0) & (col < ri(1, 8, (m, 1))), torch.full_like(q, 2), q)
    at = ri(0, L - 10, (m, 1))
    q = torch.where((i % 11 == 0) & (col >= at) & (col < at + ri(1, 10, (m, 1))), torch.full_like(q, 2), q)
    q = (q.clamp(0, 41) + 33).to(torch.uint8)
    quals[c0 * L:(c0 + m) * L] = q.reshape(-1)
    sample_q.append(q[:: args.check_every].cpu().numpy())
    del q, at, i
torch.cuda.synchronize()
sample_q = np.concatenate(sample_q).astype(np.int64) - 33
assert quals.data_ptr() % 4 == 0
# the sample's bases, unpacked from the words on the host
host_words = words.cpu().numpy().view(np.uint32)
idx = (np.arange(0, n, args.check_every, dtype=np.int64) * L)[:, None] + np.arange(L, dtype=np.int64)[None, :]
sample_b = ((host_words[idx >> 4] >> (30 - 2 * (idx & 15)).astype(np.uint32)) & 3).astype(np.int64)
del host_words, idx
classes = torch.zeros(n, dtype=torch.uint8, device=dev)
classes[:: args.check_every] = 1


def rule(C, from_end):
    """the report of the sample by the rule of include/sdt_gpu.h: reads of one length L, all counted, qualities 0 .. 41"""
    m = len(sample_b)
    rep = np.zeros(pkg.QC_TOTALS + 99 * (C + 1) + pkg.QC_GC_BINS + pkg.QC_QUALS, dtype=np.uint64)
    s = {k: v for k, v in zip(("totals", "base", "qual", "len", "gc", "meanq"),
                              np.split(rep, np.cumsum([8, 4 * (C + 1), 94 * (C + 1), C + 1, 101])))}
    base, qual = s["base"].reshape(C + 1, 4), s["qual"].reshape(C + 1, 94)
    s["totals"][0], s["totals"][2], s["totals"][3] = m, m * L, n - m
    for i in range(L):
        row = min(L - 1 - i if from_end else i, C)
        base[row] += np.bincount(sample_b[:, i], minlength=4).astype(np.uint64)
        qual[row] += np.bincount(sample_q[:, i], minlength=94).astype(np.uint64)
    s["len"][min(L, C)] = m
    s["gc"] += np.bincount(100 * (sample_b & 1).sum(axis=1) // L, minlength=101).astype(np.uint64)
    s["meanq"] += np.bincount(sample_q.sum(axis=1) // L, minlength=94).astype(np.uint64)
    return rep


res = {"metric": "sdt_gpu_qc_reads_device with qualities beside sdt_gpu_quality_reads_device and sdt_gpu_clip_reads_device (one adapter): ms per call",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "seed": args.seed, "tile": pkg.QC_TILE}

with pkg.PregraphGPU(K, est_distinct=1 << 16) as g:
    res["library"] = os.path.basename(pkg.LIB_PATH)      # (SDT_GPU_LIB: an A/B build)

    def timed(name, call):
        call()                                          # warm-up
        per = []
        for _ in range(args.steps):
            g.kernel_time(reset=True)
            call()
            per.append(g.kernel_time(reset=True)[0])
        res[name + "_ms"] = [round(x, 3) for x in per]
        return min(per)

    best = {}
    for C in args.cycles:
        d_rep = torch.zeros(pkg.qc_report_words(C), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        best[C] = timed(f"qc_{C}", lambda: g.qc_reads_device(words, offsets, n, d_rep, quals, None, None, dict(cycles=C)))
        res[f"qc_{C}_bases_per_s"] = round(n * L / (best[C] * 1e-3))
        calls = args.steps + 1
        tot = d_rep[:8].cpu().numpy()
        res[f"qc_{C}_totals_per_call"] = [int(x) // calls for x in tot[:5]]
        assert tot[0] == calls * n and tot[2] == calls * n * L, tot
    # every check-every-th read, picked by its class byte, against the rule on the CPU
    same = []
    for C in args.cycles:
        for flags in (0, pkg.QC_FROM_END):
            d_rep = torch.zeros(pkg.qc_report_words(C), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            g.qc_reads_device(words, offsets, n, d_rep, quals, None, classes, dict(cycles=C, flags=flags, class_sel=1))
            same.append(bool((d_rep.cpu().numpy().view(np.uint64) == rule(C, bool(flags))).all()))
    res.update({"sample_reads": len(sample_b), "sample_reports_equal_the_rule": same})
    # the yardsticks, in the same run on the same reads
    d_out = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    quality = timed("quality", lambda: g.quality_reads_device(quals, offsets, n, d_out, d_keep,
                                                              dict(phred_offset=33, cut_q=20, low_q=15, max_low_pct=40, max_ee_ppm=0, min_len=0, flags=0, reserved=0)))
    rng = np.random.default_rng(33)
    aset = pkg.pack_adapters([(rng.integers(0, 4, size=33, dtype=np.uint8), 0)])
    clip = timed("clip_1", lambda: g.clip_reads_device(words, offsets, n, d_out, d_keep, aset,
                                                       dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=1,
                                                            tail5_bases=4, flags=0)))
    first = args.cycles[0]
    res.update({f"qc_{C}_over_quality": round(best[C] / quality, 3) for C in args.cycles})
    res.update({f"qc_{C}_over_clip_1": round(best[C] / clip, 3) for C in args.cycles})
    res["bar"] = f"qc_{first}_over_quality <= 2"
    res["under_the_bar"] = bool(best[first] <= 2 * quality)
    res["not_measured"] = ["the host form", "the command line", "long reads", "a FASTA-only batch (no qualities)"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
