#!/usr/bin/env python3
"""sdt_gpu_overlap_pairs_device beside sdt_gpu_clip_reads_device (one adapter) and sdt_gpu_dedup_reads_device on the same reads, on a
synthetic workload that is resident in HBM (torch_workload: the workload of DESIGN.md 4g), taken as pairs: reads 2t and 2t + 1 are
mates.  One pair in ten is a read-through pair: a fragment of 86 .. 145 bases (the first bases of mate 1), on either mate a 33-base
adapter and random bases behind it.  One pair in ten is a fragment of 160 .. 270 bases read from both ends: the mates overlap by
30 .. 140 bases, nothing is cut.  The rest are the workload's reads as they are: unrelated mates.
    python tools/bench_overlap.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first), pairs per second, the
pairs found and the reads by verdict, and the yardstick of DESIGN.md 4l: the bytes the stage must move at the least -- the stream read
once and 25 B written per read (the record and the keep byte) -- and the rate that they make of the time.  The other two stages run
in the same process on the same reads, as the parent commit has them."""
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
ap.add_argument("--through-every", type=int, default=10, help="one pair in this many is a read-through pair")
ap.add_argument("--meet-every", type=int, default=10, help="one pair in this many overlaps without a base to cut")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
assert L == 150 and n % 2 == 0, "the fragment lengths of the workload are those of 150-base reads"
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
rng = np.random.default_rng(34)
ad1 = torch.from_numpy(rng.integers(0, 4, size=33, dtype=np.uint8)).to(dev).long()
ad2 = torch.from_numpy(rng.integers(0, 4, size=33, dtype=np.uint8)).to(dev).long()
gen = torch.Generator(device=dev)
gen.manual_seed(34)

# the fragments into the packed stream, a million reads at a time (a chunk starts on a word boundary and holds whole pairs)
shifts = 30 - 2 * torch.arange(16, device=dev, dtype=torch.int64)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
chunk = 1 << 20
assert (chunk * L) % 16 == 0
for c0 in range(0, n, chunk):
    m = min(chunk, n - c0)
    w0, w1 = c0 * L // 16, ((c0 + m) * L + 15) // 16
    w = words[w0:w1].long() & 0xFFFFFFFF
    codes = ((w[:, None] >> shifts[None, :]) & 3).reshape(-1)[: m * L].reshape(m // 2, 2, L)
    a, b = codes[:, 0, :], codes[:, 1, :]
    t = torch.arange(c0 // 2, (c0 + m) // 2, device=dev, dtype=torch.int64)
    junk = torch.randint(0, 4, (m // 2, L), device=dev, dtype=torch.int64, generator=gen)
    # a read-through pair: b = the reverse complement of a[0, F), then on either mate the adapter and random bases
    F = (86 + (t * 2654435761 >> 7) % 60)[:, None]
    through = (t % args.through_every == 0)[:, None]
    behind = col >= F + 33
    rc = torch.gather(a, 1, (F - 1 - col).clamp(0, L - 1)) ^ 2
    new_a = torch.where(col < F, a, torch.where(behind, junk, ad1[(col - F).clamp(0, 32)]))
    new_b = torch.where(col < F, rc, torch.where(behind, junk.flip(1), ad2[(col - F).clamp(0, 32)]))
    # a fragment of F2 >= 160 bases read from both ends: b' = a[F2 - L, L) and random bases behind it; b[j] = b'[L - 1 - j] ^ 2
    F2 = (160 + (t * 40503 >> 5) % 111)[:, None]
    meet = (t % args.meet_every == args.meet_every // 2)[:, None]
    q = L - 1 - col
    bp = torch.where(q < 2 * L - F2, torch.gather(a, 1, (F2 - L + q).clamp(0, L - 1)), junk)
    a_out = torch.where(through, new_a, a)
    b_out = torch.where(through, new_b, torch.where(meet, bp ^ 2, b))
    flat = torch.stack([a_out, b_out], dim=1).reshape(-1)
    pad = (-flat.numel()) % 16
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64, device=dev)])
    w = (flat.view(-1, 16) << shifts).sum(dim=1)
    words[w0:w1] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    del w, codes, flat, junk, rc, bp, new_a, new_b, a_out, b_out
torch.cuda.synchronize()

res = {"metric": "sdt_gpu_overlap_pairs_device beside sdt_gpu_clip_reads_device (1 adapter) and sdt_gpu_dedup_reads_device: ms per call", "reads": n,
       "pairs": n // 2, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "through_share": round(1 / args.through_every, 4),
       "meet_share": round(1 / args.meet_every, 4)}
params = dict(min_overlap=30, max_err_pct=10, min_len=0, flags=0)
res["params"] = params

with pkg.PregraphGPU(K, est_distinct=1 << 20) as g:

    def timed(name, call):
        call()                                          # warm-up
        per = []
        for _ in range(args.steps):
            g.kernel_time(reset=True)
            call()
            per.append(g.kernel_time(reset=True)[0])
        res[name + "_ms"] = [round(x, 3) for x in per]
        return min(per)

    d_ov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    moved = n * L // 4 + 25 * n                            # the stream once, 24 + 1 B written per read
    kept = []
    best = timed("overlap", lambda: kept.append(g.overlap_pairs_device(words, offsets, n, d_ov, d_keep, params)))
    v, ins = d_ov[:, 5], d_ov[0::2, 2]
    res.update({"overlap_pairs_per_s": round(n // 2 / (best * 1e-3)), "overlap_reads_per_s": round(n / (best * 1e-3)), "overlap_kept": kept[-1],
                "overlap_whole": int((v == 0).sum()), "overlap_clipped": int((v == 2).sum()), "overlap_dropped": int((v == 3).sum()),
                "pairs_overlapping": int((ins > 0).sum()), "pairs_read_through": int(((ins > 0) & (ins < L)).sum()),
                "median_insert": int(ins[ins > 0].float().median()) if int((ins > 0).sum()) else 0,
                "overlap_yardstick_bytes": moved, "overlap_yardstick_GB_per_s": round(moved / (best * 1e-3) / 1e9, 1)})
    del d_ov
    # the parent commit's stages, in the same run on the same reads: the clip with one adapter (the planted one of mate 1), and one dedup
    d_clip = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    aset = pkg.pack_adapters([(ad1.cpu().numpy().astype(np.uint8), 0)])
    cparams = dict(min_overlap=5, max_err_pct=10, min_len=0, min_tail=10, tail_err_pct=20, tail3_bases=1, tail5_bases=4, flags=0)
    clip = timed("clip_1", lambda: g.clip_reads_device(words, offsets, n, d_clip, d_keep, aset, cparams))
    res["clip_1_by_planted_adapter"] = int(((d_clip[:, 0] & 0xFFFF) == 1).sum())
    del d_clip
    d_dup = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dedup = timed("dedup", lambda: g.dedup_reads_device(words, offsets, n, d_dup, d_keep))
    res["overlap_over_clip_1"] = round(best / clip, 3)
    res["overlap_over_dedup"] = round(best / dedup, 3)
print(json.dumps(res))
