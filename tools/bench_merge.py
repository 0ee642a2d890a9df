#!/usr/bin/env python3
"""sdt_gpu_merge_pairs_device, without qualities and with them, beside sdt_gpu_overlap_pairs_device and
sdt_gpu_compact_trimmed_device on the same pairs, resident in HBM: pairs of 2 x 150 bases read from both ends of random fragments of
120 .. 400 bases (uniform), random bases past a fragment's end, substitution errors at --err per base, random quality bytes.  Most
pairs overlap: every fragment of up to 270 bases under min_overlap 30.
    python tools/bench_merge.py --pairs 4000000 --steps 5
Prints one JSON line.  Per call: the wall clock around the call, which ends in a synchronise (`*_wall_ms`: one warm-up call, then
--steps calls; the figures use their median), and the HIP events inside the library around the stage's own kernel (`*_kernel_ms`;
the compaction has none).  The yardstick of the merge: the bytes it must move -- the stream read once, 24 B read and 24 B written
per read for the two kinds of records, and each merged base written to the scratch stream, read from it and written to the dense
stream (3 x 2 bits) -- and the rate that they make of the wall time.  The other two calls run in the same process on the same pairs,
as the parent commit has them; the compaction runs on the overlap records (it moves the bases that the overlap keeps)."""
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
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4_000_000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--err", type=float, default=0.005)
ap.add_argument("--frag-min", type=int, default=120)
ap.add_argument("--frag-max", type=int, default=400)
args = ap.parse_args()

dev = torch.device("cuda:0")
L, P = 150, args.pairs
n = 2 * P
gen = torch.Generator(device=dev)
gen.manual_seed(35)
nwords = (n * L + 15) // 16 + 4
words = torch.zeros((nwords,), dtype=torch.int32, device=dev)
offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
shifts = 30 - 2 * torch.arange(16, device=dev, dtype=torch.int64)
col = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
chunk = 1 << 18                                           # pairs at a time; a chunk starts on a word boundary
assert (chunk * 2 * L) % 16 == 0
rnd = lambda shape, hi=4: torch.randint(0, hi, shape, device=dev, dtype=torch.int64, generator=gen)
for c0 in range(0, P, chunk):
    m = min(chunk, P - c0)
    F = torch.randint(args.frag_min, args.frag_max + 1, (m, 1), device=dev, dtype=torch.int64, generator=gen)
    frag = rnd((m, args.frag_max))
    a = torch.where(col < F, frag[:, :L], rnd((m, L)))
    b = torch.where(col < F, torch.gather(frag, 1, (F - 1 - col).clamp(0, args.frag_max - 1)) ^ 2, rnd((m, L)))     # b[j] = frag[F - 1 - j] ^ 2
    for x in (a, b):
        hit = torch.rand((m, L), device=dev, generator=gen) < args.err
        x[hit] = (x[hit] + 1 + rnd((int(hit.sum()),), 3)) & 3
    flat = torch.stack([a, b], dim=1).reshape(-1)
    pad = (-flat.numel()) % 16
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64, device=dev)])
    w = (flat.view(-1, 16) << shifts).sum(dim=1)
    w0 = c0 * 2 * L // 16
    words[w0:w0 + w.numel()] = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    del F, frag, a, b, flat, w
quals = torch.randint(35, 75, ((n * L + 3) // 4 * 4,), device=dev, dtype=torch.uint8, generator=gen)
torch.cuda.synchronize()

res = {"metric": "sdt_gpu_merge_pairs_device beside sdt_gpu_overlap_pairs_device and sdt_gpu_compact_trimmed_device: ms per call", "pairs": P, "reads": n,
       "read_len": L, "fragments": [args.frag_min, args.frag_max], "err": args.err, "steps": args.steps}
oparams = dict(min_overlap=30, max_err_pct=10, min_len=0, flags=0)
mparams = dict(min_len=0, max_len=0, phred_offset=33, flags=0)

with pkg.PregraphGPU(31, est_distinct=1 << 20) as g:

    def timed(name, call, events=True):
        call()                                          # warm-up
        wall, kern = [], []
        for _ in range(args.steps):
            g.kernel_time(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(g.kernel_time(reset=True)[0])
        res[name + "_wall_ms"] = [round(x, 3) for x in wall]
        if events:
            res[name + "_kernel_ms"] = [round(x, 3) for x in kern]
        return statistics.median(wall)

    d_ov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_mg = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_ow = torch.zeros((nwords,), dtype=torch.int32, device=dev)
    d_oo = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    overlap = timed("overlap", lambda: g.overlap_pairs_device(words, offsets, n, d_ov, None, oparams))
    ins = d_ov[0::2, 2]
    res.update({"pairs_overlapping": int((ins > 0).sum()), "median_insert": int(ins[ins > 0].float().median())})
    out = []
    plain = timed("merge", lambda: out.append(g.merge_pairs_device(words, offsets, n, d_ov, d_mg, d_ow, nwords, d_oo, None, mparams)))
    nm, nw = out[-1]
    merged_bases = int(d_oo[nm])
    res.update({"pairs_merged": nm, "merged_bases": merged_bases, "mismatch_columns": int(d_mg[0::2, 1].sum())})
    withq = timed("merge_quals", lambda: out.append(g.merge_pairs_device(words, offsets, n, d_ov, d_mg, d_ow, nwords, d_oo, quals, mparams)))
    assert out[-1] == (nm, nw)
    res["from_b"] = int(d_mg[0::2, 2].sum())
    compact = timed("compact_trimmed", lambda: out.append(g.compact_trimmed_device(words, offsets, n, d_ov, d_ow, nwords, d_oo)), events=False)
    res["compact_trimmed_bases"] = int(d_oo[out[-1][0]])
    moved = n * L // 4 + 48 * n + 3 * merged_bases // 4
    res.update({"merge_yardstick_bytes": moved, "merge_bytes_per_merged_base": round(moved / merged_bases, 3),
                "merge_yardstick_GB_per_s": round(moved / (plain * 1e-3) / 1e9, 1), "merge_quals_yardstick_GB_per_s": round(moved / (withq * 1e-3) / 1e9, 1),
                "merge_over_overlap": round(plain / overlap, 3), "merge_quals_over_overlap": round(withq / overlap, 3),
                "merge_over_compact_trimmed": round(plain / compact, 3), "merge_quals_over_compact_trimmed": round(withq / compact, 3)})
print(json.dumps(res))
