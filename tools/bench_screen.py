#!/usr/bin/env python3
"""sdt_gpu_screen_reads_device beside sdt_gpu_profile_reads_device on the same reads, on a synthetic workload that is resident in HBM
(torch_workload: the workload of DESIGN.md 4g).  The reference set is every tenth transcript of the workload's transcriptome (200 of
2 000), one reference each; the parameters are the defaults of `sdt-kmers screen` (k = 31, min_hits 1, min_hit_pct 0, drop the matched).
    python tools/bench_screen.py --reads 4000000 --read-len 150 --K 31 --T 2000 --steps 4
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first), reads per second, the share
of the reads that are matched, the wall time of sdt_gpu_screen_load (staging, build and the wait for it), the size of the set, and the
ratio to the profile call: the existing stage that also does one look-up per k-mer, in the much larger counted table.  The records of
every --check-every-th read are held to the rule restated in numpy on the CPU (canonical k-mers as 64-bit integers, the set as a sorted
array with the smallest reference per k-mer), and the first 200 of them also to the plain Python restatement of tests/read_screen_util.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
from soapdenovo_trans_amd import synth  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import read_screen_util as su  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--K", type=int, default=31)
ap.add_argument("--T", type=int, default=2000)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--screen-k", type=int, default=31)
ap.add_argument("--ref-every", type=int, default=10, help="one transcript in this many is a reference")
ap.add_argument("--check-every", type=int, default=16, help="one read in this many is held to the rule on the CPU")
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n, k = pkg.clamp_K(args.K), args.read_len, args.reads, args.screen_k
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
tx_codes, tx_starts, _ = synth.make_transcriptome(args.T, seed=42)              # (torch_workload's transcriptome: tx_seed = 42)
refs = [tx_codes[int(tx_starts[t]):int(tx_starts[t + 1])] for t in range(0, args.T, args.ref_every)]
ref_codes, ref_offs = su.concat(refs)
ref_words = synth.pack_2bit(ref_codes)
ref_of_seq = np.arange(len(refs), dtype=np.uint32)
params = dict(min_hits=1, min_hit_pct=0, flags=0, reserved=0)


def canonical(codes2d):
    """the canonical k-mers of reads of one length, (m, L) codes -> (m, L - k + 1) uint64"""
    c = codes2d.astype(np.uint64)
    nk = c.shape[1] - k + 1
    fw = np.zeros((c.shape[0], nk), dtype=np.uint64)
    rc = np.zeros((c.shape[0], nk), dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | c[:, j:j + nk]
        rc |= (c[:, j:j + nk] ^ np.uint64(2)) << np.uint64(2 * j)
    return np.minimum(fw, rc)


def set_arrays():
    """(sorted distinct canonical k-mers of the references, the smallest reference of each)"""
    keys, ref = [], []
    for i, r in enumerate(refs):
        if len(r) >= k:
            x = canonical(r[None, :])[0]
            keys.append(x)
            ref.append(np.full(len(x), i, dtype=np.uint32))
    keys, ref = np.concatenate(keys), np.concatenate(ref)
    order = np.lexsort((ref, keys))
    keys, ref = keys[order], ref[order]
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    return keys[first], ref[first]


def rule(codes2d, keys, kref):
    m = codes2d.shape[0]
    x = canonical(codes2d)
    at = np.minimum(np.searchsorted(keys, x), len(keys) - 1)
    hit = keys[at] == x
    hits = hit.sum(axis=1)
    ref = np.where(hit, kref[at], su.NO_REF).min(axis=1)
    rec = np.zeros(m, dtype=pkg.READ_SCREEN_DTYPE)
    dropped = hits >= 1
    rec["kmers"], rec["hits"], rec["ref"] = x.shape[1], hits, ref
    rec["len"], rec["verdict"] = np.where(dropped, 0, codes2d.shape[1]), dropped
    return rec


res = {"metric": "sdt_gpu_screen_reads_device beside sdt_gpu_profile_reads_device: ms per call", "reads": n, "read_len": L, "K": K, "T": args.T,
       "err": args.err, "steps": args.steps, "screen_k": k, "references": len(refs), "reference_bases": int(ref_offs[-1]), "params": params}

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

    load = []
    for _ in range(args.steps + 1):                     # (the first is the warm-up)
        t0 = time.perf_counter()
        distinct = g.screen_load(ref_words, ref_offs, ref_of_seq, len(refs), k)
        load.append((time.perf_counter() - t0) * 1e3)
    info = g.screen_info()
    res.update({"screen_load_wall_ms": [round(x, 3) for x in load[1:]], "set_kmers": distinct, "set_slots": info[3], "set_bytes": 16 * info[3]})
    d_rec = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    d_keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    kept = []
    best = timed("screen", lambda: kept.append(g.screen_reads_device(words, offsets, n, d_rec, d_keep, params=params)))
    matched = int((d_rec[:, 1] > 0).sum())
    res.update({"screen_reads_per_s": round(n / (best * 1e-3)), "screen_kmers_per_s": round(n * (L - k + 1) / (best * 1e-3)), "screen_kept": kept[-1],
                "matched_reads": matched, "matched_share": round(matched / n, 4)})
    # the sample against the rule on the CPU
    shifts = 30 - 2 * torch.arange(16, device=dev, dtype=torch.int64)
    sample = []
    chunk = 1 << 20
    assert (chunk * L) % 16 == 0 and chunk % args.check_every == 0
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        w = words[c0 * L // 16:((c0 + m) * L + 15) // 16].long() & 0xFFFFFFFF
        codes = ((w[:, None] >> shifts[None, :]) & 3).reshape(-1)[: m * L].reshape(m, L)
        sample.append(codes[:: args.check_every].to(torch.uint8).cpu().numpy())
    sample = np.concatenate(sample)
    got = d_rec[:: args.check_every].cpu().numpy().view(np.uint8).copy().view(pkg.READ_SCREEN_DTYPE).reshape(-1)
    keys, kref = set_arrays()
    want = rule(sample, keys, kref)
    head = min(200, len(sample))
    hcodes, hoffs = su.concat(list(sample[:head]))
    plain = su.expect_screen(hcodes, hoffs, k, su.build_set(refs, list(range(len(refs))), k), params)[0]
    res.update({"sample_reads": len(sample), "sample_records_equal_the_rule": bool((got == want).all()), "set_kmers_by_the_rule": int(len(keys)),
                "sample_matched": [int((got["hits"] > 0).sum()), int((want["hits"] > 0).sum())],
                "first_200_equal_the_plain_restatement": bool((got[:head] == plain).all())})
    del d_rec, d_keep
    # the yardstick: the profile of the same reads against their counted table, in the same process
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers_counted"], res["nodes"] = g.finish_count()
    d_cov = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prof = timed("k_profile_reads", lambda: g.profile_reads_device(words, offsets, n, L, 0, d_cov))
    res["screen_over_profile"] = round(best / prof, 3)
    res["set_kept_across_the_count"] = g.screen_info()[2] == distinct
    res["not_measured"] = ["long reads", "large sets such as a full SILVA", "the host form", "the kept form", "the command line"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
