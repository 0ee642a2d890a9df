#!/usr/bin/env python3
"""sdt_gpu_asm_add_device beside sdt_gpu_profile_reads_device on the same sequences and table, and sdt_gpu_asm_spectrum, in one process:
reads of tools/bench_trim.py's kind (torch_workload, resident in HBM) counted into the table, and as the assembly the transcriptome
they were drawn from -- every transcript a contig, 500 to 4 000 bases, so profile's strip holds each one and both kernels make the same
look-ups; profile keeps the counts for a median, asm_add tallies a byte per found k-mer and walks the gaps.
    python tools/bench_asm.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 3 --out profiles/asm_support/bench_asm_8M_T45000.json
Prints one JSON line: ms per call (HIP events inside the library around the kernel, one warm-up call first, the best of --steps),
k-mers/s of both, their ratio; the wall clock of asm_spectrum (kernel, 64 KiB back, the wait) and the bytes of the table it scans.  The
records of every --check-every-th contig, the totals and the matrix's column sums are held to profile's records and to each other."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
from soapdenovo_trans_amd import synth  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=8_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--K", type=int, default=31)
ap.add_argument("--T", type=int, default=45000, help="transcripts: about 2 250 bases each, so 45 000 are about 10^8 bases of contigs")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--min-count", type=int, default=2)
ap.add_argument("--rows", type=int, default=256)
ap.add_argument("--check-every", type=int, default=97)
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, err=args.err)
# the assembly: the transcriptome itself (tx_seed 42, as torch_workload draws it), packed on the host once
codes, starts, _ = synth.make_transcriptome(args.T)
asm_words = torch.from_numpy(synth.pack_2bit(codes).view(np.int32)).to(dev)
asm_offs = torch.from_numpy(starts.astype(np.int64)).to(dev)
nseq, longest = args.T, int((starts[1:] - starts[:-1]).max())
kmers = int(np.maximum(starts[1:] - starts[:-1] - K + 1, 0).sum())
del codes

res = {"metric": "sdt_gpu_asm_add_device beside sdt_gpu_profile_reads_device on the same contigs and table: ms per call and k-mers/s; sdt_gpu_asm_spectrum: wall ms",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "min_count": args.min_count, "rows": args.rows,
       "contigs": nseq, "contig_bases": int(starts[-1]), "contig_kmers": kmers, "longest_contig": longest}

with pkg.PregraphGPU(K, est_distinct=max(1 << 20, int(1.3 * int(starts[-1]) + 0.07 * n * L))) as g:
    res["library"] = os.path.basename(pkg.LIB_PATH)
    g.count_reads_device(words, nwords, offsets, n, L)
    res["kmers_in_reads"], res["nodes"] = g.finish_count()
    res["table_slots"] = int(g.lib.sdt_gpu_table_slots(g._ctx))

    def timed(name, call, before=lambda: None):
        before()
        call()                                          # warm-up (the first add also collects the high halves: k_hi_count)
        per = []
        for _ in range(args.steps):
            before()
            torch.cuda.synchronize()
            g.kernel_time(reset=True)
            call()
            torch.cuda.synchronize()
            per.append(g.kernel_time(reset=True)[0])
        res[name + "_ms"] = [round(x, 3) for x in per]
        return min(per)

    d_cov = torch.zeros((nseq, 6), dtype=torch.int32, device=dev)
    d_rec = torch.zeros((nseq, 4), dtype=torch.int64, device=dev)
    prm = dict(min_count=args.min_count, rows=args.rows)
    profile = timed("profile", lambda: g.profile_reads_device(asm_words, asm_offs, nseq, longest, args.min_count, d_cov))
    # every timed add starts from a zeroed tally: the bytes go 0 -> 1, the common case of an assembly
    asm = timed("asm_add", lambda: g.asm_add_device(asm_words, asm_offs, nseq, d_rec), before=lambda: g.asm_begin(prm))
    # a second add on top of the first: the bytes go 1 -> 2, the same words are swapped again
    g.asm_begin(prm)
    g.asm_add_device(asm_words, asm_offs, nseq, d_rec)
    again = timed("asm_add_again", lambda: g.asm_add_device(asm_words, asm_offs, nseq, None))
    # the spectrum: wall clock of the blocking call
    g.asm_begin(prm)
    g.asm_add_device(asm_words, asm_offs, nseq, d_rec)
    g.asm_spectrum()
    walls = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, tot = g.asm_spectrum()
        walls.append(1e3 * (time.perf_counter() - t0))
    res["spectrum_wall_ms"] = [round(x, 3) for x in walls]
    entry = 16 if K <= 31 else (32 if K <= 63 else 48)
    res["spectrum_bytes"] = res["table_slots"] * (entry + 4 + 1)
    res["spectrum_gb_per_s_wall"] = round(res["spectrum_bytes"] / (min(walls) * 1e-3) / 1e9, 1)
    # held to profile's records and to each other
    rec = d_rec.cpu().numpy().view(pkg.SEQ_SUPPORT_DTYPE).reshape(nseq)
    cov = d_cov.cpu().numpy().view(pkg.READ_COV_DTYPE).reshape(nseq)
    pick = slice(None, None, args.check_every)
    res["records_agree_with_profile"] = bool((rec["kmers"][pick] == cov["kmers"][pick]).all() and (rec["found"][pick] == cov["found"][pick]).all()
                                             and (rec["solid"][pick] == np.where(args.min_count >= 1, cov["solid"][pick], cov["found"][pick])).all())
    res["totals"] = [int(x) for x in tot]
    res["totals_agree_with_records"] = bool(int(tot[0]) == nseq and int(tot[1]) == int(rec["kmers"].sum()) == kmers and int(tot[2]) == int(rec["found"].sum())
                                            and int(tot[3]) == int(rec["solid"].sum()))
    res["matrix_nodes"] = int(m.sum())
    res["matrix_agrees_with_node_count"] = bool(int(m.sum()) == res["nodes"])
    res["matrix_columns"] = [int(x) for x in m.sum(axis=0)]
    res["profile_kmers_per_s"] = round(kmers / (profile * 1e-3))
    res["asm_add_kmers_per_s"] = round(kmers / (asm * 1e-3))
    res["asm_add_again_kmers_per_s"] = round(kmers / (again * 1e-3))
    res["asm_add_over_profile"] = round(asm / profile, 3)
    res["not_measured"] = ["the tally alone (no build without it)", "the host form", "the command line", "contigs past profile's limit of 16 384 k-mers",
                           "a table with high halves (HI_HASH / HI_AUX)"]
    g.asm_end()
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
