#!/usr/bin/env python3
"""sdt_gpu_compare_tables and sdt_gpu_compare_select on two counted tables, beside two kernels that were there before, in one process:
two libraries of tools/bench_asm.py's kind (torch_workload, resident in HBM) from the same transcriptome -- B under another sampling
seed and another expression (sigma 1.5 against 2.0 on the same draws) -- each counted into a context of its own.
    python tools/bench_compare.py --reads 8000000 --read-len 150 --K 31 --T 45000 --steps 3 --out profiles/table_compare/bench_compare_8M_T45000.json
Prints one JSON line.  Pass 1 (A walked, B probed), pass 2 (B walked, A probed) and the selection are timed by the HIP events the
library records around each kernel (pass 1 and the selection are booked on A, pass 2 on B: sdt_gpu_kernel_time), one warm-up call
first, the best of --steps.  The yardsticks, in the same process on the same tables:
  (a) k_asm_spectrum on A at 256 rows, the scan without a probe: events on the stream around the blocking call (a memset of 16 KiB, the
      kernel, 16 KiB back), since that call books no events of its own;
  (b) sdt_gpu_search_kmers_device on B with A's exported keys, the probes without a scan: the library's events.
Both contexts run on torch's current stream for this.  What is compared is held to the node counts and to (b)'s answers."""
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
ap.add_argument("--T", type=int, default=45000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--err", type=float, default=0.002)
ap.add_argument("--min-count", type=int, default=2)
ap.add_argument("--out", default="", help="also write the JSON line to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K, L, n = pkg.clamp_K(args.K), args.read_len, args.reads
bases = 2250 * args.T                                    # (about: transcripts of 500 to 4 000 bases)
est = max(1 << 20, int(1.3 * bases + 0.07 * n * L))
res = {"metric": "sdt_gpu_compare_tables (pass 1, pass 2) and sdt_gpu_compare_select beside k_asm_spectrum (a) and sdt_gpu_search_kmers_device (b): ms per kernel",
       "reads": n, "read_len": L, "K": K, "T": args.T, "err": args.err, "steps": args.steps, "min_count": args.min_count,
       "library_b": "seed 43, sigma 1.5 (A: seed 42, sigma 2.0), the same transcriptome"}


def counted(seed, sigma):
    words, offsets, nwords = synth.torch_workload(n, L, args.T, dev, seed=seed, err=args.err, sigma=sigma)
    torch.cuda.synchronize()                            # (the context counts on a stream of its own: the reads must be there first)
    g = pkg.PregraphGPU(K, est_distinct=est)
    g.count_reads_device(words, nwords, offsets, n, L)
    kmers, nodes = g.finish_count()
    del words, offsets
    torch.cuda.empty_cache()
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return g, kmers, nodes


a, res["kmers_a"], res["nodes_a"] = counted(42, 2.0)
b, res["kmers_b"], res["nodes_b"] = counted(43, 1.5)
with a, b:
    res["library"] = os.path.basename(pkg.LIB_PATH)
    res["slots_a"], res["slots_b"] = int(a.lib.sdt_gpu_table_slots(a._ctx)), int(b.lib.sdt_gpu_table_slots(b._ctx))
    res["occupied_share_a"], res["occupied_share_b"] = round(res["nodes_a"] / res["slots_a"], 4), round(res["nodes_b"] / res["slots_b"], 4)

    def reset():
        torch.cuda.synchronize()
        a.kernel_time(reset=True)
        b.kernel_time(reset=True)

    def timed_tables(rows, cols):
        out = pkg.compare_tables(a, b, rows, cols)      # warm-up (the first call also collects both tables' high halves)
        p1, p2, wall = [], [], []
        for _ in range(args.steps):
            reset()
            t0 = time.perf_counter()
            out = pkg.compare_tables(a, b, rows, cols)
            wall.append(1e3 * (time.perf_counter() - t0))
            p1.append(a.kernel_time(reset=True)[0])
            p2.append(b.kernel_time(reset=True)[0])
        tag = f"{rows}x{cols}"
        res[f"pass1_{tag}_ms"], res[f"pass2_{tag}_ms"] = [round(x, 3) for x in p1], [round(x, 3) for x in p2]
        res[f"tables_{tag}_wall_ms"] = [round(x, 3) for x in wall]
        return out, min(p1), min(p2)

    (m, tot), p1, p2 = timed_tables(64, 64)
    (m2, tot2), q1, q2 = timed_tables(2, 8192)
    res["totals"] = [int(x) for x in tot]
    X, Y, S = (int(x) for x in tot[:3])
    res["totals_agree_with_node_counts"] = bool(X == res["nodes_a"] and Y == res["nodes_b"] and int(tot[3]) == res["kmers_a"] and int(tot[4]) == res["kmers_b"])
    res["matrix_sums_to_the_union"] = bool(int(m.sum()) == X + Y - S == int(m2.sum()) and (tot2 == tot).all())
    res["matrices_agree"] = bool(int(m2[0].sum()) == int(m[0].sum()) == Y - S and int(m2[1, 0]) == int(m[1:, 0].sum()) == X - S)
    c = args.min_count
    res["solid_a"], res["solid_b"], res["solid_shared"] = int(m[c:].sum()), int(m[:, c:].sum()), int(m[c:, c:].sum())

    # the selection: the solid k-mers of A that B does not hold; counted only (capacity 0), then listed in full (wall clock: the kernel,
    # the scan of the chunk fills, the compaction, the list back to the host and split into its arrays)
    rg = (c, 2**32 - 1, 0, 0)
    n_sel = pkg.compare_select_count(a, b, *rg)
    per = []
    for _ in range(args.steps):
        reset()
        assert pkg.compare_select_count(a, b, *rg) == n_sel
        per.append(a.kernel_time(reset=True)[0])
    res["select_count_ms"] = [round(x, 3) for x in per]
    sel_count = min(per)
    per, wall = [], []
    for _ in range(args.steps):
        reset()
        t0 = time.perf_counter()
        keys, ca, cb = pkg.compare_select(a, b, *rg, capacity=n_sel)
        wall.append(1e3 * (time.perf_counter() - t0))
        per.append(a.kernel_time(reset=True)[0])
    res["select_list_kernel_ms"], res["select_list_wall_ms"] = [round(x, 3) for x in per], [round(x, 3) for x in wall]
    res["selected"] = int(n_sel)
    res["selection_agrees_with_matrix"] = bool(n_sel == int(m[c:, 0].sum()) == len(keys) and (cb == 0).all() and (ca >= c).all())
    sel_list = min(per)

    # (a) the scan without a probe
    a.asm_begin(dict(min_count=c, rows=256))
    a.asm_spectrum()
    per = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.steps):
        torch.cuda.synchronize()
        e0.record()
        a.asm_spectrum()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1))
    a.asm_end()
    res["a_asm_spectrum_ms"] = [round(x, 3) for x in per]
    ya = min(per)

    # (b) the probes without a scan: every node of A asked of B
    keys_a = a.export_nodes()[0]
    d_keys = torch.from_numpy(keys_a.view(np.int64)).to(dev)
    d_cnt = torch.zeros(len(keys_a), dtype=torch.int32, device=dev)
    d_st = torch.zeros(len(keys_a), dtype=torch.uint8, device=dev)
    b.search_kmers_device(d_keys, len(keys_a), d_count=d_cnt, d_status=d_st)
    per = []
    for _ in range(args.steps):
        reset()
        b.search_kmers_device(d_keys, len(keys_a), d_count=d_cnt, d_status=d_st)
        torch.cuda.synchronize()
        per.append(b.kernel_time(reset=True)[0])
    res["b_search_kmers_ms"] = [round(x, 3) for x in per]
    yb = min(per)
    res["search_agrees_with_totals"] = bool(int((d_st & 1).sum().item()) == S and int(d_cnt.long().sum().item()) == int(tot[7]))

    entry = 16 if K <= 31 else (32 if K <= 63 else 48)
    res["scan_bytes_a"], res["scan_bytes_b"] = res["slots_a"] * (entry + 4), res["slots_b"] * (entry + 4)
    res["best_ms"] = {"pass1_64x64": round(p1, 3), "pass2_64x64": round(p2, 3), "pass1_2x8192": round(q1, 3), "pass2_2x8192": round(q2, 3),
                      "select_count": round(sel_count, 3), "select_list_kernel": round(sel_list, 3), "a_scan": round(ya, 3), "b_probes": round(yb, 3),
                      "a_plus_b": round(ya + yb, 3)}
    res["pass1_over_a_plus_b"] = round(p1 / (ya + yb), 3)
    res["lds_64KiB_over_16KiB_pass1"] = round(q1 / p1, 3)
    res["not_measured"] = ["pass 2 against yardsticks of its own (B's scan, A probed with B's keys)", "the command line", "key widths of 2 and 4 words",
                           "tables with many high halves (HI_HASH beyond a handful of nodes, HI_AUX)", "two tables of very different size"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
