#!/bin/bash
# round 4, final measurements on the GPU box (one gpurun call, every step under its own timeout): the whole -m gpu suite, kernel
# statistics + the three PMC passes of the judged configuration with the shipped build, the judged bench line, the reporting
# matrix (K = 23 / 63 / 95, C2, C5), the whole sdt-pregraph at 200 M reads (twice) and at 20 M reads against the reference.
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=gpurun_out/r4_final; rm -rf $O; mkdir -p $O
timeout 1500 python -m pytest tests -x -q -m gpu > $O/pytest_gpu.log 2>&1; tail -2 $O/pytest_gpu.log
# (--est-distinct = what bench.py's own estimate gives for this workload: its four prefix passes would otherwise be profiled too)
bash tools/pmc_pipeline.sh $O/pmc200 --est-distinct 809675638
python3 tools/pmc_pipeline_summary.py $O/pmc200 200000000 150 31 1 $O/pmc_pass1_200M_k31.json
cp $O/pmc200/kernel_stats.csv $O/kernel_stats_bench_200M_k31.csv 2>/dev/null; cp $O/pmc200/bench_under_rocprof.json $O/bench_under_rocprof_200M_k31.json 2>/dev/null
find $O/pmc200 -name "pass_*" -type d | xargs rm -rf
mkdir -p profiles/r4 && cp $O/pmc_pass1_200M_k31.json profiles/r4/pmc_pass1_200M_k31.json      # bench.py reads the traffic from here
timeout 900 python bench.py --full > $O/bench_default_200M_k31.json 2> $O/bench_default_200M_k31.err
tail -1 $O/bench_default_200M_k31.json | cut -c1-300
run() { name=$1; shift; timeout 600 python bench.py --full "$@" > $O/bench_$name.json 2> $O/bench_$name.err; tail -1 $O/bench_$name.json | cut -c1-160; }
run K23_100bp_200M --reads 200000000 --read-len 100 --K 23 --cpu-sample 4000000
run K63_250bp_50M --reads 50000000 --read-len 250 --K 63 --cpu-sample 2000000
run K95_250bp_50M --reads 50000000 --read-len 250 --K 95 --cpu-sample 2000000 --extras 0
run C2_50M_k31 --reads 50000000 --steps 3 --warmup 1 --cpu-sample 0
run C5_400M_k31_d1_sigma2.5 --reads 400000000 --sigma 2.5 --d 1 --steps 2 --warmup 1 --cpu-sample 0 --extras 0
timeout 400 python tools/e2e_pregraph.py --reads 200000000 --p 16 --T 20000 --skip-ref --timeout 150 --runs 3 > $O/e2e_pregraph_200M_k31_p16_ours_only.json 2> $O/e2e_200M.err
timeout 900 python tools/e2e_pregraph.py --reads 20000000 --p 16 --T 20000 --timeout 600 --runs 2 > $O/e2e_pregraph_20M_k31_p16.json 2> $O/e2e_20M.err
python3 - $O <<'E'
import json, sys
o = sys.argv[1]
for f in ("e2e_pregraph_200M_k31_p16_ours_only.json", "e2e_pregraph_20M_k31_p16.json"):
    try:
        d = json.load(open(o + "/" + f))
        print(f, d.get("ours_walls_s"), d.get("ref_wall_s"), d.get("identical"))
    except Exception as e:
        print(f, "FAILED", e)
E
