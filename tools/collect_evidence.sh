#!/bin/bash
# copy a gpu_evidence.sh run's summaries from $OUT/ into profiles/ (committed):
# the per-line PMC files bench.py reads, the bench line, the rocprof kernel-trace
# summary with its roctx windows, and the line-vs-trace check
TAG=${1:?tag}; R=${2:-r06}
cd "$(dirname "$0")/.." || exit 1
export OUT=${OUT:-bench_out}  # where the logs and records go
cp $OUT/pmc_traffic_d*_W*_k*.json $OUT/pmc_sq_d*_W*_k*.json profiles/ 2>/dev/null
# (tools/gpu_pmc_side.sh also leaves its pmc_{traffic,sq}_side_ops.json under $OUT/pmc_side)
cp $OUT/pmc_side/pmc_*_side_ops.json profiles/ 2>/dev/null
grep "^{" $OUT/bench_$TAG.log | tail -1 > profiles/${R}_bench.json
grep "^{" $OUT/benchprof_$TAG.log | tail -1 > profiles/${R}_benchprof.json
cp $OUT/bench_detail_$TAG.json profiles/${R}_bench_detail.json
cp $OUT/benchprof_detail_$TAG.json profiles/${R}_benchprof_detail.json
cp $OUT/stats_$TAG.md profiles/${R}_rocprof_stats_windows.md
cp $OUT/stats_$TAG.windows.json profiles/${R}_rocprof_stats_windows.json
python tools/check_profile.py $OUT/benchprof_$TAG.log $OUT/stats_$TAG.windows.json > profiles/${R}_check_profile.txt
python tools/check_profile.py $OUT/bench_$TAG.log $OUT/stats_$TAG.windows.json > profiles/${R}_check_bench_vs_trace.txt
exit 0
