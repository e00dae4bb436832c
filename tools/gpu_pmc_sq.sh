#!/bin/bash
# SQ issue/stall counters for every kernel of a short default-workload bench run (one --pmc pass).
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
TAG=${1:-sq}
mkdir -p $OUT
timeout -s KILL 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_SALU \
  SQ_ACTIVE_INST_ANY SQ_WAVES GRBM_GUI_ACTIVE -d $OUT/pmc_sq_$TAG -o run --output-format csv -- \
  python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-small-shape ${BENCH_ARGS} > $OUT/pmc_sq_$TAG.log 2>&1
echo "rc=$?"
