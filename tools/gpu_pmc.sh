#!/bin/bash
# PMC passes on the GPU box (MI355X_MICROARCH.md §HBM / §rocprofv3 PMC slots):
# FETCH_SIZE and WRITE_SIZE in separate passes, then SQ issue counters.
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
TAG=${1:-pmc}
ARGS="--steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS}"
mkdir -p $OUT
rocprofv3 -L > $OUT/counters_$TAG.txt 2>&1 || true
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch_$TAG -o run --output-format csv -- \
  python bench.py --full $ARGS > $OUT/pmc_fetch_$TAG.log 2>&1 && echo fetch ok &&
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write_$TAG -o run --output-format csv -- \
  python bench.py --full $ARGS > $OUT/pmc_write_$TAG.log 2>&1 && echo write ok &&
timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \
  -d $OUT/pmc_sq_$TAG -o run --output-format csv -- \
  python bench.py --full $ARGS > $OUT/pmc_sq_$TAG.log 2>&1 && echo sq ok
