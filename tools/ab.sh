#!/bin/bash
# A/B timing on one box: alternate bench runs of ab/lib*.so builds (names as args)
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
TAG=${TAG:-}
for rep in 1 2; do
  for v in "$@"; do
    LATTICEUM_AMD_LIB=ab/lib$v.so timeout -k 10 300 python bench.py --full --no-cpu-baseline ${BENCH_ARGS} > $OUT/ab_${TAG}${v}_$rep.log 2>&1 || exit 1
  done
done
