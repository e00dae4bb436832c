#!/bin/bash
# One GPU-box check of the tree as it is: the -m gpu suite, smoke(), then the
# default bench line (compact line on stdout, the full record in
# $OUT/bench_detail_$TAG.json). Stops at the first failure.
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
TAG=${1:-check}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread \
  > $OUT/pytest_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/pytest_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -1 $OUT/smoke_$TAG.log; [ $rc -eq 0 ] || exit $rc
[ -n "$SKIP_BENCH" ] && exit 0
timeout -k 10 600 python bench.py --full --detail $OUT/bench_detail_$TAG.json > $OUT/bench_$TAG.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 2500 $OUT/bench_$TAG.log; exit $rc
