#!/bin/bash
# end-of-round check of HEAD on the GPU box: the whole -m gpu suite, smoke(), the default
# bench line and a rocprofv3 kernel-trace --stats run of the default workload
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
TAG=${1:-final}
timeout -k 10 900 python -u -m pytest tests -m gpu -q -x -p no:cacheprovider --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
rc=$?; tail -3 $OUT/pytest_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1
rc=$?; tail -1 $OUT/smoke_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.log 2>&1
rc=$?; tail -c 400 $OUT/bench_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- \
  python bench.py --full --no-cpu-baseline --no-small-shape > $OUT/benchprof_$TAG.log 2>&1
rc=$?; echo "prof rc=$rc"; [ $rc -eq 0 ] || exit $rc
python tools/prof_summary.py stats $OUT/prof_$TAG $OUT/stats_${TAG}_d1024_W16384.md > /dev/null
