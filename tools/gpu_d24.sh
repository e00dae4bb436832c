#!/bin/bash
# the reference ring: Phi72 GPU tests, then its bench line twice (4 streams, one batch of 4)
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
TAG=${1:-d24}
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_parity.py \
  tests/test_gpu_batch.py tests/test_gpu_scale.py -k "${KSEL:-24 or phi72 or reference}" > $OUT/pytest_$TAG.log 2>&1
rc=$?; tail -3 $OUT/pytest_$TAG.log; [ $rc -eq 0 ] || exit $rc
run() {  # name, args
  timeout -k 10 300 python -u bench.py --full --no-small-shape --no-cpu-baseline $2 > $OUT/bench_${TAG}_$1.log 2>&1 || return 1
  python3 -c "
import json; d=json.loads([l for l in open('$OUT/bench_${TAG}_$1.log') if l.startswith('{')][-1])
print('$1', round(d['value'],2), round(d['ms_per_step'],3), {k: round(v['avg_launch_ms'],3) for k,v in d['phases'].items()})"
}
A="--d 24 --w 19763 --streams 4 --batch 4 --steps 128 --warmup 8"
run a "$A" && run b "$A"
