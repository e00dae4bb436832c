#!/bin/bash
# the default headline (no side lines) several times on one box: run-to-run spread
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
for rep in 1 2 3 4; do
  timeout -k 10 300 python -u bench.py --full --no-small-shape --no-cpu-baseline > $OUT/bench_hr_$rep.log 2>&1 || exit 1
  python3 -c "
import json; d=json.loads([l for l in open('$OUT/bench_hr_$rep.log') if l.startswith('{')][-1])
print('$rep', round(d['value'],2), round(d['ms_per_step'],3), d['steps'], d['warmup'])"
done
