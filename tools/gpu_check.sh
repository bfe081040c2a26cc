#!/bin/bash
# GPU parity suite, then the streaming (cfg5) and default fan-in benches; stops at the first failure.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
timeout -k 10 900 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests > $BENCH_OUT/t_gpu.log 2>&1
rc=$?; tail -3 $BENCH_OUT/t_gpu.log; [ $rc -eq 0 ] || exit $rc
for spec in "$@"; do
  name=$(echo "$spec" | cut -d: -f1); args=$(echo "$spec" | cut -d: -f2-)
  timeout -k 10 400 python -u bench.py --full $args > $BENCH_OUT/bench_$name.json 2> $BENCH_OUT/bench_$name.log
  rc=$?; echo "[bench $name] exit $rc"; cat $BENCH_OUT/bench_$name.json; [ $rc -eq 0 ] || exit $rc
done
