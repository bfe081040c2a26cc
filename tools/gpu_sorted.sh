#!/bin/bash
# Sorted-path session: parity tests for both paths, then benches + a kernel trace.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py -x -v --timeout 300 --timeout-method thread -k "sorted" \
  > $BENCH_OUT/pytest_sorted.log 2>&1
rc=$?; tail -5 $BENCH_OUT/pytest_sorted.log; echo "[pytest sorted] exit $rc"; [ $rc -eq 0 ] || exit $rc
for spec in "$@"; do
  name=$(echo "$spec" | cut -d: -f1); cmd=$(echo "$spec" | cut -d: -f2-)
  timeout -k 10 400 python -u bench.py --full $cmd > $BENCH_OUT/bench_$name.json 2> $BENCH_OUT/bench_$name.log
  rc=$?; echo "[bench $name] exit $rc"; cat $BENCH_OUT/bench_$name.json; [ $rc -eq 0 ] || exit $rc
done
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $BENCH_OUT/trace_sorted -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-census --path sorted > $BENCH_OUT/trace_sorted.log 2>&1
rc=$?; echo "[trace] exit $rc"; exit $rc
