#!/bin/bash
# Several bench.py configurations back to back; stops at the first crash/timeout.
# usage: tools/gpu_benches.sh "<name>:<bench args>" ...
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
for spec in "$@"; do
  name=$(echo "$spec" | cut -d: -f1); cmd=$(echo "$spec" | cut -d: -f2-)
  timeout -k 10 400 python -u bench.py --full $cmd > $BENCH_OUT/bench_$name.json 2> $BENCH_OUT/bench_$name.log
  rc=$?; echo "[bench $name] exit $rc"; cat $BENCH_OUT/bench_$name.json
  [ $rc -eq 0 ] || exit $rc
done
