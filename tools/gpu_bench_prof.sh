#!/bin/bash
# Default bench + rocprofv3 kernel-trace of the same command (short run).
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u bench.py --full "$@" > $BENCH_OUT/bench_default.json 2> $BENCH_OUT/bench_default.log
rc=$?; echo "[bench] exit $rc"; cat $BENCH_OUT/bench_default.json; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $BENCH_OUT/prof -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-census "$@" > $BENCH_OUT/prof_bench.log 2>&1
rc=$?; echo "[rocprof] exit $rc"; [ $rc -eq 0 ] || exit $rc
find $BENCH_OUT/prof -name "*stats*" | head
