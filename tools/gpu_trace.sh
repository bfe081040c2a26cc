#!/bin/bash
# rocprofv3 kernel trace of one bench configuration: $BENCH_OUT/trace_<name>/
# usage: tools/gpu_trace.sh <name> <bench args...>
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
name=$1; shift
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $BENCH_OUT/trace_$name -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-census "$@" > $BENCH_OUT/trace_$name.log 2>&1
rc=$?; echo "[trace $name] exit $rc"; tail -3 $BENCH_OUT/trace_$name.log
exit $rc
