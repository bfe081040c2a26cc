#!/bin/bash
# GPU parity suite, then a rocprofv3 kernel-trace summary of one bench config.
# usage: tools/gpu_prof_cfg.sh <name> <bench args...>
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
name=$1; shift
timeout -k 10 900 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests > $BENCH_OUT/t_gpu.log 2>&1
rc=$?; tail -3 $BENCH_OUT/t_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u bench.py --full "$@" --no-cpu > $BENCH_OUT/bench_$name.json 2> $BENCH_OUT/bench_$name.log
rc=$?; echo "[bench $name] exit $rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $BENCH_OUT/prof_$name -o run -- python3 bench.py --full "$@" --steps 2 --warmup 1 --no-cpu --no-census > $BENCH_OUT/prof_$name.log 2>&1
rc=$?; echo "[prof $name] exit $rc"; exit $rc
