#!/bin/bash
# Round evidence: default bench (with CPU baselines + census), rocprofv3 kernel-trace stats of
# the same command, host-ingest end to end, 2-rank gloo rehearsal of the multi-GPU bench.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
stop_on() { case "$1" in 0) ;; *) echo "[$2] exit $1 -> stop"; exit $1 ;; esac; }
timeout -k 10 600 python -u bench.py --full > $BENCH_OUT/bench_default.json 2> $BENCH_OUT/bench_default.log
stop_on $? bench; cat $BENCH_OUT/bench_default.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $BENCH_OUT/prof_default -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-census > $BENCH_OUT/prof_default.log 2>&1
stop_on $? rocprof
timeout -k 10 300 python -u tools/ingest_bench.py --records 1000000 --gpu > $BENCH_OUT/ingest.json 2> $BENCH_OUT/ingest.log
stop_on $? ingest; cat $BENCH_OUT/ingest.json
CRDT_BENCH_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 2 --warmup 1 --records 250000000 > $BENCH_OUT/bench_weak2.json 2> $BENCH_OUT/bench_weak2.log
stop_on $? weak2; cat $BENCH_OUT/bench_weak2.json
