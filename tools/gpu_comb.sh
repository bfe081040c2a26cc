#!/bin/bash
# Map-side combine checks: the small combine tests, then the N = 2 bench path over gloo (one GPU).
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
mkdir -p $BENCH_OUT
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest -v --timeout 150 --timeout-method thread -m gpu tests -k "${TESTS:-combine}" > $BENCH_OUT/comb_tests.log 2>&1
echo "[tests] exit $?"; tail -3 $BENCH_OUT/comb_tests.log
CRDT_BENCH_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29563 bench.py --full --gpus 2 --steps 2 --warmup 1 --records 4000000 --replicas 16 ${BENCH_ARGS:-} > $BENCH_OUT/comb_bench2.json 2> $BENCH_OUT/comb_bench2.log
echo "[bench2] exit $?"
python3 -c "
import json; d=json.load(open('$BENCH_OUT/comb_bench2.json')); print(d['ms_per_step'], json.dumps(d.get('parity')), d['roofline']['dominant_kernel'].get('plan'))" || tail -30 $BENCH_OUT/comb_bench2.log
