BENCH_OUT=${BENCH_OUT:-bench_out}      # where the result lines, logs and traces go
cd "$(dirname "$0")/.."; mkdir -p $BENCH_OUT
for i in 1 2 3; do
  for v in early late; do
    a=""; [ $v = late ] && a="--late-alloc"
    timeout -k 10 300 python -u bench.py --full --steps 4 --warmup 1 --no-cpu --no-pcie --no-census $a > $BENCH_OUT/al_$v$i.json 2> $BENCH_OUT/al_$v$i.log || exit 1
    python3 -c "import json; d=json.load(open('$BENCH_OUT/al_$v$i.json')); print('$v$i', d['ms_per_step'], d['roofline']['dominant_kernel']['phases_ms_per_step'])"
  done
done
