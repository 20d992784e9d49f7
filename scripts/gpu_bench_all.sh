#!/bin/bash
# Default bench (c2, with CPU baseline) + rocprofv3 stats + c3/c5 bench lines.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 400 python bench.py --full > $OUT/bench_c2.log 2>&1 || { echo "bench c2 failed"; tail $OUT/bench_c2.log; exit 1; }
tail -1 $OUT/bench_c2.log
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_c2 -o run --output-format csv -- python3 bench.py --no-cpu-baseline > $OUT/prof_c2.log 2>&1 || { echo "prof failed"; tail $OUT/prof_c2.log; exit 1; }
find $OUT/prof_c2 -name "*kernel_stats.csv" -exec head -4 {} \;
for c in c3 c5; do
  timeout -k 10 400 python bench.py --config $c --no-cpu-baseline > $OUT/bench_$c.log 2>&1 || { echo "bench $c failed"; tail $OUT/bench_$c.log; exit 1; }
  tail -1 $OUT/bench_$c.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$c', d['value'], d['ms_per_step'], d['roofline']['kernel_ms_per_launch'])"
done
