#!/bin/bash
# GPU box: the packed tail as a step.  First the interleaved A/B of scripts_dev/ab_packed_tail.py (profiler off), then each arm alone
# under rocprofv3 --kernel-trace --stats for the per-kernel totals; everything into $OUT (default bench_out/ab)
# usage: scripts_dev/ab_packed_tail.sh [bf16|fp32|mx8]   (fp32: _ops.PACKED_TAIL_FP32 on the fp32 step, fewer replays of a ~34 ms step;
#        mx8: the three arms a / b / c of the MX-fp8 mode at the cfg-5 shape, see ab_packed_tail.py)
# every GPU step runs under its own timeout and the script stops at the first one that fails
set -o pipefail
PREC=${1:-bf16}
ROUNDS=7; REPLAYS=30; PROF=20
ARMS="off on"
if [ "$PREC" = fp32 ]; then REPLAYS=10; PROF=5; fi
if [ "$PREC" = mx8 ]; then REPLAYS=20; PROF=10; ARMS="a b c"; fi
export TMPDIR=/tmp
export OUT=${OUT:-bench_out/ab}
mkdir -p $OUT
timeout -k 10 400 python3 scripts_dev/ab_packed_tail.py $PREC $ROUNDS $REPLAYS 2>&1 | tee $OUT/ab.log | tail -15 || exit 3
for m in $ARMS; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/$m -- python3 scripts_dev/ab_packed_tail.py $PREC profile $m $PROF > $OUT/$m.log 2>&1 || exit 4
  python3 - $m <<'PY' || exit 5
import csv, glob, os, sqlite3, sys
m = sys.argv[1]
d = sqlite3.connect(glob.glob(os.environ["OUT"] + f"/{m}/**/*.db", recursive=True)[0])
with open(os.environ["OUT"] + f"/{m}_kernel_stats.csv", "w", newline="") as f:
    w = csv.writer(f)
    w.writerow(["Name", "Calls", "TotalDurationUs", "AverageUs", "Percentage"])
    for n, c, t, a, p in d.execute("select name,total_calls,total_duration,average,percentage from top_kernels"):
        w.writerow([n, c, round(t, 1), round(a, 2), round(p, 3)])
PY
  rm -rf $OUT/$m
  tail -2 $OUT/$m.log
done
