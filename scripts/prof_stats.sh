#!/bin/bash
# rocprofv3 kernel stats of the bench (fp32 split, eager launches) and of the fp16 leg -> OUT_DIR/{f32,fp16}_stats.csv
#   bash scripts/prof_stats.sh OUT_DIR
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: bash scripts/prof_stats.sh OUT_DIR}" && cd "$1" && pwd)
rm -rf $O/prof_f32 $O/prof_fp16
# --full: the per-kernel timeline frames are part of what is profiled (the 36 frames below)
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_f32 -o bench -- python $R/bench.py --full --steps 31 --warmup 3 --cpu-frames 0 --no-secondary --no-graph > $O/prof_f32.log 2>&1); echo "prof f32 rc=$?"
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_fp16 -o bench -- python $R/bench.py --full --steps 31 --warmup 3 --cpu-frames 0 --no-secondary --no-graph --dtype fp16 > $O/prof_fp16.log 2>&1); echo "prof fp16 rc=$?"
grep -h "^{" $O/prof_f32.log | cut -c1-200; grep -h "^{" $O/prof_fp16.log | cut -c1-200
for m in f32 fp16; do
  db=$(find $O/prof_$m -name "*.db" | head -1)
  # 31 timed + 3 warm-up + 2 timeline frames (one eager warm-up + the bracketed one)
  [ -n "$db" ] && python $R/scripts/rocprof_summary.py $db $O/${m}_stats.csv 36
  find $O/prof_$m -name "*.db" -delete
done
