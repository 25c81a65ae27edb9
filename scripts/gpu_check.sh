#!/bin/bash
# The end-of-change check on a GPU machine: smoke, GPU parity tests, a short bench (--full), rocprofv3 kernel stats.
# Everything lands in OUT_DIR.
#   bash scripts/gpu_check.sh OUT_DIR        (ROCPROF=1: + kernel stats of the bench)
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: bash scripts/gpu_check.sh OUT_DIR}" && cd "$1" && pwd)
cd $R
export TMPDIR=/tmp
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx9" | head -4 > $O/device.txt
nproc >> $O/device.txt; lscpu | grep -E "Model name|Socket|NUMA node\(s\)" >> $O/device.txt
timeout 600 python __graft_entry__.py smoke > $O/smoke.log 2>&1; echo "smoke rc=$?" | tee -a $O/summary.txt
timeout 1500 python -m pytest tests -m gpu -q --timeout=600 ${PYTEST_ARGS} > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $O/summary.txt
tail -${PYTEST_TAIL:-60} $O/pytest_gpu.log
timeout 900 python bench.py --full --steps ${BENCH_STEPS:-31} --warmup 3 > $O/bench.log 2>&1; echo "bench rc=$?" | tee -a $O/summary.txt
tail -3 $O/bench.log
if [ -n "${ROCPROF}" ]; then
  rm -rf $O/prof
  (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python $R/bench.py --full --steps 31 --warmup 3 --cpu-frames 0 > $O/bench_prof.log 2>&1); echo "rocprof rc=$?" | tee -a $O/summary.txt
  find $O/prof -name "*kernel_stats*" | head;
  f=$(find $O/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -30 "$f"
  # keep the merged output small: drop the per-dispatch trace, keep stats
  find $O/prof -name "*kernel_trace.csv" -size +20M -delete
fi
tail -5 $O/smoke.log
