#!/bin/bash
# Runs on the GPU box: kernel trace + stats of the C3 bench command (with --full) → build/traces/<tag>/c3_kernel_stats.txt
# usage: scripts/quick_trace.sh <tag> [extra bench args]
TAG=$1; shift
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/build/traces/$TAG
mkdir -p "$OUT"
cd /tmp
rocprofv3 --kernel-trace --stats -d "$OUT" -o trace -- python "$R/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-callsite --no-graph "$@" > "$OUT/trace.log" 2>&1
cd "$R"
python scripts/rocprof_summary.py "$OUT/trace_results.db" > "$OUT/c3_kernel_stats.txt" 2>&1
rm -f "$OUT"/*.db
head -16 "$OUT/c3_kernel_stats.txt"
grep stages "$OUT/trace.log"
