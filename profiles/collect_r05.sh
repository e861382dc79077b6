#!/bin/bash
# Round-5 evidence of one build (run on a GPU box from the repo root): bash profiles/collect_r05.sh OUTDIR [LIBRARY]
# LIBRARY: the libfxrx.so to measure (default: the tree's own; the parent commit's build for the r05_parent_* files).
# Kernel trace of the plain bench command (per-kernel averages, hardware queues, launches per block), the lone-block figures
# and the stage shares.  Every GPU step under its own time limit; the script stops at the first step that fails.
set -e -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; O="$1"; [ -n "$2" ] && export FXRX_LIB="$2"
mkdir -p "$O"; cd "$R"
echo "GPU_MAX_HW_QUEUES in the environment: ${GPU_MAX_HW_QUEUES:-unset}" > "$O/env.txt"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o bench -- python3 bench.py --steps 20 --warmup 5 > "$O/bench_under_rocprof.json" 2> "$O/trace.err"
python3 tools/dev/trace_summary.py "$(find "$O/trace" -name "*kernel_trace.csv" | head -1)" > "$O/bench_timeline.txt"
cp "$(find "$O/trace" -name "*kernel_stats.csv" | head -1)" "$O/bench_kernel_stats.csv"
rm -rf "$O/trace"
timeout -k 10 180 python3 bench.py --full --no-cpu-baseline --no-constellation --no-pipeline --steps 50 > "$O/bench_lat.json" 2> "$O/lat.err"
timeout -k 10 240 python3 tools/dev/dev_stage_cost.py > "$O/stage_cost.txt" 2> "$O/stage.err"
