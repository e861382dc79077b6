#!/bin/bash
# Round-6 evidence (run on a GPU box from the repo root): bash profiles/collect_r06.sh OUTDIR PARENT [PART ...]
# PARENT: a built checkout of the parent commit (its Python layer does not know the new entry points, so the parent runs from
# its own tree; bench.py is the same file in both); the tree's own build is the new library.  Parent and new are alternated
# within every round, in this one job.  PARTs (default: all):
#   rates  python bench.py (200 steps) x 3 and --steps 20 --warmup 5 x 6: parent, FXRX_TAIL_GANG = 1, 2, 4
#   guard  what must not regress, 3 rounds: --no-pipeline --steps 50, --continuous, tools/dropin_latency.py at 100 Msamples/s:
#          parent, FXRX_TAIL_GANG = 2, 4
#   trace  rocprofv3 kernel trace of bench.py --steps 20 --warmup 5, one run each: parent, FXRX_TAIL_GANG = 2, 4
# Every bench line goes to OUTDIR/rates.jsonl as {"label", "gang", "out": [the tool's JSON lines]}.  Every GPU step under its own time limit; the
# script stops at the first step that fails.
set -e -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; O="$1"; P="$2"; shift 2; PARTS="${*:-rates guard trace}"
mkdir -p "$O"; O="$(cd "$O" && pwd)"; P="$(cd "$P" && pwd)"
[ -f "$P/gr-liquiddsp_amd/csrc/libfxrx.so" ] || { echo "no built parent tree at $P" >&2; exit 2; }
cd "$R"
echo "GPU_MAX_HW_QUEUES in the environment: ${GPU_MAX_HW_QUEUES:-unset}" > "$O/env.txt"

# one LABEL GANG(- = parent) TOOL ARGS...
one() {
    local label="$1" gang="$2"; shift 2
    local line
    if [ "$gang" = - ]; then line="$(cd "$P" && timeout -k 10 240 python3 "$@" 2>> "$O/stderr.txt" | grep '^{' | paste -sd, -)"
    else line="$(FXRX_TAIL_GANG="$gang" timeout -k 10 240 python3 "$@" 2>> "$O/stderr.txt" | grep '^{' | paste -sd, -)"; fi
    [ "$gang" = - ] && gang=null
    echo "{\"label\": \"$label\", \"gang\": $gang, \"out\": [$line]}" | tee -a "$O/rates.jsonl"
}
trace() {   # NAME GANG
    local name="$1" gang="$2"
    if [ "$gang" = - ]; then (cd "$P" && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace_$name" -o bench -- python3 bench.py --steps 20 --warmup 5 > "$O/${name}bench_under_rocprof.json" 2>> "$O/stderr.txt")
    else FXRX_TAIL_GANG="$gang" timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace_$name" -o bench -- python3 bench.py --steps 20 --warmup 5 > "$O/${name}bench_under_rocprof.json" 2>> "$O/stderr.txt"; fi
    python3 tools/dev/trace_summary.py "$(find "$O/trace_$name" -name "*kernel_trace.csv" | head -1)" > "$O/${name}bench_timeline.txt"
    cp "$(find "$O/trace_$name" -name "*kernel_stats.csv" | head -1)" "$O/${name}bench_kernel_stats.csv"
    rm -rf "$O/trace_$name"
}
for part in $PARTS; do case "$part" in
rates)
    for r in 1 2 3; do one parent_200 - bench.py; for g in 1 2 4; do one new_g${g}_200 $g bench.py; done; done
    for r in 1 2 3 4 5 6; do one parent_20 - bench.py --steps 20 --warmup 5; for g in 1 2 4; do one new_g${g}_20 $g bench.py --steps 20 --warmup 5; done; done ;;
guard)
    for r in 1 2 3; do
        one parent_nopipe - bench.py --no-pipeline --steps 50; for g in 2 4; do one new_g${g}_nopipe $g bench.py --no-pipeline --steps 50; done
        one parent_cont - bench.py --continuous; for g in 2 4; do one new_g${g}_cont $g bench.py --continuous; done
        one parent_dropin - tools/dropin_latency.py --rates 100e6 --repeats 2; for g in 2 4; do one new_g${g}_dropin $g tools/dropin_latency.py --rates 100e6 --repeats 2; done
    done ;;
trace)
    trace parent_ -; trace g2_ 2; trace "" 4 ;;
*) echo "unknown part $part" >&2; exit 2 ;;
esac; done
