#!/bin/bash
# Host path against device path of the Hungarian targets (scratch/assign_bench.py), then the solver kernel alone from a
# kernel trace of its own (no counters in that run).  Every GPU step under its own time limit; the first failure ends the script.
set -u
OUT=${OUT:-scratch/out}/assign
mkdir -p "$OUT"
timeout -k 10 420 python scratch/assign_bench.py time > "$OUT/assign_times.jsonl" 2> "$OUT/assign_times.err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o assign -- python scratch/assign_bench.py trace > "$OUT/trace.log" 2>&1 &&
python scratch/assign_bench.py report "$OUT/trace" > "$OUT/assign_kernel.jsonl"
rc=$?
cat "$OUT/assign_times.jsonl" "$OUT/assign_kernel.jsonl" 2>/dev/null
tail -5 "$OUT/assign_times.err" 2>/dev/null
exit $rc
