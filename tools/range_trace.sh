#!/bin/bash
# Kernel trace (a run of its own, no counters) of the threshold search: one 2,560-query block of
# CosineIndex.search_above against 1 M rows (tools/range_bench.py --only-new). Prints the leg's JSON
# line and the per-kernel totals of libclm's kernels; the full CSVs stay under bench_out/range_trace.
set -o pipefail
out=bench_out/range_trace
mkdir -p $out
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $out -o run -- \
  python tools/range_bench.py --rows 1000000 --queries 2560 --only-new > $out/run.log 2>&1 || { tail -20 $out/run.log; exit 1; }
grep '"leg"' $out/run.log
head -1 $out/run_kernel_stats.csv
grep 'clm::' $out/run_kernel_stats.csv
