#!/bin/bash
# the default bench line with its step trace
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p bench_out
CLM_TRACE_KEEP=bench_out/trace timeout -k 10 600 python -u bench.py --full > bench_out/bench.json 2> bench_out/bench.err; rc=$?
echo "bench rc=$rc"; tail -c 300 bench_out/bench.json; exit $rc
