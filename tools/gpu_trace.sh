#!/bin/bash
# kernel traces of the headline pair step per variant: SPECS="name:VAR=val,...|bench args" (args after |)
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p bench_out/tl
IFS=';' read -ra ARR <<< "$SPECS"
for spec in "${ARR[@]}"; do
  name=${spec%%:*}; rest=${spec#*:}; envs=${rest%%|*}; args=""
  [ "$rest" != "$envs" ] && args=${rest#*|}
  rm -rf bench_out/tl/$name
  env $(echo "$envs" | tr ',' ' ') timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d bench_out/tl/$name -o run -- python bench.py --full --no-search --no-cpu-baseline --no-l14 --no-varlen --no-index-build --no-unmerged --no-parity-mode --no-trace --steps 10 --warmup 2 $args > bench_out/tl/$name.log 2>&1 || { tail -5 bench_out/tl/$name.log; exit 1; }
  echo "== $name"; python tools/timeline.py $(find bench_out/tl/$name -name "*kernel_trace.csv" | head -1) 5 | head -${LINES_OUT:-24}
done
