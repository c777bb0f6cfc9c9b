#!/bin/bash
# Round benchmark + rocprofv3 kernel-trace summary on the GPU box. Each GPU step has its own timeout;
# steps are chained so that a failure stops the script.
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}  # where this script writes (relative to the repository root)
mkdir -p $OUT
STEPS=${STEPS:-20}
timeout -k 10 900 python bench.py --full --steps "$STEPS" --warmup 3 > $OUT/bench.json 2> $OUT/bench.err || { echo "bench failed rc=$?"; exit 1; }
cat $OUT/bench.json
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$OUT/prof" -o run -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_bench.json 2> $OUT/prof.err || { echo "rocprof failed rc=$?"; exit 1; }
find $OUT/prof -name "*stats*" | head
