#!/bin/bash
# Round-end evidence at the current tree: counters of MODES (default refil) merged into profiles/counters.json
# (COMMIT names the commit), the whole GPU suite + smoke + the default bench line (gpu_quick.sh), and the default
# `python3 bench.py` under rocprofv3 --kernel-trace --stats (the driver's command).
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}  # where this script writes (relative to the repository root)
export TMPDIR=/tmp
mkdir -p $OUT
if [ -n "${MODES-refil}" ]; then
  MODES=${MODES-refil} COMMIT=${COMMIT:-unknown} MERGE=profiles/counters.json bash scripts/gpu_counters.sh \
      > $OUT/cnt.log 2>&1 || { tail -20 $OUT/cnt.log; exit 1; }
  tail -1 $OUT/cnt.log
fi
SMOKE=1 bash scripts/gpu_quick.sh || exit 1
mkdir -p $OUT/final_prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$OUT/final_prof" -o run \
    -- python3 bench.py --full > $OUT/final_prof/bench.json 2> $OUT/final_prof/bench.err \
    || { tail -20 $OUT/final_prof/bench.err; exit 1; }
python3 -c "
import json; d=json.load(open('$OUT/final_prof/bench.json'))
print('under rocprofv3', round(d['value']/1e6,2), d['roofline']['avg_kernel_ms'], d['league']['value']/1e6, d['refil']['value']/1e6)"
