#!/bin/bash
# usage: tools/env_sweep.sh <tag> "<ENV=.. ENV=..>" ["<ENV..>" ...] -- [bench args]   (GPU box) one bench line per environment setting: step times and per-kernel PME stamps
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
TAG=$1; shift
SETS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do SETS+=("$1"); shift; done
[ "$1" == "--" ] && shift
for S in "${SETS[@]}"; do
  env $S python3 bench.py --full --no-cpu-baseline --no-double "$@" 2>$OUT/sweep_$TAG.err | tail -1 > $OUT/sweep_$TAG.json && python3 tools/pmeprint.py $OUT/sweep_$TAG.json "[$S]" | tee -a $OUT/sweep_$TAG.txt || { echo "[$S] failed"; tail -3 $OUT/sweep_$TAG.err; }
done
