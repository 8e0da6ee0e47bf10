#!/bin/bash
# usage: tools/ab_pme.sh <tag> <libA.so> <libB.so> [bench args]   (GPU box) A/B/A/B of two builds through SNB_LIB_PATH: step times and per-kernel PME stamps
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
TAG=$1; A=$2; B=$3; shift; shift; shift
for rep in 1 2; do for L in "$A" "$B"; do
  SNB_LIB_PATH=$L python3 bench.py --full --no-cpu-baseline --no-double "$@" 2>/dev/null | tail -1 > $OUT/ab_$TAG.json && python3 tools/pmeprint.py $OUT/ab_$TAG.json $(basename $L) | tee -a $OUT/ab_$TAG.txt
done; done
