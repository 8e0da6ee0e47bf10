#!/bin/bash
# usage: tools/prof_kernels.sh <tag> [bench args...]   (run on the GPU box; prints per-kernel averages > 1 %)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
tag=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -- python3 bench.py --full --no-cpu-baseline --no-double "$@" > $OUT/$tag.log 2>&1
python3 - "$tag" <<'PY'
import os
import csv,glob,sys
f=glob.glob(os.environ["OUT"] + "/%s/*/*kernel_stats.csv"%sys.argv[1])[0]
for r in csv.DictReader(open(f)):
    if float(r["Percentage"])>1.0: print(r["Name"][:64], r["Calls"], round(float(r["AverageNs"])/1e3,1))
PY
grep "^{" $OUT/$tag.log | cut -c1-150
