#!/bin/bash
# usage: tools/prof_all.sh <tag> [bench args...]   (GPU box) per-kernel averages of EVERY kernel of the bench command, sorted by total time
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
tag=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -- python3 bench.py --full --no-cpu-baseline "$@" > $OUT/$tag.log 2>&1
python3 - "$tag" <<'PY'
import os
import csv,glob,sys
f=glob.glob(os.environ["OUT"] + "/%s/*/*kernel_stats.csv"%sys.argv[1])[0]
rows=list(csv.DictReader(open(f)))
for r in rows:
    print("%-70s calls %6s avg %8.1f us total %8.2f ms  %5.1f%%" % (r["Name"][:70], r["Calls"], float(r["AverageNs"])/1e3, float(r["TotalDurationNs"])/1e6, float(r["Percentage"])))
PY
grep "^{" $OUT/$tag.log | cut -c1-150
