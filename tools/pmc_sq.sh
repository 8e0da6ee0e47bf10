#!/bin/bash
# usage: tools/pmc_sq.sh <tag> "<counters>" [bench args...]   (GPU box) one --pmc pass, per-kernel averages
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
tag=$1; ctrs=$2; shift; shift
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
timeout -k 10 500 rocprofv3 --kernel-trace --pmc $ctrs --output-format csv -d $OUT/$tag -- python3 bench.py --full --no-cpu-baseline --no-double "$@" > $OUT/$tag.log 2>&1 || exit 1
python3 - "$tag" <<'PY'
import os
import csv, glob, sys, collections
tag = sys.argv[1]
f = glob.glob(os.environ["OUT"] + "/%s/*/*counter_collection.csv" % tag)[0]
acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
for r in csv.DictReader(open(f)):
    k = r["Kernel_Name"].split("(")[0][:60]
    a = acc[k][r["Counter_Name"]]; a[0] += float(r["Counter_Value"]); a[1] += 1
for k, v in acc.items():
    if any(x in k for x in ("k_direct", "k_spread", "k_interp", "k_conv", "k_fft", "k_plane", "k_nbBuild")):
        print(k, {c: round(a[0] / a[1]) for c, a in v.items()})
PY
