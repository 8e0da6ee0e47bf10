#!/bin/bash
# usage: tools/timeline_run.sh <tag> "<ENV=... settings>" [bench args]   (GPU box) kernel-trace of a short bench run under the given environment,
# then the timeline of one replayed step and a one-line-per-step table (tools/step_timeline.py) into $OUT/<tag>.txt
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
tag=$1; envs=$2; shift; shift
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
export $envs
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/$tag -- python3 bench.py --full --no-cpu-baseline --no-double --steps 40 --warmup 5 "$@" > $OUT/$tag.log 2>&1
python3 tools/step_timeline.py $OUT/$tag 12 1 > $OUT/$tag.txt
python3 tools/step_timeline.py $OUT/$tag summary 100 100 >> $OUT/$tag.txt
rm -rf $OUT/$tag
echo "== $tag: $envs"; head -14 $OUT/$tag.txt
