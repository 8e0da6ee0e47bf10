#!/bin/bash
# GPU box: the round's judged artefacts in one call -- the default bench line (replayed steps overlapped, round 4), the same command with
# SNB_OVERLAP=0 SNB_SIDE_REBUILD=0 (serial replayed steps and in-line rebuilds, rounds 1-3's form), rocprofv3 --kernel-trace --stats of the bench command with the kernels
# running ALONE (SNB_OVERLAP=0: the per-kernel durations the `roofline` objects are defined on; the stamped eager steps of the default line
# are serial too and must agree) and once more as shipped (overlapped: the pair kernel's two launches and the PME kernels beside it),
# one SQ --pmc pass and one MFMA pass (kernels alone).  Copy $OUT/final/* into profiles/ afterwards (tools/make_profiles.py).
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; export OUT=${OUT:-tools_out}; mkdir -p "$OUT"      # results go to $OUT (relative paths: under the repository root)
set -e
mkdir -p $OUT/final
python3 bench.py --full > $OUT/final/bench.json 2> $OUT/final/bench.err
SNB_OVERLAP=0 SNB_SIDE_REBUILD=0 python3 bench.py --full --no-cpu-baseline --no-double > $OUT/final/bench_serial.json 2> $OUT/final/bench_serial.err
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
export SNB_OVERLAP=0 SNB_SIDE_REBUILD=0      # (kernels alone: no PME chain and no list build beside the pair kernel)
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final/stats -- python3 bench.py --full --no-cpu-baseline --no-double > $OUT/final/bench_under_rocprof.json 2> $OUT/final/rocprof.err
cp $OUT/final/stats/*/*kernel_stats.csv $OUT/final/kernel_stats.csv
bash tools/pmc_sq.sh final_sq "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_LDS SQ_INSTS_MFMA SQ_WAIT_INST_ANY" --steps 40 --warmup 5 > $OUT/final/pmc_sq.txt
# matrix-core BUSY cycles of the kernel that carries the lambda mix (plane path: k_fftZInvMix, v_mfma_f32_4x4x1_16b_f32; else k_convolveX), beside the count above
bash tools/pmc_sq.sh final_mfma "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_MFMA" --steps 40 --warmup 5 > $OUT/final/pmc_mfma.txt
unset SNB_OVERLAP SNB_SIDE_REBUILD
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final/stats_overlap -- python3 bench.py --full --no-cpu-baseline --no-double > $OUT/final/bench_under_rocprof_overlap.json 2> $OUT/final/rocprof_overlap.err
cp $OUT/final/stats_overlap/*/*kernel_stats.csv $OUT/final/kernel_stats_overlap.csv
rm -rf $OUT/final/stats $OUT/final/stats_overlap $OUT/final_sq $OUT/final_mfma
head -c 400 $OUT/final/bench.json; echo; head -5 $OUT/final/kernel_stats.csv | cut -c1-160
