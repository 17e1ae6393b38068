#!/bin/bash
# rocprofv3 evidence for one round (run on the GPU box from the repo root;
# OUT: output folder, default bench_out):
#   1. --kernel-trace --stats of a short plain bench run -> $OUT/prof_bench
#   2. FETCH_SIZE pass, 3. WRITE_SIZE pass (eager step)  -> $OUT/pmc_fetch|pmc_write
#   4. MFMA pass (SQ_VALU_MFMA_BUSY_CYCLES, MOPS_BF16, GRBM_GUI_ACTIVE) -> $OUT/pmc_mfma
# then scripts/pmc_traffic.py turns 2+3 into $OUT/pmc_traffic.json and
# scripts/pmc_mfma.py turns 4 into $OUT/pmc_mfma.json.  Copy the summaries
# into profiles/ afterwards.
set -o pipefail
export TMPDIR=/tmp
R=${ROUND:-r02}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -o bench \
  -- python3 bench.py --steps 10 --warmup 3 > "$OUT/prof_bench.log" 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_fetch" -o run \
  -- python3 scripts/layer_profile.py --top 3 $LP_ARGS > "$OUT/pmc_fetch.log" 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_write" -o run \
  -- python3 scripts/layer_profile.py --top 3 $LP_ARGS > "$OUT/pmc_write.log" 2>&1 || exit $?
python3 scripts/pmc_traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" "$OUT/pmc_traffic.json" --config "${PMC_CONFIG:-resnet34/w1/plain/bf16/16x512}" \
  > "$OUT/pmc_traffic.txt"
timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_BF16 GRBM_GUI_ACTIVE \
  --kernel-trace --output-format csv -d "$OUT/pmc_mfma" -o run \
  -- python3 scripts/layer_profile.py --top 3 > "$OUT/pmc_mfma.log" 2>&1 || exit $?
python3 scripts/pmc_mfma.py "$OUT/pmc_mfma" "$OUT/pmc_mfma.json" > "$OUT/pmc_mfma.txt"
