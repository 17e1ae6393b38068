#!/bin/bash
# Full bench line (parity + roofline) of every config (one box, graph replay)
# -> $OUT/configs.jsonl (OUT: output folder, default bench_out)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
: > "$OUT/configs.jsonl"
for args in "--attention" "--width 2" "--size 1024 --batch 4" "--backbone resnet50" "--width 2 --fp8" "--data --batch 256"; do
  echo "=== bench.py $args"
  timeout -k 10 300 python3 bench.py $args --full --no-cpu-baseline > "$OUT/cfg.log" 2>&1 || { tail -5 "$OUT/cfg.log"; exit 1; }
  grep '^{' "$OUT/cfg.log" | tee -a "$OUT/configs.jsonl" | grep -o '"value": [0-9.]*'
done
