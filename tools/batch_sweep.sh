#!/bin/bash
# keyframes/s as a function of the batch: one `bench.py --full` line per batch size into $OUT/sweep_<B>.json (OUT defaults to sweep/)
cd "$(dirname "$0")/.."; OUT=${OUT:-sweep}; mkdir -p "$OUT"
for b in ${BATCHES:-1 4 16 64 128 256 512}; do
  timeout 400 python bench.py --full --batch $b --no-cpu-baseline --inputs resident --unique-frames 16 --render-workers 0 > "$OUT/sweep_$b.json" 2> "$OUT/sweep_$b.err"
  python - $b "$OUT/sweep_$b.json" <<'PY'
import json, sys
b = sys.argv[1]
try:
    d = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
    k = d["kernels_ms_per_step"]
    print(b, d["value"], d["ms_per_step"], k.get("lm_window_kernel"), round(sum(v for n, v in k.items() if n.startswith("orb_")), 4), d["roofline"]["frac"])
except Exception as e:
    print(b, "failed", e)
PY
done
