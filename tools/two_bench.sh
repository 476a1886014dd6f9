#!/bin/bash
# Both bench lines (even and skewed index) without extras or CPU baseline: step and stage times (development aid, GPU box).
#   tools/two_bench.sh <outdir>
cd "$(dirname "$0")/.."
OUT=${1:?usage: tools/two_bench.sh <outdir>}
mkdir -p "$OUT"
for d in uniform markov; do
  python3 bench.py --full --dist $d --no-extras --no-cpu-baseline > "$OUT/two_bench_$d.json" 2> "$OUT/two_bench_$d.err"
  python3 -c "
import json
d = json.load(open('$OUT/two_bench_$d.json'))
print('$d', round(d['ms_per_step'], 3), {k: round(v, 3) for k, v in d['kernel_ms'].items()})"
done
