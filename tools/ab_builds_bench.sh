#!/bin/bash
# Same-box A/B of two builds of the library through bench.py itself (see tools/ab_builds.sh for the recipe):
# tools/_build/libissl_hip_prev.so (the parent's) against the tree's own, alternating.
#   bash tools/ab_builds_bench.sh [ROUNDS, default 5]
# Plain `python3 bench.py`: a warm round and ROUNDS rounds on the even index, then three each on the skewed index and with
# 500 k guides per step, then three with the stage times (--full --no-cpu-baseline --no-extras).  One line per run; a run
# that fails ends the script (nothing is started on a GPU that has just faulted).
set -o pipefail
cd "$(dirname "$0")/.."
ROUNDS=${1:-5}
cp crackling_amd/libissl_hip.so tools/_build/libissl_hip_cur.so
one() { # label prev|cur [bench.py arguments]
  local label=$1 which=$2; shift 2
  cp tools/_build/libissl_hip_$which.so crackling_amd/libissl_hip.so
  timeout -k 10 420 python3 bench.py "$@" 2>/dev/null | python3 -c "
import json,sys
d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d['roofline']
print('$label', {'prev':'parent','cur':'branch'}['$which'], 'ms_per_step', round(d['ms_per_step'],4), 'avg_launch_ms', round(r['avg_launch_ms'],4), 'comparisons_per_launch', r['comparisons_per_launch'], {k:round(x,3) for k,x in (d.get('kernel_ms') or {}).items()})"
  local rc=$?
  if [ $rc -ne 0 ]; then cp tools/_build/libissl_hip_cur.so crackling_amd/libissl_hip.so; echo "FAILED $label $which rc=$rc"; exit 1; fi
}
for round in warm $(seq -f "round%g" 1 $ROUNDS); do
  for which in prev cur; do one $round $which; done
done
for n in 1 2 3; do
  for which in prev cur; do one markov$n $which --dist markov; done
done
for n in 1 2 3; do
  for which in prev cur; do one 500k_$n $which --guides 500000; done
done
for n in 1 2 3; do
  for which in prev cur; do one stages$n $which --full --no-cpu-baseline --no-extras; done
done
cp tools/_build/libissl_hip_cur.so crackling_amd/libissl_hip.so
