#!/usr/bin/env python3
"""Time of the efficiency consensus on a resident guide set: issl_consensus_begin + issl_consensus_finish (DESIGN.md,
"Efficiency consensus").  The guides are those of the first --mbp Mbp of tools/genome_index.py's seeded repeat genome
(the default gives about 5 M distinct guides); mm10db is off, so nothing has to be folded: G20 and the sgRNAScorer2
score of every guide at ultralow, where the filter holds no guide back, and at the default, high with n = 2.  A host
clock around the two calls, which end in a synchronise and include their allocations; warm-up runs first; the median and
the spread of --runs runs.  Prints one JSON line and writes it to --out."""
import argparse
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, default=42.0)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import crackling_amd as ca
    import genome_index
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    model = (z["sv"], z["coef"], float(z["intercept"]))
    with tempfile.TemporaryDirectory() as work:
        fa = pathlib.Path(work) / "genome.fa"
        genome_index.genome(fa, a.mbp, "repeat", a.seed)
        gs = ca.GuideSet.extract([str(fa)])
    res = {"genome_mbp": a.mbp, "seed": a.seed, "guides": gs.n_guides, "guides_seen_once": gs.n_unique, "support_vectors": len(model[1]),
           "timed": "issl_consensus_begin + issl_consensus_finish, host clock, allocations included", "runs": a.runs, "warmup": a.warmup}
    for level in ("ultralow", "high"):
        kw = dict(optimisation=level, n=2, mm10db=False, model=model)
        times, scored, selected = [], 0, 0
        for r in range(a.warmup + a.runs):
            t = time.perf_counter()
            c = gs.consensus(kw)
            c.finish(None)
            dt = time.perf_counter() - t
            if r >= a.warmup:
                times.append(dt * 1e3)
            if r == 0:
                scored = int((~np.isnan(c.rows["sgrna_score"])).sum())
                selected = c.n_selected
            c.close()
        res[level] = {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "guides_scored": scored,
                      "selected": selected, "ns_per_guide": 1e6 * statistics.median(times) / max(gs.n_guides, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
