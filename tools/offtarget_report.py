#!/usr/bin/env python3
"""Times the off-target report beside threshold-0 scoring on bench.py's index and writes profiles/offtarget_report.json.

  python tools/offtarget_report.py [--dist uniform|markov] [--sites N] [--guides N]          # this tree
  python tools/offtarget_report.py --baseline --package-root <checkout of the parent commit>   # the parent's scoring and issl_dump_hits

Every figure is the median wall time of `--reps` calls after `--warmup` calls on the same device-resident batch, each call
synchronous (the entry points return when the batch is done).  Results are merged into the JSON under a key per
(distribution, tree), so that the runs of both trees on one box end up side by side; `--bench-lines FILE` adds the
`python bench.py` lines of both trees (one JSON line per run, prefixed `parent ` or `branch `)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
ap = argparse.ArgumentParser()
ap.add_argument("--dist", default="uniform", choices=["uniform", "markov"])
ap.add_argument("--sites", type=int, default=300_000_000)
ap.add_argument("--guides", type=int, default=100_000)
ap.add_argument("--max-dist", type=int, default=4)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--baseline", action="store_true", help="only what the parent commit has: issl_score_device and issl_dump_hits at threshold 0")
ap.add_argument("--package-root", default=str(ROOT), help="tree whose crackling_amd (and built library) is imported")
ap.add_argument("--out", default=str(ROOT / "profiles" / "offtarget_report.json"))
ap.add_argument("--bench-lines", default=None)
a = ap.parse_args()
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, a.package_root)
import torch  # noqa: E402  (first: one HIP runtime per process)
torch.zeros(1, device="cuda:0")
import crackling_amd as ca  # noqa: E402
from synth import markov_sites_fast, random_guides_fast, random_sites_fast  # noqa: E402

t0 = time.time()
sigs, occ = (markov_sites_fast if a.dist == "markov" else random_sites_fast)(a.sites, seed=1)
guides = random_guides_fast(sigs, a.guides, seed=2)
ix = ca.IsslIndex.build_on_device(sigs, occ, device=0)
print(f"index of {len(sigs)} sites ready after {time.time() - t0:.0f} s", flush=True)
del sigs, occ
d_g = torch.from_numpy(guides.view(np.int64)).cuda()
d_m = torch.empty(len(guides), dtype=torch.float64, device="cuda:0")
d_c = torch.empty_like(d_m)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


res = {"sites": a.sites, "guides": a.guides, "max_dist": a.max_dist, "warmup": a.warmup, "reps": a.reps,
       "timing": "wall clock around synchronous calls, device-resident guides, median of reps after warmup"}
res["score_device_thr0"] = timed(lambda: ix.score_device(d_g, d_m, d_c, a.max_dist, 0.0, "and"))
res["hits"] = int(ix.stats()["hits"])
if a.baseline:
    res["dump_hits_thr0"] = timed(lambda: ix.dump_hits(guides, a.max_dist, 0.0, "and"))
    res["dump_hits_thr0"]["bytes"] = 24 * res["hits"]
else:
    d_prof = torch.empty(len(guides) * 88, dtype=torch.uint8, device="cuda:0")
    res["profile_device"] = timed(lambda: ix.offtarget_profile_device(d_g, d_prof, a.max_dist))
    d_off = torch.empty(len(guides) + 1, dtype=torch.int64, device="cuda:0")
    total = ix.offtargets_device(d_g, d_off, None, a.max_dist)
    d_recs = torch.empty(total * 40, dtype=torch.uint8, device="cuda:0")
    res["offtargets_device"] = timed(lambda: ix.offtargets_device(d_g, d_off, d_recs, a.max_dist))
    res["offtargets_device"].update(records=total, bytes=40 * total,
                                    records_per_s=total / res["offtargets_device"]["median_ms"] * 1e3)
    res["offtargets_host"] = timed(lambda: ix.offtargets(guides, a.max_dist))
    res["profile_over_score"] = res["profile_device"]["median_ms"] / res["score_device_thr0"]["median_ms"]
ix.close()
out = pathlib.Path(a.out)
doc = json.loads(out.read_text()) if out.exists() else {}
doc[f"{a.dist}|{'parent' if a.baseline else 'branch'}"] = res
if a.bench_lines:
    lines = {"parent": [], "branch": []}
    for line in pathlib.Path(a.bench_lines).read_text().splitlines():
        who, _, body = line.partition(" ")
        if who in lines and body.startswith("{"):
            lines[who].append(json.loads(body))
    doc["bench"] = {k: [{"ms_per_step": r.get("ms_per_step"), "line": r} for r in v] for k, v in lines.items()}
out.write_text(json.dumps(doc, indent=1) + "\n")
print(json.dumps(res), flush=True)
