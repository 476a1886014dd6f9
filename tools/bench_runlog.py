#!/usr/bin/env python3
"""What the run's log costs: the method of tools/bench_folds.py --parent DIR on its seeded set of about a million guides.
A record for profiles/runlog.json, not a pass mark; bench.py does not know of it.

    python tools/bench_runlog.py --out profiles/runlog.json [--mbp 8] [--parent DIR] [--pipeline-runs 2]

Pipeline: pipeline.run (medium, n = 2; the genome is input, Bowtie text and off-target index) in processes of their own,
alternating between this tree without `log`, this tree with `log` (a RunLog) and, with --parent, a directory that holds
the parent commit's crackling_amd package with its built library: one warm-up run and --pipeline-runs timed runs per
process, the stand-in's own time taken off.  Every process also times GuideSet.extract alone, warm: the extraction's added
kernel always runs.
Device: the counting launches of issl_runlog_batches by their HIP events (BatchCounts.ms) for one batch and for batches of
5000 rows, warm; the Bowtie step's event count (its sort and k_occur_events) and the extraction's k_guide_files by the HIP
events the library records around them under ISSL_LOCATE_TIMING=1 / ISSL_GUIDES_TIMING=1 and prints in its stage lines,
beside the stage's host-clock figure (the stream synchronised around it; for "files" with its two copies), second run."""
import argparse
import hashlib
import json
import os
import pathlib
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from bench_folds import stand_in, synthetic_genome  # noqa: E402


def child(mbp, runs, with_log):
    """One process: warm-up and `runs` timed pipeline.run, then GuideSet.extract three times -> a JSON line."""
    import torch
    import crackling_amd as ca
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    blob = synthetic_genome(mbp)
    genome = ca.Genome.open([blob])
    index = ca.IsslIndex.build_from_fasta([blob])
    config = dict(optimisation="medium", n=2, model=(z["sv"], z["coef"], float(z["intercept"])))
    spent = {"rnafold": 0.0}

    def rnafold(lines):
        t0 = time.perf_counter()
        out = stand_in(lines)
        spent["rnafold"] += time.perf_counter() - t0
        return out

    times, digest, n_bytes, log_bytes = [], None, 0, 0
    for run in range(runs + 1):
        spent["rnafold"] = 0.0
        kw = {}
        if with_log:
            kw["log"] = ca.RunLog(config)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ca.pipeline.run([blob], genome, index, config, rnafold, **kw)
        dt = time.perf_counter() - t0
        if run:
            times.append(dt - spent["rnafold"])
        digest, n_bytes = hashlib.sha256(out).hexdigest(), len(out)
        if with_log:
            log_bytes = len(kw["log"].text())
    extract = []
    for run in range(4):
        t0 = time.perf_counter()
        ca.GuideSet.extract([blob]).close()
        if run:
            extract.append(time.perf_counter() - t0)
    print(json.dumps({"package": os.path.dirname(ca.__file__), "log": with_log, "seconds": times, "extract_seconds": extract,
                      "bytes": n_bytes, "log_bytes": log_bytes, "sha256": digest}))


def run_children(parent, mbp, runs, rounds=2):
    out = {"this": [], "this_with_log": [], "parent": []}
    trees = [("this", str(ROOT), []), ("this_with_log", str(ROOT), ["--with-log"])]
    if parent:
        trees.append(("parent", str(pathlib.Path(parent).resolve()), []))
    for _ in range(rounds):
        for name, tree, flags in trees:
            env = dict(os.environ, PYTHONPATH=tree)
            r = subprocess.run([sys.executable, __file__, "--child", "--mbp", str(mbp), "--pipeline-runs", str(runs)] + flags,
                               capture_output=True, text=True, env=env, cwd=tree, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    return out


def stages_child(mbp):
    """One process with the libraries' timing lines on: the extraction twice, the Bowtie step with its events twice; the
    lines go to stderr."""
    import torch
    import crackling_amd as ca
    torch.zeros(1, device="cuda:0")
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    blob = synthetic_genome(mbp)
    genome = ca.Genome.open([blob])
    for _ in range(2):
        with ca.GuideSet.extract([blob]) as gs, ca.Consensus(gs, optimisation="medium", n=2, model=(z["sv"], z["coef"], float(z["intercept"]))) as c:
            with c.folds() as f:
                f.read(stand_in(f.input().decode()))
                c.finish(f)
                ca.BowtieStep(c, genome, 0, 0, events=True)


def device_times(mbp, runs=5):
    import torch
    import crackling_amd as ca
    torch.zeros(1, device="cuda:0")
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    blob = synthetic_genome(mbp)
    out = {}
    with ca.GuideSet.extract([blob]) as gs, ca.Consensus(gs, optimisation="medium", n=2, model=(z["sv"], z["coef"], float(z["intercept"]))) as c:
        with c.folds() as f:
            f.read(stand_in(f.input().decode()))
            c.finish(f)
            genome = ca.Genome.open([blob])
            bowtie = c.bowtie(genome, 0, 0)
            rows = bowtie.selected_tensor()
            mit = torch.rand(rows.numel(), dtype=torch.float64, device="cuda") * 100
            scores = (rows, mit, mit.flip(0).contiguous())
            out.update(guides=gs.n_guides, fold_rows=int(c.n_fold), selected=int(c.n_selected), scored=int(rows.numel()))
            for name, batch_size, page in (("one_batch", 0, 5000000), ("batches_of_5000", 5000, 100)):
                ms = [ca.BatchCounts(c, f, bowtie, scores, 75.0, "and", batch_size, page).ms for _ in range(runs + 1)][1:]
                out[f"counts_ms_{name}"] = ms
            genome.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "runlog.json"))
    ap.add_argument("--mbp", type=float, default=8.0)
    ap.add_argument("--parent", default=None, help="a directory with the parent commit's crackling_amd package, built")
    ap.add_argument("--pipeline-runs", type=int, default=2)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stages-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-log", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.mbp, a.pipeline_runs, a.with_log)
    if a.stages_child:
        return stages_child(a.mbp)
    sys.path.insert(0, str(ROOT))
    import torch
    out = {"genome_mbp": a.mbp, "device": torch.cuda.get_device_name(0)}
    out.update(device_times(a.mbp))
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, __file__, "--stages-child", "--mbp", str(a.mbp)], capture_output=True, text=True, cwd=str(ROOT),
                       env=dict(os.environ, PYTHONPATH=str(ROOT), ISSL_GUIDES_TIMING="1", ISSL_LOCATE_TIMING="1"), timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out["extract_files_ms"] = [float(x) for x in re.findall(r" files ([\d.]+) ms", r.stderr)]
    out["bowtie_events_ms"] = [float(x) for x in re.findall(r" events ([\d.]+) ms", r.stderr)]
    out["extract_files_kernel_ms_events"] = [float(x) for x in re.findall(r"k_guide_files ([\d.]+) ms by events", r.stderr)]
    out["bowtie_events_ms_events"] = [float(x) for x in re.findall(r"k_occur_events ([\d.]+) ms by events", r.stderr)]
    out["bowtie_verdicts_ms"] = [float(x) for x in re.findall(r" verdicts ([\d.]+) ms", r.stderr)]
    out["stage_lines"] = [line for line in r.stderr.splitlines() if line.startswith("[issl")][-4:]
    runs = run_children(a.parent, a.mbp, a.pipeline_runs)
    out["pipeline"] = runs
    for name, rs in runs.items():
        secs = [s for r in rs for s in r["seconds"]]
        if secs:
            out[f"pipeline_{name}_s_median"] = statistics.median(secs)
            out[f"pipeline_{name}_s_spread"] = max(secs) - min(secs)
            out[f"extract_{name}_s_median"] = statistics.median(s for r in rs for s in r["extract_seconds"])
            ex = [s for r in rs for s in r["extract_seconds"]]
            out[f"extract_{name}_s_spread"] = max(ex) - min(ex)
    out["pipeline_same_bytes"] = len({r["sha256"] for rs in runs.values() for r in rs}) == 1
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "pipeline"}))


if __name__ == "__main__":
    main()
