#!/usr/bin/env python3
"""RNAfold's exchange at the scale of a batch: the seeded set of tools/bench_results.py, about a million guides with every
guide folded.  A record for profiles/folds.json, not a pass mark; bench.py does not know of it.

    python tools/bench_folds.py --out profiles/folds.json [--mbp 8] [--runs 5] [--parent DIR] [--pipeline-runs 2]

Device: Folds.input() and Folds.read() over the whole fold list, several times, warm, by the library's own HIP events
(issl_folds_times), next to the host clock around the whole call (the upload of RNAfold's text and the one wait included).
Host: Consensus.fold_input(), read_rnafold_output() and read_rnafold_text() on the same box, by the host clock; their
results must equal the device's.  RNAfold's stand-in answers every line with one made-up structure line of the real length.
Table: ResultTable over the same set with the ss columns from the Folds (quoted in the kernel) and from a host-packed
PackedFolds, by ResultTable.times(), alternating; same bytes.
Pipeline: pipeline.run (medium, n = 2; the genome is input, Bowtie text and off-target index) in processes of their own,
alternating between this tree and, with --parent, a directory that holds the parent commit's crackling_amd package with
its built library: one warm-up run and --pipeline-runs timed runs per process, the stand-in's own time taken off."""
import argparse
import hashlib
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
SECOND = "." * 28 + "((((....))))...))))" + "." * 21 + "((((....))))(((((((...)))))))... (-21.30)\n"


def synthetic_genome(mbp, seed=20261019, records=20):
    rng = np.random.default_rng(seed)
    per = int(mbp * 1e6) // records
    parts = []
    for r in range(records):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, per)].tobytes()
        parts.append(b">chr%d synthetic record\n" % (r + 1) + seq + b"\n")
    return b"".join(parts)


def stand_in(lines):
    """RNAfold's answer to its input: every line, and one structure line behind it."""
    return lines.replace("\n", "\n" + SECOND)


def pipeline_child(mbp, runs):
    """One process: warm-up and `runs` timed pipeline.run -> a JSON line."""
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

    times, digest, n_bytes = [], None, 0
    for run in range(runs + 1):
        spent["rnafold"] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ca.pipeline.run([blob], genome, index, config, rnafold)
        dt = time.perf_counter() - t0
        if run:
            times.append(dt - spent["rnafold"])
        digest, n_bytes = hashlib.sha256(out).hexdigest(), len(out)
    print(json.dumps({"package": os.path.dirname(ca.__file__), "has_folds": hasattr(ca, "Folds"), "seconds": times, "bytes": n_bytes,
                      "sha256": digest}))


def run_children(parent, mbp, runs, rounds=2):
    out = {"this": [], "parent": []}
    trees = [("this", str(ROOT))] + ([("parent", str(pathlib.Path(parent).resolve()))] if parent else [])
    for _ in range(rounds):
        for name, tree in trees:
            env = dict(os.environ, PYTHONPATH=tree)
            r = subprocess.run([sys.executable, __file__, "--pipeline-child", "--mbp", str(mbp), "--pipeline-runs", str(runs)],
                               capture_output=True, text=True, env=env, cwd=tree, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "folds.json"))
    ap.add_argument("--mbp", type=float, default=8.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a directory with the parent commit's crackling_amd package, built")
    ap.add_argument("--pipeline-runs", type=int, default=2)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--pipeline-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.pipeline_child:
        return pipeline_child(a.mbp, a.pipeline_runs)
    sys.path.insert(0, str(ROOT))
    import torch
    import crackling_amd as ca
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    gs = ca.GuideSet.extract([synthetic_genome(a.mbp)])
    c = ca.Consensus(gs, optimisation="ultralow", n=2, model=(z["sv"], z["coef"], float(z["intercept"])))
    out = {"guides": gs.n_guides, "fold_rows": int(c.n_fold), "genome_mbp": a.mbp, "runs": a.runs, "device": torch.cuda.get_device_name(0)}
    dev = {"input_ms_events": [], "input_ms_call": [], "read_ms_events": [], "read_ms_call": []}
    lines = answer = folds = texts = None
    for run in range(a.runs + 1):  # run 0 warms up
        with c.folds() as f:
            t0 = time.perf_counter()
            lines = f.input()
            t_in = 1e3 * (time.perf_counter() - t0)
            if answer is None:
                answer = stand_in(lines.decode()).encode()
            t0 = time.perf_counter()
            f.read(answer)
            t_read = 1e3 * (time.perf_counter() - t0)
            t = f.times()
            if run:
                dev["input_ms_events"].append(t["input"])
                dev["input_ms_call"].append(t_in)
                dev["read_ms_events"].append(t["read"])
                dev["read_ms_call"].append(t_read)
            if run == a.runs:
                folds, texts = f.folds, f.texts()
    out["device_ms_median"] = {k: statistics.median(v) for k, v in dev.items()}
    out["device_ms_all_runs"] = dev
    out["input_bytes"], out["answer_bytes"] = len(lines), len(answer)
    out["input_gb_per_s"] = len(lines) / (out["device_ms_median"]["input_ms_events"] * 1e-3) / 1e9
    out["read_gb_per_s"] = len(answer) / (out["device_ms_median"]["read_ms_events"] * 1e-3) / 1e9
    host = {"fold_guides_s": [], "fold_input_s": [], "read_rnafold_output_s": [], "read_rnafold_text_s": []}
    text = answer.decode()
    for run in range(2):
        t0 = time.perf_counter()
        guides = c.fold_guides()
        host["fold_guides_s"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h_lines = c.fold_input()
        host["fold_input_s"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h_folds = ca.read_rnafold_output(text, guides)
        host["read_rnafold_output_s"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h_texts = ca.read_rnafold_text(text, guides)
        host["read_rnafold_text_s"].append(time.perf_counter() - t0)
    out["host_s"] = host
    out["identical"] = bool(h_lines.encode() == lines and h_folds.tobytes() == folds.tobytes() and h_texts == texts)
    # the result table's three ss columns: spans of the device's text, quoted by the kernel (put_fold_span), against the
    # host-packed pool of the same texts; no Bowtie rows and no scores, the variants alternating run by run
    table = {"folds_on_device": [], "packed_on_host": []}
    with c.folds() as f:
        f.read(answer)
        c.finish(f)
        packed = ca.PackedFolds(h_texts)
        same = None
        for run in range(a.runs + 1):
            for name, arg in (("folds_on_device", f), ("packed_on_host", packed)):
                with ca.ResultTable(c, arg) as t:
                    if run:
                        table[name].append(t.times())
                    elif same is None:
                        same = t.to_bytes()
                    else:
                        same = same == t.to_bytes()
    out["table_ms_median"] = {k: {s: statistics.median(t[s] for t in v) for s in ("measure", "scan", "emit")} for k, v in table.items()}
    out["table_ms_all_runs"] = table
    out["table_same_bytes"] = bool(same)
    c.close()
    gs.close()
    del c, gs
    torch.cuda.empty_cache()
    if not a.no_pipeline:
        runs = run_children(a.parent, a.mbp, a.pipeline_runs)
        out["pipeline"] = runs
        for name, rs in runs.items():
            secs = [s for r in rs for s in r["seconds"]]
            if secs:
                out[f"pipeline_{name}_s_median"] = statistics.median(secs)
        if runs["parent"]:
            out["pipeline_same_bytes"] = len({r["sha256"] for rs in runs.values() for r in rs}) == 1
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    assert out["identical"], "the device and the host helpers disagree"
    print(json.dumps({k: v for k, v in out.items() if k not in ("device_ms_all_runs", "table_ms_all_runs", "pipeline")}))


if __name__ == "__main__":
    main()
