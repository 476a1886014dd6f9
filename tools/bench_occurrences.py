#!/usr/bin/env python3
"""Time of the Bowtie step on a resident genome: issl_genome_occurrences_device ("Bowtie step").

Genome: the seeded 200 Mbp repeat genome of tools/genome_index.py.  Queries: the selection of a `high`, n = 2 consensus
(mm10db off: nothing to fold, as tools/bench_consensus.py) over the guide set of the genome's first --guides-mbp Mbp, and
its first 1 000 as a second point.  Stage times are those of the ISSL_LOCATE_TIMING line, summed over the pieces of a
call: --warmup runs first, then --runs, median and range.  The yardstick is the extraction's `match` stage
(k_match_count + k_match_emit, ISSL_UPLOAD_TIMING) on the same text in the same process: both read the text and test two
patterns at every position.  The free-HBM low-water mark of one call is reported per query.  Prints one JSON line and
writes it to --out."""
import argparse
import json
import os
import pathlib
import re
import statistics
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def head_of(fa, out, bases):
    """The first `bases` bases of the FASTA, records kept."""
    left = bases
    with open(fa, "rb") as src, open(out, "wb") as dst:
        for line in src:
            if line[:1] == b">":
                dst.write(line)
                continue
            if len(line) - 1 >= left:
                dst.write(line[:left] + b"\n")
                return
            dst.write(line)
            left -= len(line) - 1


def stages_of(err):
    """The [issl occurrences] lines of one call -> ({stage: ms summed over the pieces}, counters of the scan, pieces)."""
    lines = [ln for ln in err.splitlines() if ln.startswith("[issl occurrences]")]
    stages, ctr = {}, {}
    for ln in lines:
        for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln):
            stages[m.group(1)] = stages.get(m.group(1), 0.0) + float(m.group(2))
        for m in re.finditer(r"(matches|filter passed|occurrences) (\d+)", ln.split("|", 1)[1] if "|" in ln else ""):
            ctr[m.group(1).replace(" ", "_")] = ctr.get(m.group(1).replace(" ", "_"), 0) + int(m.group(2))
    return stages, ctr, sum(" sites:" in ln for ln in lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, default=200.0)
    ap.add_argument("--guides-mbp", type=float, default=45.0)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import crackling_amd as ca
    import genome_index as gi
    torch.zeros(1, device="cuda:0")
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    model = (z["sv"], z["coef"], float(z["intercept"]))
    res = {"device": torch.cuda.get_device_name(0), "genome_mbp": a.mbp, "kind": "repeat", "seed": a.seed, "guides_mbp": a.guides_mbp,
           "runs": a.runs, "warmup": a.warmup, "timed": "stage times of the ISSL_LOCATE_TIMING line, summed over the pieces of a call"}
    with tempfile.TemporaryDirectory() as work:
        fa, head = pathlib.Path(work) / "genome.fa", pathlib.Path(work) / "head.fa"
        gi.genome(fa, a.mbp, "repeat", a.seed)
        head_of(fa, head, int(a.guides_mbp * 1e6))
        os.environ["ISSL_UPLOAD_TIMING"] = "1"
        ix, err = gi.stderr_of(lambda: ca.IsslIndex.build_from_fasta([str(fa)]))
        os.environ.pop("ISSL_UPLOAD_TIMING")
        ix.close()
        extraction = {m.group(1): float(m.group(2)) for m in re.finditer(r"\[issl genome\] (\w+) ([0-9.]+) ms", err)}
        res["yardstick_match_stage_ms"] = extraction.get("match")
        gs = ca.GuideSet.extract([str(head)])
        os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when the handle is made
        genome = ca.Genome.open([str(fa)])
        os.environ.pop("ISSL_LOCATE_TIMING")
    c = gs.consensus(optimisation="high", n=2, mm10db=False, model=model).finish(None)
    sel = c.selected_tensor().to(torch.int64)
    sigs = gs.sigs_tensor()[sel].contiguous()
    res.update({"guides": gs.n_guides, "selected": int(sigs.numel()), "n_bases": genome.n_bases, "records": len(genome.records)})
    res["queries"] = []
    for n in (int(sigs.numel()), 1000):
        q = sigs[:n].contiguous()
        rows = torch.empty((q.numel(), 32), dtype=torch.uint8, device=q.device)
        runs, ctr, pieces = [], {}, 0
        for r in range(a.warmup + a.runs):
            _, err = gi.stderr_of(lambda: genome.occurrences_device(q, rows))
            stages, ctr, pieces = stages_of(err)
            if r >= a.warmup:
                runs.append(stages)
        with gi.HbmWatch(torch) as hbm:
            genome.occurrences_device(q, rows)
        host = rows.cpu().numpy().view(ca.OCCURRENCE_DTYPE).reshape(-1)
        summary = {k: {"median": statistics.median(s[k] for s in runs), "min": min(s[k] for s in runs), "max": max(s[k] for s in runs)}
                   for k in runs[0]}
        scan = summary["scan"]["median"]
        res["queries"].append({
            "query_sites": int(q.numel()), "pieces": pieces, "stages_ms": summary, "scan_counters": ctr,
            "filter_pass_rate": ctr.get("filter_passed", 0) / max(ctr.get("matches", 1), 1),
            "scan_over_yardstick": scan / res["yardstick_match_stage_ms"] if res["yardstick_match_stage_ms"] else None,
            "rejected": int((host["code"] == 0).sum()), "accepted": int((host["code"] == 1).sum()), "untested": int((host["code"] == 2).sum()),
            "read0_occurs": int((host["record"] != 0xFFFFFFFF).sum()), "max_n_perfect": int(host["n_perfect"].max()) if len(host) else 0,
            "hbm_low_water_bytes": hbm.peak, "hbm_low_water_bytes_per_query": hbm.peak / max(q.numel(), 1)})
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
