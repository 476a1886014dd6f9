#!/usr/bin/env python3
"""The result table at the scale of a batch: about a million guides of a made-up genome (fixed seed), every stage's columns
filled.  A record for profiles/results.json, not a pass mark; bench.py does not know of it.

    python tools/bench_results.py --out profiles/results.json [--mbp 8] [--runs 7] [--no-cpu]

GPU: the guide set, an ultralow consensus that folds every guide (made-up RNAfold lines of the real lengths), the real
Bowtie step against the same genome and made-up scores for every guide; then issl_results_build several times, warm, with
the library's own HIP events around its three launches (issl_results_times): the median of measure + scan + emit, the
bytes written and the resulting GB/s; the same with sgrnascorer2score forced to '?' (ISSL_RESULTS_NO_SGRNA) and with every
row stored directly (ISSL_RESULTS_DIRECT), the variants alternating run by run; and the host clock around
issl_results_copy into pageable memory.
CPU: the reference's own method (Crackling.py:845-852) on the same rows held as dicts: csv.writer, one writerow per guide
into a file, timed with the host clock; its bytes must equal the GPU's."""
import argparse
import csv
import ctypes as C
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ORDER = ["seq", "sgrnascorer2score", "header", "start", "end", "strand", "isUnique", "passedG20", "passedTTTT", "passedATPercent",
         "passedSecondaryStructure", "ssL1", "ssStructure", "ssEnergy", "acceptedByMm10db", "acceptedBySgRnaScorer",
         "consensusCount", "passedBowtie", "passedOffTargetScore", "AT", "bowtieChr", "bowtieStart", "bowtieEnd",
         "mitOfftargetscore", "cfdOfftargetscore", "passedAvoidLeadingT"]
SS = (b"G" + b"ACGUACGUACGUACGUACG" + b"GUUUUAGAGCUAGAAAUAGCAAGUUAAAAUAAGGCUAGUCCGUUAUCAACUUGAAAAAGUGGCACCGAGUCGGUGCUUUU",
      b"." * 28 + b"((((....))))...))))" + b"." * 21 + b"((((....))))(((((((...)))))))...", b"-21.30")


def synthetic_genome(mbp, seed=20261019, records=20):
    rng = np.random.default_rng(seed)
    per = int(mbp * 1e6) // records
    parts = []
    for r in range(records):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, per)].tobytes()
        parts.append(b">chr%d synthetic record\n" % (r + 1) + seq + b"\n")
    return b"".join(parts)


def build(ca, gs, c, spans, blob, bowtie, scores, flags):
    from crackling_amd import _lib
    cfg = _lib.ResultsConfig(b",", flags, b"and", 75.0)
    h = C.c_void_p()
    rows, mit, cfd = scores
    ca._lib.check(_lib.lib.issl_results_build(gs._h, c._h, blob, len(blob), spans.ctypes.data, len(spans) // 3,
                                              bowtie.rows_tensor().data_ptr(), bowtie.rows_tensor().shape[0], bowtie.genome._h,
                                              rows.data_ptr(), mit.data_ptr(), cfd.data_ptr(), rows.numel(), C.byref(cfg), C.byref(h)))
    a, b, d = C.c_double(), C.c_double(), C.c_double()
    _lib.lib.issl_results_times(h, C.byref(a), C.byref(b), C.byref(d))
    n_bytes = C.c_uint64()
    _lib.lib.issl_results_info(h, None, C.byref(n_bytes), None)
    return h, {"measure": a.value, "scan": b.value, "emit": d.value}, n_bytes.value


def reference_rows(gs, c, bowtie, scores, genome):
    """The rows as the reference holds them when it writes (a dict per guide, typed as it types them)."""
    guides, rows = gs.guides, c.rows
    n = len(guides)
    code = np.array([0, 1, "?", "!"], dtype=object)
    cols = {k: np.full(n, "?", dtype=object) for k in ORDER}
    cols["seq"] = np.array(gs.strings(), dtype=object)
    uniq = guides["seen"] == 1
    names = np.array([name.decode() for name, _ in gs.records], dtype=object)
    cols["header"] = np.where(uniq, names[guides["record"]], "-")
    cols["start"] = np.where(uniq, np.array([str(x) for x in guides["start"].tolist()], dtype=object), "-")
    cols["end"] = np.where(uniq, np.array([str(x + 23) for x in guides["start"].tolist()], dtype=object), "-")
    cols["strand"] = np.where(uniq, np.where(guides["strand"] == 1, "-", "+"), "-")
    cols["isUnique"] = np.where(uniq, 1, 0).astype(object)
    for f, k in (("g20", "passedG20"), ("lead_t", "passedAvoidLeadingT"), ("at_pct", "passedATPercent"), ("tttt", "passedTTTT"),
                 ("ss", "passedSecondaryStructure"), ("mm10db", "acceptedByMm10db"), ("sgrna", "acceptedBySgRnaScorer")):
        cols[k] = code[rows[f]]
    cols["consensusCount"] = rows["count"].astype(object)
    for f, k in (("at", "AT"), ("sgrna_score", "sgrnascorer2score")):
        v = rows[f].astype(object)
        v[np.isnan(rows[f])] = "?"
        cols[k] = v
    fold = c.fold_rows
    for k, text in zip(("ssL1", "ssStructure", "ssEnergy"), SS):
        cols[k][fold] = text.decode()
    sel, b = c.selected, bowtie.rows
    tested = b["code"] != 2
    at = sel[tested]
    cols["passedBowtie"][at] = b["code"][tested].astype(object)
    chrs = np.array([(name.split() or [b""])[0].decode() for name, _ in genome.records] + ["*"], dtype=object)
    found = b["record"][tested] != 0xFFFFFFFF
    cols["bowtieChr"][at] = chrs[np.where(found, b["record"][tested], len(chrs) - 1)]
    cols["bowtieStart"][at] = np.where(found, b["pos"][tested] + 1, 0).astype(object)
    cols["bowtieEnd"][at] = np.where(found, b["pos"][tested] + 23, 22).astype(object)
    srows, mit, cfd = scores
    mit = np.array([float("%f" % x) for x in mit.tolist()])
    cfd = np.array([float("%f" % x) for x in cfd.tolist()])
    cols["mitOfftargetscore"][srows] = mit.astype(object)
    cols["cfdOfftargetscore"][srows] = cfd.astype(object)
    cols["passedOffTargetScore"][srows] = np.where((mit < 75.0) & (cfd < 75.0), 0, 1).astype(object)
    lists = [cols[k].tolist() for k in ORDER]
    return [dict(zip(ORDER, vals)) for vals in zip(*lists)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "results.json"))
    ap.add_argument("--mbp", type=float, default=8.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    import crackling_amd as ca
    z = np.load(ROOT / "tests" / "golden" / "consensus" / "model.npz")
    blob_fa = synthetic_genome(a.mbp)
    gs = ca.GuideSet.extract([blob_fa])
    genome = ca.Genome.open([blob_fa])
    c = ca.Consensus(gs, optimisation="ultralow", n=2, model=(z["sv"], z["coef"], float(z["intercept"])))
    rng = np.random.default_rng(1)
    folds = np.zeros(c.n_fold, dtype=ca.FOLD_DTYPE)
    folds["energy"], folds["scaffold"], folds["present"] = -21.3, rng.integers(0, 2, c.n_fold), 1
    c.finish(folds)
    bowtie = c.bowtie(genome)
    spans = np.zeros(3 * c.n_fold, dtype=ca.results.TEXT_SPAN_DTYPE)
    at = 0
    for k, text in enumerate(SS):
        spans["offset"][k::3], spans["length"][k::3] = at, len(text)
        at += len(text)
    blob = b"".join(SS)
    srows = c.selected
    mit, cfd = rng.uniform(0, 100, len(srows)), rng.uniform(0, 100, len(srows))
    d_scores = (torch.from_numpy(srows.astype(np.int32)).cuda(), torch.from_numpy(mit).cuda(), torch.from_numpy(cfd).cuda())
    torch.cuda.synchronize()
    from crackling_amd import _lib
    variants = {"staged": 0, "staged_no_sgrna_repr": ca.results.NO_SGRNA, "direct": ca.results.DIRECT}
    times = {k: [] for k in variants}
    n_bytes = {}
    for run in range(a.runs + 1):                                   # run 0 warms every variant up
        for name, flags in variants.items():
            h, t, nb = build(ca, gs, c, spans, blob, bowtie, d_scores, flags)
            _lib.lib.issl_results_close(h)
            n_bytes[name] = nb
            if run:
                times[name].append(t)
    med = {k: {s: statistics.median(t[s] for t in v) for s in ("measure", "scan", "emit")} for k, v in times.items()}
    for v in med.values():
        v["total"] = v["measure"] + v["scan"] + v["emit"]
    h, _, nb = build(ca, gs, c, spans, blob, bowtie, d_scores, 0)
    host = np.empty(nb, dtype=np.uint8)
    copies = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        _lib.lib.issl_results_copy(h, host.ctypes.data, nb)
        copies.append(1e3 * (time.perf_counter() - t0))
    _lib.lib.issl_results_close(h)
    out = {"guides": gs.n_guides, "genome_mbp": a.mbp, "fold_rows": int(c.n_fold), "selected": int(len(srows)), "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "bytes": nb, "bytes_per_row": nb / max(gs.n_guides, 1),
           "gpu_ms_median": med, "gpu_ms_all_runs": times, "gb_per_s": nb / (med["staged"]["total"] * 1e-3) / 1e9,
           "copy_to_host_ms_median": statistics.median(copies), "copy_to_host_ms": copies,
           "emit_fraction_sgrna_repr": 1.0 - med["staged_no_sgrna_repr"]["emit"] / med["staged"]["emit"],
           "bytes_without_sgrna_repr": n_bytes["staged_no_sgrna_repr"]}
    if not a.no_cpu:
        rows = reference_rows(gs, c, bowtie, (srows, mit, cfd), genome)
        with tempfile.TemporaryDirectory() as tmp:
            path = pathlib.Path(tmp) / "guides.txt"
            with open(path, "a+") as fh:
                csv.writer(fh, delimiter=",", quotechar='"', dialect="unix", quoting=csv.QUOTE_MINIMAL).writerow(ORDER)
            t0 = time.perf_counter()
            with open(path, "a+") as fh:                             # Crackling.py:845-852
                w = csv.writer(fh, delimiter=",", quotechar='"', dialect="unix", quoting=csv.QUOTE_MINIMAL)
                for row in rows:
                    w.writerow([row[x] for x in ORDER])
            cpu_s = time.perf_counter() - t0
            same = path.read_bytes() == host.tobytes()
        out.update(cpu_csv_writer_s=cpu_s, cpu_bytes_identical=same, cpu_us_per_field=1e6 * cpu_s / (26 * max(len(rows), 1)),
                   ratio_cpu_over_gpu_device_time=cpu_s / (med["staged"]["total"] * 1e-3),
                   ratio_cpu_over_gpu_with_copy=cpu_s / ((med["staged"]["total"] + statistics.median(copies)) * 1e-3))
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    assert out.get("cpu_bytes_identical", True), "the reference's method wrote other bytes"
    print(json.dumps({k: v for k, v in out.items() if k not in ("gpu_ms_all_runs", "copy_to_host_ms")}))
    c.close()
    genome.close()
    gs.close()


if __name__ == "__main__":
    main()
