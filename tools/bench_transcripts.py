#!/usr/bin/env python3
"""Transcript hit counts at the scale of a human annotation: 25 sequences, about 200 k transcripts and 1.5 M exons, made
up with a fixed seed.  A record for profiles/transcripts.json, not a pass mark; bench.py does not know of it.

    python tools/bench_transcripts.py --out profiles/transcripts.json [--base FILE] [--reference DIR] [--queries N]

With a GPU: the open, split by the library's own host clock (ISSL_ANNOTATION_TIMING=1: parse, interval merge, device
build up to its synchronise); then N queries through Annotation.hits_device
with events around the call, warm, the median of several runs.  With --reference DIR (a checkout of Crackling): the
reference's process() on the CPU over the same annotation, given only as many rows as it finishes in about a minute.
Each part fills its own section of the JSON; --base names a file whose other sections are kept.  When the reference's
section is there, the GPU's answers to the rows the reference was given are compared with the reference's."""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import pathlib
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_SEQS, GENES_PER_SEQ, SEQ_LEN = 25, 2000, 100_000_000


def synthetic_annotation(seed=7):
    """-> (GFF3 bytes, counts).  Genes of 1..7 transcripts; a transcript takes a random subset of its gene's 4..20 exon
    slots, so transcripts of a gene overlap the way isoforms do."""
    rng = np.random.default_rng(seed)
    lines = []
    n_tr = n_ex = 0
    for s in range(N_SEQS):
        seq = f"chr{s + 1}"
        starts = np.sort(rng.integers(1, SEQ_LEN, GENES_PER_SEQ))
        for g, at in enumerate(starts.tolist()):
            gene = f"g{s}_{g}"
            slots = int(rng.integers(4, 21))
            lens = rng.integers(50, 400, slots)
            gaps = rng.integers(100, 5000, slots)
            a = at + np.cumsum(gaps + lens) - lens
            b = a + lens
            lines.append(f"{seq}\tsynth\tgene\t{at}\t{int(b[-1])}\t.\t+\t.\tID={gene}\n")
            for t in range(int(rng.integers(1, 8))):
                tid = f"{gene}.{t}"
                lines.append(f"{seq}\tsynth\tmRNA\t{at}\t{int(b[-1])}\t.\t+\t.\tID={tid};Parent={gene}\n")
                keep = np.nonzero(rng.random(slots) < 0.62)[0]
                jitter = rng.integers(0, 30, len(keep))
                for k, j in zip(keep.tolist(), jitter.tolist()):
                    lines.append(f"{seq}\tsynth\texon\t{int(a[k]) + j}\t{int(b[k])}\t.\t+\t.\tID={tid}.e{k};Parent={tid}\n")
                n_tr += 1
                n_ex += len(keep)
    return "".join(lines).encode(), {"sequences": N_SEQS, "genes": N_SEQS * GENES_PER_SEQ, "transcripts": n_tr, "exons": n_ex}


def synthetic_queries(n, seed=11):
    """The first k queries are the same for every n: the reference is given a prefix of what the GPU answers."""
    return (np.random.default_rng(seed).integers(0, N_SEQS, n).astype(np.int32),
            np.random.default_rng(seed + 1).integers(1, SEQ_LEN, n).astype(np.int64))


def digest(column):
    import hashlib
    return hashlib.sha256("\n".join(column).encode()).hexdigest()[:16]


def timed_open(ca, blob):
    """Annotation.open under ISSL_ANNOTATION_TIMING=1 -> (annotation, the library's stderr line with the stage times)."""
    os.environ["ISSL_ANNOTATION_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            a = ca.Annotation.open(blob)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return a, tmp.read().decode()


def run_gpu(blob, n_queries, reference=None, runs=7):
    import torch
    import crackling_amd as ca
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    stages, opens = [], []
    for run in range(4):                             # the first open warms the allocator up and is dropped
        t0 = time.perf_counter()
        a, line = timed_open(ca, blob)
        if run:
            opens.append((time.perf_counter() - t0) * 1e3)
            stages.append({k: float(v) for k, v in re.findall(r"(parse|intervals|device build) ([0-9.]+) ms", line)})
        info = a.info
        if run < 3:
            a.close()
    stage = {k: round(statistics.median(x[k] for x in stages), 1) for k in ("parse", "intervals", "device build")}
    seq, start = synthetic_queries(n_queries)
    d_seq, d_start = torch.from_numpy(seq).cuda(), torch.from_numpy(start).cuda()
    d_out = torch.empty((n_queries, 16), dtype=torch.uint8, device="cuda")
    times = []
    for r in range(runs + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        a.hits_device(d_seq, d_start, d_out, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        e1.synchronize()
        if r >= 2:
            times.append(e0.elapsed_time(e1))
    rows = d_out.cpu().numpy().view(ca.TRANSCRIPT_HITS_DTYPE).reshape(-1)
    ms = statistics.median(times)
    out = {"device": torch.cuda.get_device_name(0), "info": info, "open_ms": {"total_median": round(statistics.median(opens), 1), "runs": [round(x, 1) for x in opens], "host_parse": stage["parse"],
                       "host_intervals": stage["intervals"], "device_build": stage["device build"],
                       "device_build_runs": [x["device build"] for x in stages]},
           "queries": n_queries, "query_ms_median": round(ms, 4), "query_ms_runs": [round(x, 4) for x in times],
           "rows_per_second": round(n_queries / (ms * 1e-3)), "rows_with_a_hit": int((rows["hit"] > 0).sum())}
    if reference:                                    # the rows the reference answered are a prefix of these
        k = reference["rows"]
        out["same_as_reference"] = {"rows": k, "equal": digest(ca.format_hits(rows[:k])) == reference["hits_sha256_16"]}
    a.close()
    return out


def run_reference(blob, root, budget_s=60.0):
    path = pathlib.Path(root) / "src" / "crackling" / "utils" / "countHitTranscripts.py"
    spec = importlib.util.spec_from_file_location("reference_countHitTranscripts", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    seq, start = synthetic_queries(100_000)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "a.gff").write_bytes(blob)

        def timed(n):
            (tmp / "c.csv").write_text("seq,bowtieChr,bowtieStart,bowtieEnd\n"
                                       + "".join(f"G,chr{int(s) + 1},{int(p)},{int(p) + 22}\n" for s, p in zip(seq[:n], start[:n])))
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rows = ref.process(str(tmp / "a.gff"), str(tmp / "c.csv"))
            return time.perf_counter() - t0, rows

        load_s, _ = timed(0)
        probe_s, _ = timed(2000)  # long enough to stand out against the spread of the load
        per_row = max((probe_s - load_s) / 2000, 1e-6)
        n = int(max(2000, min(len(seq), budget_s / per_row)))
        total_s, rows = timed(n)
    return {"load_annotation_s": round(load_s, 2), "rows": n, "rows_s": round(total_s - load_s, 2),
            "rows_per_second": round(n / max(total_s - load_s, 1e-9), 2), "rows_with_a_hit": sum(1 for r in rows[1:] if r[-1] != "0/0"),
            "hits_sha256_16": digest([r[-1] for r in rows[1:]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--base")
    ap.add_argument("--reference")
    ap.add_argument("--queries", type=int, default=10_000_000)
    args = ap.parse_args()
    result = json.loads(pathlib.Path(args.base).read_text()) if args.base and pathlib.Path(args.base).exists() else {}
    blob, counts = synthetic_annotation()
    result["annotation"] = dict(counts, bytes=len(blob))
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        gpu = False
    if args.reference:
        result["reference_cpu"] = run_reference(blob, args.reference)
    if gpu:
        result["gpu"] = run_gpu(blob, args.queries, result.get("reference_cpu"))
    if "gpu" in result and "reference_cpu" in result:
        result["rows_per_second_ratio"] = round(result["gpu"]["rows_per_second"] / result["reference_cpu"]["rows_per_second"])
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
