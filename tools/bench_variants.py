#!/usr/bin/env python3
"""The variant-aware genome search beside the plain one on DESIGN 5's search workload.

Genome: the seeded repeat genome of tools/genome_index.py (--mbp, default 200).  Queries: --queries guides (default
10 000) read off the genome's own text + NNN, pattern NNNNNNNNNNNNNNNNNNNNNGG, max_dist 4 -- the workload of
`genome_index.py --search`.  On one resident handle, three legs:
  (a) Genome.search                         the plain search, the yardstick
  (b) Genome.search_variants                on the same text, which holds no ambiguity code: the same rows
  (c) Genome.search_variants                after apply_snps() of seeded SNPs, one base in --snp-every (default 300), at
                                            max_variants --max-variants (default 2)
(a) and (b) alternate for --rounds rounds after a warm-up; the host clock is around a call that ends in a device
synchronise (the counting call and the filling call of the rows, as Genome.search* makes them).  Then a second handle
under ISSL_LOCATE_TIMING=1 gives the device stage times of the filling call of each leg, and the rows of (b) are compared
with those of (a), re-encoded.  One JSON document on stdout or in --out."""
import argparse
import json
import os
import pathlib
import re
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import genome_index as gi  # noqa: E402

PATTERN, MAX_DIST = "N" * 21 + "GG", 4


def seeded_snps(ca, genome, every, seed, text_of):
    """One SNP at about one base in `every` of every record: REF as the text has it, one other base as ALT."""
    rng = np.random.default_rng(seed)
    parts = []
    for r, (_, length) in enumerate(genome.records):
        seq = text_of(r)
        pos = np.flatnonzero(rng.random(length) < 1.0 / every)
        code = np.full(256, 4, dtype=np.uint8)
        for k, c in enumerate(b"ACGT"):
            code[c] = k
        ref = code[seq[pos]]
        pos, ref = pos[ref < 4], ref[ref < 4]
        part = np.zeros(len(pos), dtype=ca.SNP_DTYPE)
        part["pos"], part["record"] = pos, r
        part["ref"] = 1 << ref
        part["alt"] = 1 << ((ref + 1 + rng.integers(0, 3, size=len(pos))) % 4)
        parts.append(part)
    return np.concatenate(parts)


def stages_of(err, tag):
    lines = [ln for ln in err.splitlines() if ln.startswith(tag)]
    fill = lines[len(lines) // 2:]  # the filling call's lines (the counting call's come first)
    stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
    ctr = {m.group(1): int(m.group(2)) for ln in fill for m in re.finditer(r"(windows|admitted|hits) (\d+)", ln)}
    return {"filling_call_stages_ms": stages, "device_ms_filling_call": sum(stages.values()), "scan_counters": ctr}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, default=200.0)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--snp-every", type=int, default=300)
    ap.add_argument("--max-variants", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import crackling_amd as ca
    import variant_util as vu
    if not torch.cuda.is_available():
        raise SystemExit("bench_variants.py needs a GPU: it measures nothing without one")

    with tempfile.TemporaryDirectory() as work:
        fa = pathlib.Path(work) / "genome.fa"
        gi.genome(fa, a.mbp, "repeat", a.seed)
        sites = gi.sample_sites(fa, a.queries, a.seed + a.queries)
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[((sites[:, None] >> (2 * np.arange(20, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)]
        pat, q = ca.search_prepare(PATTERN, [bytes(row) + b"NNN" for row in text])
        warm = q[:8]
        recs = [b"".join(r.split(b"\n")[1:]) for r in fa.read_bytes().split(b">")[1:]]  # as sample_sites reads them
        text_of = lambda r: np.frombuffer(recs[r], dtype=np.uint8)

        def timed_call(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t) * 1e3, out

        res = {"genome_mbp": a.mbp, "pattern": PATTERN, "max_dist": MAX_DIST, "queries": int(len(q)), "rounds": a.rounds,
               "device": torch.cuda.get_device_name(0)}
        with ca.Genome.open([str(fa)]) as g:
            res["n_bases"], res["records"] = g.n_bases, len(g.records)
            g.search(pat, warm, MAX_DIST)
            g.search_variants(pat, warm, MAX_DIST, a.max_variants)
            walls = {"a_search": [], "b_search_variants_clean_text": [], "c_search_variants_with_snps": []}
            for _ in range(a.rounds):
                ms, (off_a, rows_a) = timed_call(lambda: g.search(pat, q, MAX_DIST))
                walls["a_search"].append(ms)
                ms, (off_b, rows_b) = timed_call(lambda: g.search_variants(pat, q, MAX_DIST, a.max_variants))
                walls["b_search_variants_clean_text"].append(ms)
            res["rows_a"], res["rows_b"] = int(len(rows_a)), int(len(rows_b))
            res["b_equals_a_reencoded"] = bool(off_a.tobytes() == off_b.tobytes() and rows_b.tobytes() == vu.from_plain(rows_a, 23).tobytes())
            snps = seeded_snps(ca, g, a.snp_every, a.seed, text_of)
            ms, changed = timed_call(lambda: g.apply_snps(snps))
            res["snps"] = {"every": a.snp_every, "entries": int(len(snps)), "changed": int(changed), "apply_wall_ms": ms}
            g.search_variants(pat, warm, MAX_DIST, a.max_variants)
            for _ in range(a.rounds):
                ms, (off_c, rows_c) = timed_call(lambda: g.search_variants(pat, q, MAX_DIST, a.max_variants))
                walls["c_search_variants_with_snps"].append(ms)
            res["rows_c"] = int(len(rows_c))
            res["rows_c_with_variants"] = int((rows_c["n_var"] > 0).sum())
            ms, (_, rows_a2) = timed_call(lambda: g.search(pat, q, MAX_DIST))
            res["rows_a_on_the_text_with_snps"] = int(len(rows_a2))
            res["wall_ms_counting_and_filling_call"] = walls
            res["wall_ms_best"] = {k: min(v) for k, v in walls.items()}
        # the device stage times, on a handle that prints them
        os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when the handle is made
        with ca.Genome.open([str(fa)]) as timed:
            os.environ.pop("ISSL_LOCATE_TIMING")
            gi.stderr_of(lambda: (timed.search(pat, warm, MAX_DIST), timed.search_variants(pat, warm, MAX_DIST, a.max_variants)))
            _, err = gi.stderr_of(lambda: timed.search(pat, q, MAX_DIST))
            res["a_search"] = stages_of(err, "[issl search]")
            _, err = gi.stderr_of(lambda: timed.search_variants(pat, q, MAX_DIST, a.max_variants))
            res["b_search_variants_clean_text"] = stages_of(err, "[issl variants]")
            gi.stderr_of(lambda: timed.apply_snps(snps))
            _, err = gi.stderr_of(lambda: timed.search_variants(pat, q, MAX_DIST, a.max_variants))
            res["c_search_variants_with_snps"] = stages_of(err, "[issl variants]")
        res["b_over_a_device_ms"] = res["b_search_variants_clean_text"]["device_ms_filling_call"] / res["a_search"]["device_ms_filling_call"]
        res["b_over_a_count_stage"] = (res["b_search_variants_clean_text"]["filling_call_stages_ms"]["count"] /
                                       res["a_search"]["filling_call_stages_ms"]["count"])
    doc = json.dumps(res, indent=1)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
