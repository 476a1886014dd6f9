#!/usr/bin/env python3
"""The bulge search on a variant-aware text beside the plain bulge search and beside the expansion it replaces.

Genome: the seeded repeat genome of tools/genome_index.py (--mbp, default 200).  Queries: --queries guides (default
10 000) read off the genome's own text + NNN, pattern NNNNNNNNNNNNNNNNNNNNNGG, span (0, 20), max_dist 4 -- the workload of
`genome_index.py --search --search-bulges`.  For D = R = each of --limits (default 1 2), on one resident handle:
  (a) Genome.search_bulges                  the plain bulge search, the yardstick
  (b) Genome.search_bulges_variants         on the same text, which holds no ambiguity code: the same rows (asserted)
  (c) Genome.search_bulges_variants         after apply_snps() of the seeded SNPs of bench_variants.py (one base in
                                            --snp-every, default 300), at max_variants --max-variants (default 2)
  (d) the expansion (c) replaces            every alignment (b, i) as a derived (pattern, query) set, each a full
                                            Genome.search_variants: 38 sets at D = R = 1, 74 at D = R = 2
(a) and (b) alternate for --rounds rounds after a warm-up on the text without codes, then the SNPs are applied and (c) and
(d) alternate; the host clock is around a call that ends in a device synchronise (the counting call and the filling call
of the rows, as Genome.search* makes them).  Every limit is measured on the clean text before the SNPs go in.  Then a
second handle under ISSL_LOCATE_TIMING=1 gives the device stage times of the filling call of (a), (b) and (c).  The pass
mark is (d) / (c) >= 3 at D = R = 2.  One JSON document on stdout or in --out."""
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

import bench_variants as bv  # noqa: E402
import genome_index as gi  # noqa: E402

PATTERN, MAX_DIST, SPAN, G = "N" * 21 + "GG", 4, (0, 20), 20


def stages_of(err, tag):
    lines = [ln for ln in err.splitlines() if ln.startswith(tag)]
    fill = lines[len(lines) // 2:]  # the filling call's lines (the counting call's come first)
    stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
    ctr = {m.group(1): int(m.group(2)) for ln in fill for m in re.finditer(r"(windows|admitted|rows) (\d+)", ln)}
    return {"filling_call_stages_ms": stages, "device_ms_filling_call": sum(stages.values()), "scan_counters": ctr}


def note(what):
    print("bench_bulge_variants: " + what, file=sys.stderr, flush=True)


def derived_sets(ca, texts, v):
    """Every alignment (b, i) of D = R = v as a prepared (pattern, queries) pair."""
    sets = []
    for b in range(-v, v + 1):
        for i in ([0] if b == 0 else range(1, G) if b > 0 else range(1, G + b)):
            cut = SPAN[0] + i
            derive = (lambda t: t[:cut] + "N" * b + t[cut:]) if b >= 0 else (lambda t: t[:cut] + t[cut - b:])
            sets.append(ca.search_prepare(derive(PATTERN), [derive(t) for t in texts]))
    return sets


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, default=200.0)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--limits", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--snp-every", type=int, default=300)
    ap.add_argument("--max-variants", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import crackling_amd as ca
    import bulge_variant_util as bvu
    if not torch.cuda.is_available():
        raise SystemExit("bench_bulge_variants.py needs a GPU: it measures nothing without one")
    mv = a.max_variants

    with tempfile.TemporaryDirectory() as work:
        fa = pathlib.Path(work) / "genome.fa"
        gi.genome(fa, a.mbp, "repeat", a.seed)
        sites = gi.sample_sites(fa, a.queries, a.seed + a.queries)
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[((sites[:, None] >> (2 * np.arange(20, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)]
        texts = [bytes(row).decode() + "NNN" for row in text]
        pat, q = ca.search_prepare(PATTERN, texts)
        warm = q[:8]
        recs = [b"".join(r.split(b"\n")[1:]) for r in fa.read_bytes().split(b">")[1:]]  # as sample_sites reads them
        text_of = lambda r: np.frombuffer(recs[r], dtype=np.uint8)
        sets = {v: derived_sets(ca, texts, v) for v in a.limits}
        note("genome and %d queries ready" % len(q))

        def timed_call(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t) * 1e3, out

        res = {"genome_mbp": a.mbp, "pattern": PATTERN, "span": list(SPAN), "max_dist": MAX_DIST, "max_variants": mv,
               "queries": int(len(q)), "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "pass_mark_at_two_bases": 3.0,
               "limits": {}}
        legs = {v: {"a_search_bulges": [], "b_search_bulges_variants_clean_text": [], "c_search_bulges_variants_with_snps": [],
                    "d_expansion_search_variants": []} for v in a.limits}
        with ca.Genome.open([str(fa)]) as g:
            res["n_bases"], res["records"] = g.n_bases, len(g.records)
            g.search_bulges(pat, warm, SPAN, MAX_DIST, 1, 1)
            g.search_bulges_variants(pat, warm, SPAN, MAX_DIST, 1, 1, mv)
            g.search_variants(pat, warm, MAX_DIST, mv)
            for v in a.limits:
                out = res["limits"][v] = {"max_dna": v, "max_rna": v, "expansion_sets": len(sets[v])}
                for _ in range(a.rounds):
                    ms, (off_a, rows_a) = timed_call(lambda: g.search_bulges(pat, q, SPAN, MAX_DIST, v, v))
                    legs[v]["a_search_bulges"].append(ms)
                    ms, (off_b, rows_b) = timed_call(lambda: g.search_bulges_variants(pat, q, SPAN, MAX_DIST, v, v, mv))
                    legs[v]["b_search_bulges_variants_clean_text"].append(ms)
                out["rows_a"], out["rows_b"] = int(len(rows_a)), int(len(rows_b))
                same = off_a.tobytes() == off_b.tobytes() and rows_b.tobytes() == bvu.from_bulges(rows_a, 23).tobytes()
                assert same, "the rows of (b) differ from those of (a), re-encoded"
                out["b_equals_a_reencoded"] = bool(same)
                note("D = R = %d: (a) and (b) done, %d rows" % (v, len(rows_b)))
                del rows_a, rows_b
            snps = bv.seeded_snps(ca, g, a.snp_every, a.seed, text_of)
            ms, changed = timed_call(lambda: g.apply_snps(snps))
            res["snps"] = {"every": a.snp_every, "entries": int(len(snps)), "changed": int(changed), "apply_wall_ms": ms}
            g.search_bulges_variants(pat, warm, SPAN, MAX_DIST, 1, 1, mv)
            for v in a.limits:
                out = res["limits"][v]
                for _ in range(a.rounds):
                    ms, (off_c, rows_c) = timed_call(lambda: g.search_bulges_variants(pat, q, SPAN, MAX_DIST, v, v, mv))
                    legs[v]["c_search_bulges_variants_with_snps"].append(ms)
                    ms, hits = timed_call(lambda: sum(len(g.search_variants(p, dq, MAX_DIST, mv)[1]) for p, dq in sets[v]))
                    legs[v]["d_expansion_search_variants"].append(ms)
                out["rows_c"], out["rows_c_over_a_code"] = int(len(rows_c)), int((rows_c["n_var"] > 0).sum())
                out["expansion_hits_before_merging"] = int(hits)
                _, rows_a2 = g.search_bulges(pat, q, SPAN, MAX_DIST, v, v)
                out["rows_a_on_the_text_with_snps"] = int(len(rows_a2))
                note("D = R = %d: (c) and (d) done, %d rows" % (v, len(rows_c)))
                del rows_c, rows_a2
                walls = legs[v]
                out["wall_ms_counting_and_filling_call"] = walls
                out["wall_ms_best"] = {k: min(w) for k, w in walls.items()}
                out["b_over_a_wall"] = min(walls["b_search_bulges_variants_clean_text"]) / min(walls["a_search_bulges"])
                out["d_over_c_wall"] = min(walls["d_expansion_search_variants"]) / min(walls["c_search_bulges_variants_with_snps"])
        # the device stage times, on a handle that prints them
        os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when the handle is made
        with ca.Genome.open([str(fa)]) as timed:
            os.environ.pop("ISSL_LOCATE_TIMING")
            gi.stderr_of(lambda: (timed.search_bulges(pat, warm, SPAN, MAX_DIST, 1, 1), timed.search_bulges_variants(pat, warm, SPAN, MAX_DIST, 1, 1, mv)))
            for v in a.limits:
                out = res["limits"][v]
                _, err = gi.stderr_of(lambda: timed.search_bulges(pat, q, SPAN, MAX_DIST, v, v))
                out["a_search_bulges"] = stages_of(err, "[issl bulges]")
                _, err = gi.stderr_of(lambda: timed.search_bulges_variants(pat, q, SPAN, MAX_DIST, v, v, mv))
                out["b_search_bulges_variants_clean_text"] = stages_of(err, "[issl bulges+variants]")
                out["b_over_a_device_ms"] = out["b_search_bulges_variants_clean_text"]["device_ms_filling_call"] / out["a_search_bulges"]["device_ms_filling_call"]
                out["b_over_a_count_stage"] = (out["b_search_bulges_variants_clean_text"]["filling_call_stages_ms"]["count"] /
                                               out["a_search_bulges"]["filling_call_stages_ms"]["count"])
            gi.stderr_of(lambda: timed.apply_snps(snps))
            for v in a.limits:
                _, err = gi.stderr_of(lambda: timed.search_bulges_variants(pat, q, SPAN, MAX_DIST, v, v, mv))
                res["limits"][v]["c_search_bulges_variants_with_snps"] = stages_of(err, "[issl bulges+variants]")
        if 2 in res["limits"]:
            res["pass_mark_met"] = bool(res["limits"][2]["d_over_c_wall"] >= res["pass_mark_at_two_bases"])
    doc = json.dumps(res, indent=1)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
