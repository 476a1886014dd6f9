#!/usr/bin/env python3
"""Genome FASTA -> ready-to-score index on one MI355X, stage by stage, against the two-program chain.

A seeded synthetic genome (generated here, nothing downloaded) of --mbp million bases:
  uniform  i.i.d. bases;
  repeat   i.i.d. bases with 10 % of the genome made of mutated copies of 64 interspersed 300-bp elements and one
           23-mer (N20 + NGG) repeated 200 000 times.
The fused path (IsslIndex.build_from_fasta, in this process) is timed per stage with ISSL_UPLOAD_TIMING=1, which
synchronises the device at every boundary: parse (host FASTA pass), upload, match, sort, collapse, build (image), then
the file write (up to --write-max-mbp); free HBM is sampled every 5 ms for the high-water mark.  The chain (bin/extractOfftargets sites.txt,
then bin/isslCreateIndex sites.txt 20 W) runs as the two processes a user runs, on the same file, up to --chain-max-mbp;
its .issl must be byte-identical.  Prints one JSON object per genome size (and writes them to --out).

--locate: instead of the chain, the genome is opened as a resident crackling_amd.Genome and --locate-sites query sites
(forward sites read off the genome's own text at seeded positions) are located: wall time of Genome.locate (its counting
call and its filling call) on a handle without timing, and, on a handle made under ISSL_LOCATE_TIMING=1, the stage times
(prep, count, emit, sort, offsets, finish) and the scan's counters (matches, those the filter let through, hits) of the
filling call.  The yardstick beside them is the `match` stage of the fused build on the same genome.

--guides: instead of the chain, the candidate guides of the genome are extracted (crackling_amd.GuideSet.extract): wall
time to a resident set without timing, then once more under ISSL_GUIDES_TIMING=1 for the stage times (parse on the host;
upload, count, emit, sort, runs, order, finish on the device) with free HBM sampled for the high-water mark per match.
The yardstick is `match` + `sort` of the fused build in the same run: it reads the same text twice and sorts a
comparable number of 64-bit words; the ratio of the device stages behind the upload to it is reported.

--search: instead of the chain, the genome is opened as a resident crackling_amd.Genome under ISSL_LOCATE_TIMING=1 and
--search-queries queries (guide + NNN, the guides read off the genome's own text at seeded positions) are searched under
the pattern NNNNNNNNNNNNNNNNNNNNNGG with max_dist 4: the stage times of the filling call (count, emit, sort, offsets,
finish), the scan's counters (windows, window-strands the pattern admits, hits), windows per second of the count pass and
comparisons per second (admitted window-strands x queries / count time).  Two yardsticks from the same run: the `match`
stage of the fused build, which reads the same bytes twice (count + emit over it for the smallest query count), and the
vector-issue bound of the compare loop -- --search-valu wave64 VALU instructions per 64 comparisons (read off the code
object: tools/isa_stats.py k_search --dump) at 2 cycles each on 1024 SIMDs at 2.4 GHz, the rate DESIGN 3.1 uses for
k_scan -- for the largest.  With --search-bulges V ... the largest query set is also searched with bulges (Genome.search_bulges,
span (0, 20), D = R = V) and, as the yardstick, through the variant expansion: every alignment (b, i) as a derived
(pattern, query) set, each a full Genome.search (74 sets at V = 2).  Both on the same handle without timing, alternating
after one warm-up each; stage times, rows, windows and comparisons per second of the count pass come from one more call
on the timed handle, --bulge-valu is read off tools/isa_stats.py k_bulge.

--haplotypes: instead of the chain, the genome is opened under ISSL_LOCATE_TIMING=1, the seeded SNPs of
tools/bench_variants.py (one base in 300) are applied, and --haplotype-indels seeded indels (default 100 000: deletions
and insertions of 1 to 10 bases behind an anchor, spread over the records) become a crackling_amd.Haplotypes for windows
of 23: the device times of the open (check, upload, build).  Then the largest of --search-queries (guide + NNN,
NNNNNNNNNNNNNNNNNNNNNGG, max_dist 4, max_variants 2) is searched on the strips and, in the same run, with
Genome.search_variants on the reference text: stage times and counters of both filling calls, and the figure to read --
device time per admitted window-strand on the strips over the same quotient on the reference text."""
import argparse
import filecmp
import json
import os
import pathlib
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def genome(path, mbp, kind, seed, records=24):
    """Write the FASTA; returns its size in bytes.  Generated 64 Mbp at a time (bounded host memory at any size)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    elements = [acgt[rng.integers(0, 4, size=300, dtype=np.uint8)] for _ in range(64)]
    unit = np.frombuffer(b"GATTACAGATTACAGATTACCGG", dtype=np.uint8)
    total = int(mbp * 1e6)
    per = total // records
    with open(path, "wb") as fh:
        for r in range(records):
            fh.write(b">chr%d synthetic %s seed %d\n" % (r, kind.encode(), seed))
            left = per
            while left:
                n = min(left, 64 << 20)
                s = acgt[rng.integers(0, 4, size=n, dtype=np.uint8)]
                if kind == "repeat":
                    for at in rng.integers(0, max(n - 300, 1), size=n // 3000):   # 10 % of the bases
                        e = elements[int(rng.integers(0, 64))].copy()
                        mut = rng.random(300) < 0.02
                        e[mut] = acgt[rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)]
                        s[at:at + 300] = e[: n - at]
                    if r == 0 and left == per:
                        rep = np.tile(unit, min(200_000, n // 23 // 2))
                        s[: len(rep)] = rep
                left -= n
                line = s[: n - n % 60].reshape(-1, 60)
                fh.write(np.hstack([line, np.full((len(line), 1), 10, np.uint8)]).tobytes())
                if n % 60:
                    fh.write(s[n - n % 60:].tobytes() + b"\n")
    return os.path.getsize(path)


class HbmWatch:
    def __init__(self, torch):
        self.torch = torch

    def __enter__(self):
        self.torch.cuda.synchronize()
        self.before = self.torch.cuda.mem_get_info(0)[0]
        self.low = self.before
        self.stop = threading.Event()

        def watch():
            while not self.stop.is_set():
                self.low = min(self.low, self.torch.cuda.mem_get_info(0)[0])
                self.stop.wait(0.005)
        self.t = threading.Thread(target=watch, daemon=True)
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.t.join()

    @property
    def peak(self):
        return self.before - self.low


def stderr_of(fn):
    """Run fn() with fd 2 redirected to a file; returns (result, captured text)."""
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def sample_sites(fa, n, seed):
    """n distinct packed forward sites ([ACG][ACGT]{19}[ACGT][AG]G at the sampled start) from the records of the FASTA,
    as the site table holds them (a site named k times would get its list k times: the repeated 23-mer alone has 200 000
    locations)."""
    rng = np.random.default_rng(seed)
    code = np.full(256, 4, dtype=np.uint8)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    recs = [b"".join(r.split(b"\n")[1:]) for r in pathlib.Path(fa).read_bytes().split(b">")[1:]]
    out = []
    per = -(-n // len(recs)) * 2
    for rec in recs:
        c = code[np.frombuffer(rec, dtype=np.uint8)]
        at = rng.integers(0, len(c) - 23, size=per * 16)
        ok = (c[at] < 3) & ((c[at + 21] == 0) | (c[at + 21] == 2)) & (c[at + 22] == 2)
        at = at[ok][:per]
        sig = np.zeros(len(at), dtype=np.uint64)
        for p in range(20):
            ok_p = c[at + p]
            sig |= ok_p.astype(np.uint64) << np.uint64(2 * p)
        out.append(sig)
    return rng.permutation(np.unique(np.concatenate(out)))[:n]


def locate_leg(fa, n_sites, seed):
    import crackling_amd as ca
    res = []
    t = time.perf_counter()
    plain = ca.Genome.open([str(fa)])
    open_s = time.perf_counter() - t
    os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when the handle is made
    timed = ca.Genome.open([str(fa)])
    os.environ.pop("ISSL_LOCATE_TIMING")
    plain.locate(sample_sites(fa, 64, seed))  # code objects
    for n in n_sites:
        sites = sample_sites(fa, n, seed + n)
        t = time.perf_counter()
        offsets, locs = plain.locate(sites)
        wall = time.perf_counter() - t
        _, err = stderr_of(lambda: timed.locate(sites))
        lines = [ln for ln in err.splitlines() if ln.startswith("[issl locate]")]
        fill = lines[len(lines) // 2:]   # the filling call's lines (the counting call's come first)
        stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
        ctr = {m.group(1).replace(" ", "_"): int(m.group(2)) for ln in fill
               for m in re.finditer(r"(matches|filter passed|hits|locations) (\d+)", ln)}
        res.append({"query_sites": int(n), "distinct_query_sites": int(len(np.unique(sites))), "locations": int(len(locs)),
                    "locate_wall_ms_counting_and_filling_call": wall * 1e3, "filling_call_stages_ms": stages,
                    "scan_counters": ctr, "filter_pass_rate": ctr.get("filter_passed", 0) / max(ctr.get("matches", 1), 1)})
    plain.close()
    timed.close()
    return {"open_s": open_s, "n_bases": plain.n_bases, "records": len(plain.records), "queries": res}


def search_leg(fa, n_queries, seed, valu_per_compare, bulges=None):
    import crackling_amd as ca
    pattern, max_dist = "N" * 21 + "GG", 4
    os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when the handle is made
    timed = ca.Genome.open([str(fa)])
    os.environ.pop("ISSL_LOCATE_TIMING")

    def queries_of(n, s):
        sites = sample_sites(fa, n, s)
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[((sites[:, None] >> (2 * np.arange(20, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)]
        return ca.search_prepare(pattern, [bytes(row) + b"NNN" for row in text])

    stderr_of(lambda: timed.search(*queries_of(8, seed), max_dist))  # code objects
    bound = 1024 * 2.4e9 / (2 * valu_per_compare) * 64  # comparisons per second at the vector-issue rate of DESIGN 3.1
    res = []
    for n in n_queries:
        pat, q = queries_of(n, seed + n)
        t = time.perf_counter()
        (offsets, hits), err = stderr_of(lambda: timed.search(pat, q, max_dist))
        wall = time.perf_counter() - t
        lines = [ln for ln in err.splitlines() if ln.startswith("[issl search]")]
        fill = lines[len(lines) // 2:]   # the filling call's lines (the counting call's come first)
        stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
        ctr = {m.group(1): int(m.group(2)) for ln in fill for m in re.finditer(r"(windows|admitted|hits) (\d+)", ln)}
        count_s = stages["count"] / 1e3
        comparisons = ctr["admitted"] * len(q)
        res.append({"queries": int(len(q)), "hits": int(len(hits)), "wall_ms_counting_and_filling_call_timed_handle": wall * 1e3,
                    "filling_call_stages_ms": stages, "scan_counters": ctr, "windows_per_s_count_pass": ctr["windows"] / count_s,
                    "comparisons": comparisons, "comparisons_per_s_count_pass": comparisons / count_s,
                    "fraction_of_vector_issue_bound": comparisons / count_s / bound})
    out = {"pattern": pattern, "max_dist": max_dist, "n_bases": timed.n_bases, "records": len(timed.records),
           "valu_per_64_comparisons": valu_per_compare, "vector_issue_bound_comparisons_per_s": bound, "runs": res}
    if bulges:
        out["bulges"] = bulge_leg(ca, fa, timed, pattern, max_dist, queries_of(max(n_queries), seed + max(n_queries)), *bulges)
    timed.close()
    return out


def bulge_leg(ca, fa, timed, pattern, max_dist, prepared, limits, valu_per_compare, rounds=2):
    """Genome.search_bulges at D = R = v for every v of `limits`, span (0, 20), against the variant expansion: every
    alignment (b, i) as a derived (pattern, query) set, each a full Genome.search.  Both on a handle without timing, the
    derived texts prepared beforehand, one warm-up each, then `rounds` rounds alternating; the stage times and counters
    come from one more call on the timed handle."""
    span, G, (pat, q) = (0, 20), 20, prepared
    texts = ["".join("ACGT"[(int(s) >> (2 * i)) & 3] if (int(c) >> (2 * i)) & 3 else "N" for i in range(len(pattern)))
             for s, c in zip(q["sig"], q["care"])]
    plain = ca.Genome.open([str(fa)])
    res = []
    for v in limits:
        sets = []
        for b in range(-v, v + 1):
            for i in ([0] if b == 0 else range(1, G) if b > 0 else range(1, G + b)):
                cut = span[0] + i
                derive = (lambda t: t[:cut] + "N" * b + t[cut:]) if b >= 0 else (lambda t: t[:cut] + t[cut - b:])
                sets.append(ca.search_prepare(derive(pattern), [derive(t) for t in texts]))
        bound = 1024 * 2.4e9 / (2 * valu_per_compare) * 64

        def new_path():
            t = time.perf_counter()
            offsets, rows = plain.search_bulges(pat, q, span, max_dist, v, v)
            return time.perf_counter() - t, len(rows)

        def expansion():
            t = time.perf_counter()
            hits = sum(len(plain.search(p, dq, max_dist)[1]) for p, dq in sets)
            return time.perf_counter() - t, hits

        new_path(), expansion()  # one warm-up each
        walls = {"search_bulges": [], "expansion": []}
        rows = hits = 0
        for _ in range(rounds):
            w, rows = new_path()
            walls["search_bulges"].append(w * 1e3)
            w, hits = expansion()
            walls["expansion"].append(w * 1e3)
        _, err = stderr_of(lambda: timed.search_bulges(pat, q, span, max_dist, v, v))
        lines = [ln for ln in err.splitlines() if ln.startswith("[issl bulges]")]
        fill = lines[len(lines) // 2:]   # the filling call's lines (the counting call's come first)
        stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
        ctr = {m.group(1): int(m.group(2)) for ln in fill for m in re.finditer(r"(windows|admitted|rows) (\d+)", ln)}
        count_s = stages["count"] / 1e3
        comparisons = ctr["admitted"] * len(q)
        ratio = min(walls["expansion"]) / min(walls["search_bulges"])
        res.append({"max_dna": v, "max_rna": v, "span": list(span), "queries": int(len(q)), "rows": int(rows),
                    "expansion_sets": len(sets), "expansion_hits_before_merging": int(hits),
                    "wall_ms_counting_and_filling_call": walls, "expansion_over_search_bulges_best_of_rounds": ratio,
                    "pass_mark_at_two_bases": 3.0, "filling_call_stages_ms": stages, "scan_counters": ctr,
                    "windows_per_s_count_pass": ctr["windows"] / count_s, "comparisons": comparisons,
                    "comparisons_per_s_count_pass": comparisons / count_s, "valu_per_64_comparisons": valu_per_compare,
                    "fraction_of_vector_issue_bound": comparisons / count_s / bound})
    plain.close()
    return res


def haplotypes_leg(fa, n_indels, n_queries, seed, window=23, max_variants=2):
    import crackling_amd as ca
    sys.path.insert(0, str(ROOT / "tools"))
    import bench_variants as bv
    pattern, max_dist = "N" * 21 + "GG", 4
    os.environ["ISSL_LOCATE_TIMING"] = "1"   # read when a handle is made
    timed = ca.Genome.open([str(fa)])
    recs = [b"".join(r.split(b"\n")[1:]) for r in pathlib.Path(fa).read_bytes().split(b">")[1:]]  # as sample_sites reads them
    snps = bv.seeded_snps(ca, timed, 300, seed, lambda r: np.frombuffer(recs[r], dtype=np.uint8))
    changed = timed.apply_snps(snps)
    # the indels: REF as the reference has it (a code an applied SNP left there holds it), half deletions, half insertions
    rng = np.random.default_rng(seed + 1)
    indels = np.zeros(n_indels, dtype=ca.INDEL_DTYPE)
    alleles, at = [], 0
    per = -(-n_indels // len(recs))
    k = 0
    for r, rec in enumerate(recs):
        for pos in np.sort(rng.choice(len(rec) - 16, size=min(per, n_indels - k), replace=False)):
            pos, size = int(pos), int(rng.integers(1, 11))
            if k % 2:
                ref, alt = rec[pos:pos + 1 + size], rec[pos:pos + 1]
            else:
                ref, alt = rec[pos:pos + 1], rec[pos:pos + 1] + bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=size))
            indels[k] = (pos, r, len(ref), len(alt), at, at + len(ref), 0)
            alleles.append(ref + alt)
            at += len(ref) + len(alt)
            k += 1
    alleles = b"".join(alleles)
    sites = sample_sites(fa, n_queries, seed + n_queries)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[((sites[:, None] >> (2 * np.arange(20, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)]
    pat, q = ca.search_prepare(pattern, [bytes(row) + b"NNN" for row in text])

    def stages_of(err, tag):
        lines = [ln for ln in err.splitlines() if ln.startswith(tag)]
        fill = lines[len(lines) // 2:]   # the filling call's lines (the counting call's come first)
        stages = {m.group(1): float(m.group(2)) for ln in fill for m in re.finditer(r" (\w+) ([0-9.]+) ms", ln)}
        ctr = {m.group(1): int(m.group(2)) for ln in fill for m in re.finditer(r"(windows|admitted|hits) (\d+)", ln)}
        return {"filling_call_stages_ms": stages, "device_ms_filling_call": sum(stages.values()), "scan_counters": ctr}

    stderr_of(lambda: timed.haplotypes(indels[:64], alleles, window).close())  # code objects
    t = time.perf_counter()
    h, err = stderr_of(lambda: timed.haplotypes(indels, alleles, window))
    open_wall = time.perf_counter() - t
    os.environ.pop("ISSL_LOCATE_TIMING")
    line = [ln for ln in err.splitlines() if ln.startswith("[issl haplotypes]")][-1]
    open_stages = {m.group(1): float(m.group(2)) for m in re.finditer(r" (\w+) ([0-9.]+) ms", line)}
    stderr_of(lambda: (h.search(pat, q[:8], max_dist, max_variants), timed.search_variants(pat, q[:8], max_dist, max_variants)))
    t = time.perf_counter()
    (_, rows), err = stderr_of(lambda: h.search(pat, q, max_dist, max_variants))
    strips_wall = time.perf_counter() - t
    strips = stages_of(err, "[issl variants]")
    strips["map_ms"] = [float(m.group(1)) for m in re.finditer(r"\[issl haplotypes\] map ([0-9.]+) ms", err)][-1] if len(rows) else 0.0
    t = time.perf_counter()
    (_, ref_rows), err = stderr_of(lambda: timed.search_variants(pat, q, max_dist, max_variants))
    ref_wall = time.perf_counter() - t
    ref = stages_of(err, "[issl variants]")
    info = h.info()
    h.close()
    timed.close()

    def per_admitted(leg, stage=None):
        ms = leg["filling_call_stages_ms"][stage] if stage else leg["device_ms_filling_call"]
        return ms * 1e6 / max(leg["scan_counters"]["admitted"], 1)   # ns

    return {"pattern": pattern, "max_dist": max_dist, "max_variants": max_variants, "window": window, "queries": int(len(q)),
            "n_bases": timed.n_bases, "records": len(recs), "snps_applied": int(changed), "indels": int(n_indels),
            "strip_text_bytes": info["text_bytes"], "open_wall_ms": open_wall * 1e3, "open_device_stages_ms": open_stages,
            "strips": dict(strips, rows=int(len(rows)), wall_ms_counting_and_filling_call=strips_wall * 1e3),
            "reference_text": dict(ref, rows=int(len(ref_rows)), wall_ms_counting_and_filling_call=ref_wall * 1e3),
            "ns_per_admitted_window_strand": {"strips_count_stage": per_admitted(strips, "count"), "reference_count_stage": per_admitted(ref, "count"),
                                              "strips_device": per_admitted(strips), "reference_device": per_admitted(ref)},
            "strips_over_reference_per_admitted_window_strand": {"count_stage": per_admitted(strips, "count") / per_admitted(ref, "count"),
                                                                 "device": per_admitted(strips) / per_admitted(ref)}}


def guides_leg(fa, torch):
    import crackling_amd as ca
    ca.GuideSet.extract([b">w\n" + b"ACGTTGCAGGTACCAGTAGGCAGG" * 100 + b"\n"]).close()   # code objects
    t = time.perf_counter()
    plain = ca.GuideSet.extract([str(fa)])
    wall = time.perf_counter() - t
    n_guides, n_unique, n_matches, n_records = plain.n_guides, plain.n_unique, plain.n_matches, len(plain.records)
    plain.close()
    os.environ["ISSL_GUIDES_TIMING"] = "1"   # read when the call starts
    with HbmWatch(torch) as hbm:
        timed, err = stderr_of(lambda: ca.GuideSet.extract([str(fa)]))
    os.environ.pop("ISSL_GUIDES_TIMING")
    resident = hbm.before - torch.cuda.mem_get_info(0)[0]
    timed.close()
    line = [ln for ln in err.splitlines() if ln.startswith("[issl guides]")][-1]
    stages = {m.group(1): float(m.group(2)) for m in re.finditer(r" (\w+) ([0-9.]+) ms", line)}
    device = sum(v for k, v in stages.items() if k not in ("parse", "upload"))
    return {"wall_s_to_resident_set": wall, "stages_ms": stages, "device_stages_ms_without_upload": device, "matches": n_matches,
            "guides": n_guides, "unique": n_unique, "records": n_records, "hbm_high_water_bytes": hbm.peak,
            "hbm_high_water_per_match": hbm.peak / max(n_matches, 1), "resident_bytes_of_the_set": resident}


def run(mbp, kind, seed, width, work, chain_max_mbp, write_max_mbp, timeout, locate_sites=None, guides=False, search=None, haplotypes=None):
    import torch
    import crackling_amd as ca
    fa = work / f"genome_{kind}_{mbp:g}.fa"
    t = time.perf_counter()
    fa_bytes = genome(fa, mbp, kind, seed)
    res = {"genome_mbp": mbp, "kind": kind, "seed": seed, "slice_width": width, "fasta_bytes": fa_bytes,
           "generate_s": time.perf_counter() - t}
    if haplotypes:   # (no index is built: the handle's text is all this leg reads)
        res["haplotypes"] = haplotypes_leg(fa, haplotypes[0], haplotypes[1], seed)
        fa.unlink()
        return res
    os.environ["ISSL_UPLOAD_TIMING"] = "1"   # read when the call starts (Tuning::from_env)
    with HbmWatch(torch) as hbm:
        t = time.perf_counter()
        ix, err = stderr_of(lambda: ca.IsslIndex.build_from_fasta([str(fa)], slice_width=width))
        fused_s = time.perf_counter() - t
    os.environ.pop("ISSL_UPLOAD_TIMING")
    stages = {m.group(1): float(m.group(2)) / 1e3 for m in re.finditer(r"\[issl genome\] (\w+) ([0-9.]+) ms", err)}
    out = work / "fused.issl"
    if mbp <= max(write_max_mbp, chain_max_mbp):
        t = time.perf_counter()
        ix.write(out)
        stages["write"] = time.perf_counter() - t
    hd = ix.header
    res.update({"raw_sites": hd["n_lines"], "distinct_sites": hd["n_sites"], "image_bytes": ix.device_bytes(),
                "fused": {"stages_s": stages, "to_resident_handle_s": fused_s, "hbm_high_water_bytes": hbm.peak,
                          "hbm_high_water_per_raw_site": hbm.peak / max(hd["n_lines"], 1),
                          "upload_notes": [ln for ln in err.splitlines() if ln.startswith("[issl upload]")]}})
    ix.close()
    if locate_sites:
        res["locate"] = locate_leg(fa, locate_sites, seed)
        res["locate"]["yardstick_match_stage_ms"] = stages.get("match", 0.0) * 1e3
        res["chain"] = "not run with --locate"
    elif search:
        res["search"] = search_leg(fa, search[0], seed, search[1], search[2])
        match_ms = stages.get("match", 0.0) * 1e3
        first = res["search"]["runs"][0]["filling_call_stages_ms"]
        res["search"]["yardstick_match_stage_ms"] = match_ms
        res["search"]["count_plus_emit_over_match_stage_smallest_query_count"] = (first["count"] + first.get("emit", 0.0)) / max(match_ms, 1e-9)
        res["chain"] = "not run with --search"
    elif guides:
        res["guides"] = guides_leg(fa, torch)
        yard = (stages.get("match", 0.0) + stages.get("sort", 0.0)) * 1e3
        res["guides"]["yardstick_match_plus_sort_ms"] = yard
        res["guides"]["device_stages_over_yardstick"] = res["guides"]["device_stages_ms_without_upload"] / max(yard, 1e-9)
        res["chain"] = "not run with --guides"
    elif mbp <= chain_max_mbp:
        sites = work / "sites.txt"
        chain_issl = work / "chain.issl"
        t = time.perf_counter()
        subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(sites), str(fa)], check=True, capture_output=True,
                       timeout=timeout)
        t_extract = time.perf_counter() - t
        t = time.perf_counter()
        subprocess.run([str(ROOT / "bin" / "isslCreateIndex"), str(sites), "20", str(width), str(chain_issl)], check=True,
                       capture_output=True, timeout=timeout)
        t_create = time.perf_counter() - t
        res["chain"] = {"extractOfftargets_s": t_extract, "isslCreateIndex_s": t_create, "text_bytes": sites.stat().st_size,
                        "total_s": t_extract + t_create,
                        "identical_issl": filecmp.cmp(chain_issl, out, shallow=False)}
        sites.unlink()
        chain_issl.unlink()
    else:
        res["chain"] = f"not run above {chain_max_mbp:g} Mbp (--chain-max-mbp)"
    out.unlink(missing_ok=True)
    fa.unlink()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mbp", type=float, nargs="+", default=[200.0])
    ap.add_argument("--kind", choices=["uniform", "repeat"], default="repeat")
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--chain-max-mbp", type=float, default=1000.0)
    ap.add_argument("--write-max-mbp", type=float, default=1000.0, help="time the .issl write up to this size (~48 B per site on disk)")
    ap.add_argument("--timeout", type=float, default=900.0, help="time limit of each chain process (s)")
    ap.add_argument("--locate", action="store_true", help="locate query sites in the resident genome instead of running the chain")
    ap.add_argument("--locate-sites", type=int, nargs="+", default=[1000, 1000000])
    ap.add_argument("--guides", action="store_true", help="extract the candidate guides of the genome instead of running the chain")
    ap.add_argument("--search", action="store_true", help="search queries in the resident genome (any-PAM search) instead of running the chain")
    ap.add_argument("--search-queries", type=int, nargs="+", default=[1, 100, 10000])
    ap.add_argument("--search-valu", type=float, default=10.0, help="wave64 VALU instructions per 64 comparisons in k_search's compare loop")
    ap.add_argument("--search-bulges", type=int, nargs="*", default=[], help="with --search: also Genome.search_bulges at D = R = each of these "
                    "limits for the largest query count, against the variant expansion through Genome.search")
    ap.add_argument("--bulge-valu", type=float, default=12.75, help="wave64 VALU instructions per 64 comparisons in k_bulge's compare loop")
    ap.add_argument("--haplotypes", action="store_true", help="the ALT haplotypes of seeded indels: the open's device times, and the search on the "
                    "strips beside the variant search on the reference text, instead of running the chain")
    ap.add_argument("--haplotype-indels", type=int, default=100000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import crackling_amd as ca
    torch.cuda.init()
    torch.zeros(1, device="cuda:0")
    ca.IsslIndex.build_from_fasta([b">w\n" + b"ACGTTGCAGGTACCAGTAGGCAGG" * 100 + b"\n"]).close()   # runtime + code objects
    results = []
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        for mbp in a.mbp:
            no_chain = a.locate or a.guides or a.search or a.haplotypes
            r = run(mbp, a.kind, a.seed, a.width, pathlib.Path(tmp), 0.0 if no_chain else a.chain_max_mbp, 0.0 if no_chain else a.write_max_mbp, a.timeout,
                    a.locate_sites if a.locate else None, a.guides, (a.search_queries, a.search_valu, (a.search_bulges, a.bulge_valu) if a.search_bulges else None) if a.search else None,
                    (a.haplotype_indels, max(a.search_queries)) if a.haplotypes else None)
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
