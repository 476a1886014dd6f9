#!/usr/bin/env python3
"""Wall time of IsslIndex.landings against the composition it replaces -- IsslIndex.offtargets + Genome.locate +
Annotation.hits with one Python name per location ("Transcript hit counts") -- on a generated repeat
genome.  Both give the same rows; the script checks that before it reports.

    python tools/bench_landings.py --mbp 50 --guides 10000 --max-dist 4 --output profiles/landings.json
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import crackling_amd as ca  # noqa: E402
import landing_util as mu  # noqa: E402
import transcripts_util as tu  # noqa: E402


def pick_guides(fasta, n, rng):
    """n sites of the forward pattern [ACG]N{19}N[AG]G at random places of the records' text."""
    seq = np.frombuffer(b"".join(line for line in fasta.split(b"\n") if not line.startswith(b">")), dtype=np.uint8)
    out = []
    while len(out) < n:
        at = rng.integers(0, len(seq) - 23, size=16 * n)
        ok = (seq[at] != ord("T")) & (seq[at + 22] == ord("G")) & ((seq[at + 21] == ord("A")) | (seq[at + 21] == ord("G")))
        out += [bytes(seq[i:i + 20]) for i in at[ok][:n - len(out)]]
    return ca.encode_guides(out)


def best(fn, repeats):
    times, result = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = fn()
        times.append(time.perf_counter() - t0)
    return min(times), times, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--guides", type=int, default=10_000)
    ap.add_argument("--max-dist", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--output", default=None)
    args = ap.parse_args()
    import torch

    rng = np.random.default_rng(args.seed)
    fasta = mu.repeat_genome(args.seed, mbp=args.mbp)
    gff = tu.random_annotation(np.random.default_rng(args.seed + 1), 5, int(400 * args.mbp), span=int(args.mbp * 1e6 / 5))
    guides = pick_guides(fasta, args.guides, rng)
    ix = ca.IsslIndex.build_from_fasta([fasta])
    genome = ca.Genome.open([fasta])
    ann = ca.Annotation.open(gff)
    name_of = [mu.query_name(n) for n, _ in genome.records]

    def composed():
        offs, recs = ix.offtargets(guides, max_dist=args.max_dist)
        loc_off, locs = genome.locate(recs["site"])
        hits = ann.hits([name_of[r] for r in locs["record"]], locs["pos"].astype(np.int64) + 1)
        return offs, recs, loc_off, locs, hits

    def fused():
        return ix.landings(guides, genome, ann, max_dist=args.max_dist)

    def profile():
        return ix.landing_profile(guides, genome, ann, max_dist=args.max_dist)

    composed()
    fused()  # (first calls: buffers grow)
    t_comp, all_comp, (offs, recs, loc_off, locs, hits) = best(composed, args.repeats)
    t_fused, all_fused, (offsets, rows) = best(fused, args.repeats)
    t_prof, all_prof, prof = best(profile, args.repeats)
    cnt = np.diff(loc_off.astype(np.int64))
    assert np.array_equal(offsets, loc_off[offs.astype(np.int64)]) and len(rows) == len(locs)
    assert all(np.array_equal(rows[f], locs[f]) for f in ("record", "pos", "strand"))
    assert np.array_equal(rows["site"], np.repeat(recs["site"], cnt)) and rows["hits"].tobytes() == hits.tobytes()
    assert int(prof["located"].sum()) == len(rows) and int(prof["in_exon"].sum()) == int((hits["hit"] > 0).sum())
    result = {
        "device": torch.cuda.get_device_name(0),
        "genome_mbp": args.mbp, "kind": "repeat", "seed": args.seed, "records": len(genome.records), "guides": args.guides,
        "max_dist": args.max_dist, "annotation": ann.info,
        "offtarget_records": int(len(recs)), "landings": int(len(rows)), "landings_in_exon": int((hits["hit"] > 0).sum()),
        "most_landings_of_one_guide": int(np.diff(offsets.astype(np.int64)).max()),
        "repeats": args.repeats,
        "composition_wall_s": t_comp, "composition_all_s": all_comp,
        "landings_wall_s": t_fused, "landings_all_s": all_fused,
        "landing_profile_wall_s": t_prof, "landing_profile_all_s": all_prof,
        "speedup_landings_over_composition": t_comp / t_fused,
        "note": "wall time of the Python calls, best of `repeats`; landings() is a counting call and a listing call, "
                "the composition is offtargets() + Genome.locate() (a counting and a listing call each) + Annotation.hits() "
                "with one Python bytes name per location",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if args.output:
        pathlib.Path(args.output).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.output).write_text(text + "\n")
    ann.close()
    genome.close()
    ix.close()


if __name__ == "__main__":
    main()
