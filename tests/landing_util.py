"""Truth for the off-target landings (include/issl_hip.h, issl_offtarget_landings*): three results that are pinned
elsewhere, joined in numpy -- the records of IsslIndex.offtargets (pinned to the oracle), the brute force of locate_util
over the parsed FASTA, and the transcript model of transcripts_util asked for (record name up to its first blank, pos + 1).
Also the per-guide profile, the two text forms of bin/isslLandOfftargets, and the FASTA generators the tests share."""
import functools
import re

import numpy as np

import locate_util as lu
import transcripts_util as tu

BINS = 7
LANDING = np.dtype([("site", "<u8"), ("pos", "<u8"), ("record", "<u4"), ("strand", "<u4"), ("guide", "<u4"), ("rank", "<u4"),
                    ("id", "<u4"), ("occ", "<u4"), ("dist", "<u2"), ("slice", "<u2"), ("pad", "<u4"), ("hits", tu.DTYPE)])
PROFILE = np.dtype([("located", "<u8", (BINS,)), ("in_exon", "<u8", (BINS,)), ("absent", "<u4", (BINS,)), ("pad", "<u4")])
assert LANDING.itemsize == 64 and PROFILE.itemsize == 144
_NAME = re.compile(rb"[ \t\n\v\f\r]*([^ \t\n\v\f\r]*)")
RUN_COUNTS = [1, 63, 64, 65, 4096, 4097, 70000]


# ---- genomes -----------------------------------------------------------------------------------------------------------

def repeat_genome(seed, mbp=1.0, records=5):
    """Seeded i.i.d. bases with interspersed copies of a few 300-bp elements, in `records` records named `chrN test` of
    wrapped lines (the generator of tests/test_locate.py, restated)."""
    rng = np.random.default_rng(seed)
    n = int(mbp * 1e6)
    seq = rng.integers(0, 4, size=n, dtype=np.uint8)
    elems = rng.integers(0, 4, size=(8, 300), dtype=np.uint8)
    for at in rng.integers(0, n - 300, size=n // 3000):
        e = elems[rng.integers(0, 8)].copy()
        mut = rng.random(300) < 0.02
        e[mut] = rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)
        seq[at:at + 300] = e
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[seq].tobytes()
    cuts = [0] + sorted(rng.integers(1, n, size=records - 1).tolist()) + [n]
    out = []
    for r in range(records):
        rec = text[cuts[r]:cuts[r + 1]]
        out.append(b">chr%d test\n" % r + b"\n".join(rec[i:i + 70] for i in range(0, len(rec), 70)) + b"\n")
    return b"".join(out)


def run_words(n=len(RUN_COUNTS)):
    """One 23-mer per run: a counter in base 4 behind a fixed head, a forward PAM behind it.  n <= 16 words differ in two
    places at most."""
    return [("ACGTTGCAACGTTGCA" + "".join("ACGT"[(k >> (2 * d)) & 3] for d in range(4)) + "AGG").encode() for k in range(n)]


def runs_genome(counts=RUN_COUNTS, names=(b"run0", b"run1", b"run2"), skip=()):
    """Word k back to back counts[k] times behind a stretch of T (no match of either pattern), the runs dealt out over
    len(names) records; the records whose index is in `skip` are left out of the FASTA text.  -> (fasta, words); the runs of
    a record start at run_starts(counts, names)[k]."""
    words = run_words(len(counts))
    recs = [b"" for _ in names]
    for k, (w, c) in enumerate(zip(words, counts)):
        recs[k % len(names)] += b"T" * (17 + k) + w * c
    fasta = b"".join(b">" + names[r] + b"\n" + s + b"\n" for r, s in enumerate(recs) if r not in skip)
    return fasta, words


def run_starts(counts=RUN_COUNTS, n_records=3):
    """pos of the first copy of every run inside its record."""
    at = [0] * n_records
    out = []
    for k, c in enumerate(counts):
        at[k % n_records] += 17 + k
        out.append(at[k % n_records])
        at[k % n_records] += 23 * c
    return out


# ---- the join ----------------------------------------------------------------------------------------------------------

def query_name(header):
    """The name a record is asked under: its header from the first non-blank character up to the next blank."""
    return _NAME.match(header).group(1)


def location_hits(records, truth, model):
    """The transcript answer of every row of `truth` (locate_util.brute_force): model.rows(names, pos + 1), asked once per
    distinct (record, pos)."""
    names = [query_name(n) for n, _ in records]
    key = (truth["record"].astype(np.uint64) << np.uint64(44)) | truth["pos"]
    uniq, inverse = np.unique(key, return_inverse=True)
    rec = (uniq >> np.uint64(44)).astype(np.int64)
    pos = (uniq & np.uint64((1 << 44) - 1)).astype(np.int64)
    return model.rows([names[r] for r in rec], pos + 1)[inverse]


def join(n_guides, offs, recs, truth, truth_hits=None):
    """offs, recs: IsslIndex.offtargets of the guides.  truth: brute_force of the genome; truth_hits: location_hits, or None
    without an annotation.  -> (offsets uint64[n + 1], rows LANDING, landings per record)."""
    order = np.argsort(truth["site"], kind="stable")  # inside a site: (record, pos, strand), the brute force's order
    sites = truth["site"][order]
    lo = np.searchsorted(sites, recs["site"], "left")
    cnt = np.searchsorted(sites, recs["site"], "right") - lo
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    total = int(first[-1])
    of_rec = np.repeat(np.arange(len(recs)), cnt)
    which = order[np.repeat(lo, cnt) + (np.arange(total) - first[of_rec])]
    rows = np.zeros(total, dtype=LANDING)
    offs = np.asarray(offs).astype(np.int64)
    guide = np.repeat(np.arange(n_guides), np.diff(offs))
    assert np.array_equal(guide, recs["guide"])
    for f in ("site", "id", "occ", "dist", "slice", "guide"):
        rows[f] = recs[f][of_rec]
    rows["rank"] = (np.arange(len(recs)) - offs[guide])[of_rec]
    for f in ("pos", "record", "strand"):
        rows[f] = truth[f][which]
    if truth_hits is None:
        rows["hits"]["status"] = 1
        rows["hits"]["first"] = tu.NONE
    else:
        rows["hits"] = truth_hits[which]
    return first[offs].astype(np.uint64), rows, cnt


def profile(n_guides, recs, cnt, rows):
    out = np.zeros(n_guides, dtype=PROFILE)
    np.add.at(out["located"], (recs["guide"], recs["dist"]), cnt.astype(np.uint64))
    gone = cnt == 0
    np.add.at(out["absent"], (recs["guide"][gone], recs["dist"][gone]), 1)
    cut = rows["hits"]["hit"] > 0
    np.add.at(out["in_exon"], (rows["guide"][cut], rows["dist"][cut]), 1)
    return out


# ---- bin/isslLandOfftargets ----------------------------------------------------------------------------------------------

def records_text(guides, rows, records, with_hits):
    g_text, s_text = lu.sig_text(guides), lu.sig_text(rows["site"])
    out = []
    for k, r in enumerate(rows):
        line = b"%s\t%s\t%d\t%d\t%s\t%d\t%s" % (g_text[int(r["guide"])], s_text[k], int(r["dist"]), int(r["occ"]), records[int(r["record"])][0],
                                                 int(r["pos"]), b"-" if r["strand"] else b"+")
        if with_hits:
            line += b"\t" + tu.hits_text(r["hits"]).encode()
        out.append(line + b"\n")
    return b"".join(out)


def profile_text(guides, prof, max_dist):
    out = []
    for g, p in zip(lu.sig_text(guides), prof):
        cols = [int(x) for f in ("located", "in_exon", "absent") for x in p[f][:max_dist + 1]]
        out.append(g + b"".join(b"\t%d" % c for c in cols) + b"\n")
    return b"".join(out)


# ---- the shared inputs of tests/test_landing_model.py and tests/test_landing_gpu.py --------------------------------------

@functools.lru_cache(maxsize=None)
def repeat_case():
    """The seed-21 repeat genome with random_annotation(default_rng(31), 5, 3000, span=250_000): (fasta, records, truth, gff,
    truth_hits, guides) -- 32 guides picked from the brute force by the answer at one of their own places: 8 with status 0
    and a hit, 8 with status 0 and none, 8 with status 2, 8 with status 3, each group spread evenly over its places."""
    fasta = repeat_genome(21)
    records = lu.parse([fasta])
    truth = lu.brute_force(records)
    gff = tu.random_annotation(np.random.default_rng(31), 5, 3000, span=250_000)
    hits = location_hits(records, truth, tu.Model(gff))
    groups = [(hits["status"] == 0) & (hits["hit"] > 0), (hits["status"] == 0) & (hits["hit"] == 0), hits["status"] == 2, hits["status"] == 3]
    picked = []
    for g in groups:
        at = np.flatnonzero(g)
        sites = []
        for i in at[np.linspace(0, len(at) - 1, 64).astype(np.int64)]:
            if int(truth["site"][i]) not in sites and int(truth["site"][i]) not in picked:
                sites.append(int(truth["site"][i]))
        picked += sites[:8]
    return fasta, records, truth, gff, hits, np.array(picked, dtype=np.uint64)
