"""Host model of the result table (issl_results_* of include/issl_hip.h): Crackling.py:263-268 and :842-852 done the
reference's way -- a dict of properties per guide, typed as the reference types them (codes and isUnique as int, AT and
the scores as float, the rest as str), through Python's csv.writer with dialect 'unix' and QUOTE_MINIMAL.  Nothing of the
library runs here.  host_stages() makes the structured arrays the table is written from with the host models of the
earlier stages (guides_util, consensus_util, bowtie_util, the C oracle), so the model can be pinned to the reference's own
files (tests/golden/results, tools/make_golden_results.py) without a GPU."""
import csv
import gzip
import io
import json
import pathlib

import numpy as np

import bowtie_util as bu
import consensus_util as cu
import guides_util as gu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "results"
ORDER = ["seq", "sgrnascorer2score", "header", "start", "end", "strand", "isUnique", "passedG20", "passedTTTT", "passedATPercent",
         "passedSecondaryStructure", "ssL1", "ssStructure", "ssEnergy", "acceptedByMm10db", "acceptedBySgRnaScorer",
         "consensusCount", "passedBowtie", "passedOffTargetScore", "AT", "bowtieChr", "bowtieStart", "bowtieEnd",
         "mitOfftargetscore", "cfdOfftargetscore", "passedAvoidLeadingT"]
DELIMITERS = [",", "\t", ";", "|", " "]
CODE = {0: 0, 1: 1, 2: "?", 3: "!"}
NONE = 0xFFFFFFFF
PRINTS_MIT, PRINTS_CFD = ("mit", "and", "or", "avg"), ("cfd", "and", "or", "avg")  # matched exactly by the scorer


def text(b):
    """bytes -> str, byte for byte (the writer looks at single characters below 128 only)."""
    return b.decode("latin-1") if isinstance(b, (bytes, np.bytes_)) else str(b)


def guide_strings(guides):
    g = guides["guide23"]
    if g.dtype.kind == "S":
        return [x.decode() for x in g]
    return ["".join("ACGT"[(int(x) >> (2 * p)) & 3] for p in range(23)) for x in g]


def through_text(x):
    """What Crackling holds after float() of the scorer's '%f' (Crackling.py:785-786)."""
    return float("%f" % x)


def verdict(mit, cfd, method, threshold):
    """Crackling.py:794-835 -> 0, 1 or '?' (no branch of the chain matches the method)."""
    m = str(method).strip().lower()
    if m == "mit":
        return 0 if mit < threshold else 1
    if m == "cfd":
        return 0 if cfd < threshold else 1
    if m == "and":
        return 0 if mit < threshold and cfd < threshold else 1
    if m == "or":
        return 0 if mit < threshold or cfd < threshold else 1
    if m == "avg":
        return 0 if (mit + cfd) / 2 < threshold else 1
    return "?"


def model_table(guides, record_names, rows, fold_rows=None, folds_text=None, selection=None, bowtie_rows=None, genome_names=None,
                scores=None, delimiter=",", method="and", threshold=75.0):
    """guides: structured array with guide23 (S23 or packed), record, start, strand, seen; record_names: bytes per record
    of the guide set; rows: consensus rows (consensus_util.ROW_DTYPE); fold_rows + folds_text: the fold list and one
    (L1, structure, energy) or None per row of it; selection + bowtie_rows + genome_names: the Bowtie step; scores:
    (rows, mit, cfd) as arrays.  -> (bytes of the file, uint64 offsets of the n rows and the end)."""
    seqs = guide_strings(guides)
    props = []
    for j, g in enumerate(guides):
        r = rows[j]
        p = dict.fromkeys(ORDER, "?")
        p["seq"] = seqs[j]
        if int(g["seen"]) == 1:
            p.update(header=text(record_names[int(g["record"])]), start=str(int(g["start"])), end=str(int(g["start"]) + 23),
                     strand="-" if int(g["strand"]) else "+", isUnique=1)
        else:
            p.update(header="-", start="-", end="-", strand="-", isUnique=0)
        for f, c in cu.COLUMNS.items():
            p[c] = CODE[int(r[f])]
        p["consensusCount"] = int(r["count"])
        if not np.isnan(r["at"]):
            p["AT"] = float(r["at"])
        if not np.isnan(r["sgrna_score"]):
            p["sgrnascorer2score"] = float(r["sgrna_score"])
        props.append(p)
    if folds_text is not None:
        assert len(folds_text) == len(fold_rows)
        for j, entry in zip(fold_rows, folds_text):
            if entry is not None:
                for c, v in zip(("ssL1", "ssStructure", "ssEnergy"), entry):
                    if v is not None:
                        props[int(j)][c] = text(v)
    if bowtie_rows is not None:
        assert len(bowtie_rows) == len(selection)
        names = [(n.split() or [b""])[0] for n in genome_names]
        for j, b in zip(selection, bowtie_rows):
            if int(b["code"]) == 2:
                continue
            p = props[int(j)]
            p["passedBowtie"] = int(b["code"])
            if int(b["record"]) == NONE:
                p.update(bowtieChr="*", bowtieStart=0, bowtieEnd=22)
            else:
                p.update(bowtieChr=text(names[int(b["record"])]), bowtieStart=int(b["pos"]) + 1, bowtieEnd=int(b["pos"]) + 23)
    if scores is not None:
        for j, mit, cfd in zip(*scores):
            p = props[int(j)]
            mit = through_text(float(mit)) if method in PRINTS_MIT else -1.0
            cfd = through_text(float(cfd)) if method in PRINTS_CFD else -1.0
            p["mitOfftargetscore"], p["cfdOfftargetscore"] = mit, cfd
            p["passedOffTargetScore"] = verdict(mit, cfd, method, float(threshold))
    out = io.StringIO(newline="")
    w = csv.writer(out, delimiter=delimiter, quotechar='"', dialect="unix", quoting=csv.QUOTE_MINIMAL)
    w.writerow(ORDER)
    offsets = np.zeros(len(props) + 1, dtype=np.uint64)
    for j, p in enumerate(props):
        offsets[j] = out.tell()
        for c in ("header", "ssL1", "ssStructure", "ssEnergy", "bowtieChr"):
            assert "\r" not in str(p[c]) and "\n" not in str(p[c]), "the csv module of older Pythons does not quote a lone CR"
        w.writerow([p[c] for c in ORDER])
    offsets[len(props)] = out.tell()
    return out.getvalue().encode("latin-1"), offsets


def read_rnafold_text(fold_text, guides):
    """The model of crackling_amd.read_rnafold_text: Crackling.py:439-474 line by line."""
    structures = {}
    lines = fold_text.splitlines()
    for i in range(0, len(lines) - 1, 2):
        l1, l2 = lines[i].rstrip(), lines[i + 1].rstrip()
        structures[l1[0:20][1:20].replace("U", "T")] = (l1, l2)
    out = []
    for g in guides:
        if g[1:20] not in structures:
            out.append(None)
            continue
        l1, l2 = structures[g[1:20]]
        out.append((l1, l2.split(" ")[0], l2.split(" ")[1][1:-1]))
    return out


# ---- the goldens ------------------------------------------------------------------------------------------------------

def golden_runs():
    return json.loads((GOLDEN / "runs.json").read_text())


def golden_bytes(name):
    return gzip.decompress((GOLDEN / f"{name}.txt.gz").read_bytes())


def golden_input(run):
    return ((GOLDEN if run["input"].startswith("headers") else bu.GOLDEN) / run["input"]).read_bytes()


def golden_fold_text(run):
    """What RNAfold's stand-in printed in (or for a superset of the guides of) this run."""
    name = "headers_fold.txt.gz" if run["name"] == "headers" else None
    return gzip.decompress((GOLDEN / name).read_bytes()).decode() if name else bu.golden_folds()


def golden_keywords(run):
    """The keywords of crackling_amd.pipeline.run's config for a run of runs.json."""
    kw = cu.golden_keywords(run)
    kw.update(offtargetscore=bool(run["enabled"]), page_length=run["page_length"], max_distance=run["max_distance"],
              score_threshold=float(run["score_threshold"]), method=run["method"], delimiter=run["delimiter"])
    return kw


def host_stages(run, fold_text):
    """The arrays of a golden run from the host models of the stages -> keyword arguments of model_table."""
    import oracle_util as ou
    records = gu.parse([golden_input(run)])
    guides = gu.brute_force(records)
    seqs = guide_strings(guides)
    kw = golden_keywords(run)
    m = cu.Model(seqs, guides["seen"], **{k: kw[k] for k in ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model",
                                                             "sgrna_threshold", "low_energy", "high_energy")})
    fold_guides = [seqs[j] for j in m.fold_rows]
    folds = None
    if len(fold_guides):
        import crackling_amd as ca
        folds = ca.read_rnafold_output(fold_text, fold_guides)
    m.finish(folds)
    out = dict(guides=guides, record_names=[n for n, _ in records], rows=m.rows, fold_rows=m.fold_rows,
               folds_text=read_rnafold_text(fold_text, fold_guides), delimiter=run["delimiter"], method=run["method"],
               threshold=float(run["score_threshold"]))
    if run["enabled"]:
        genome = bu.golden_model()
        sel = m.selected
        brows = genome.rows(np.array([bu.sig(seqs[j][:20]) for j in sel], dtype=np.uint64), run["page_length"])
        scored = sel if m.level < 2 else sel[brows["code"] != 0]
        oracle = ou.OracleIndex(bu.GOLDEN / "index.issl")
        mit, cfd = oracle.score(np.array([bu.sig(seqs[j][:20]) for j in scored], dtype=np.uint64), run["max_distance"],
                                float(run["score_threshold"]), run["method"])
        oracle.close()
        out.update(selection=sel, bowtie_rows=brows, genome_names=[n.encode() for n, _ in genome.records], scores=(scored, mit, cfd))
    return out


# ---- crafted input ----------------------------------------------------------------------------------------------------

ODD = ['plain', 'with,comma', 'semi;colon', 'pipe|here', 'tab\there', 'a "quoted" word', '"', '""', ',";|', "caf\xe9 \xff", "x  y",
       "'single'", "q\"a,b\"c;d|e\tf g"]
SCORES = [1 / 128, 3 / 128, 99.9999995, 4e-7, 5e-7, 0.0, 100.0, -1.0, 0.5e-6, 1.5e-6, 2.5e-6, 74.9999995, 75.0000005, 1e-4, 99.99995]


def crafted_fasta(n_guides, seed=3, long_header=0):
    """A FASTA of records of 30 .. 70 random bases whose guide set has exactly n_guides guides: unique header lines that need
    quoting under one delimiter or another, records without a guide, records that repeat an earlier one (guides seen twice)
    and, with long_header, one header line of that many bytes.  -> bytes"""
    rng = np.random.default_rng(seed)
    records, seqs, distinct = [], [], set()
    have, tries = 0, 0
    while have < n_guides or len(records) < 3:
        tries += 1
        assert tries < 20000
        kind = rng.integers(0, 10)
        if kind == 0 and seqs:
            seq = seqs[rng.integers(0, len(seqs))]                         # again: its guides are seen twice
        elif kind == 1:
            seq = "AT" * int(rng.integers(5, 20))                           # no guide
        else:
            seq = "".join(rng.choice(list("ACGT"), int(rng.integers(30, 70))))
        name = f"{ODD[rng.integers(0, len(ODD))]} {len(records)} {ODD[rng.integers(0, len(ODD))]}"
        if long_header and len(records) == 2:
            name = ("long, \"header\" " + "x;y|z\t " * (long_header // 7))[:long_header] + " end"
            seq = "".join(rng.choice(list("ACGT"), 30)) + "ACGTACGTTGCATGCAAGCTAGG"  # (a guide of its own)
        new = {g for _, _, g in gu.matches(seq.encode())}
        if len(distinct | new) > n_guides and not (long_header and len(records) == 2):
            continue
        records.append(f">{name}\n{seq}\n")
        seqs.append(seq)
        distinct |= new
        have = len(distinct)
    blob = "".join(records).encode("latin-1")
    assert len(gu.brute_force(gu.parse([blob]))) == n_guides == have, (have, n_guides)
    return blob


def crafted_fold_texts(n, seed, delimiter):
    """n entries for a fold list: None, or three texts (bytes) with quotes, every delimiter, blanks, bytes above 127, the
    empty text and None (a span that leaves '?')."""
    rng = np.random.default_rng(seed)
    pool = [b"", b"?", b"-5.30", b"(((...)))", b'"', b'""', b'a"b', b"x,y", b"x;y", b"x|y", b"x\ty", b"x y", b" lead", b"trail ",
            b"\xff\xfe\x80", b"GUUUUAGAGCUAGAAAUAGC" * 5, delimiter.encode() * 3, b'",";"|"', b"'"]
    out = []
    for _ in range(n):
        if rng.integers(0, 6) == 0:
            out.append(None)
        else:
            out.append(tuple(None if rng.integers(0, 12) == 0 else pool[rng.integers(0, len(pool))] for _ in range(3)))
    return out


def crafted_scores(rows, seed):
    """(rows, mit, cfd) for every second row of `rows`: SCORES first, then doubles in [0, 100]."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows)[::2]
    mit, cfd = rng.uniform(0, 100, len(rows)), rng.uniform(0, 100, len(rows))
    k = min(len(rows), len(SCORES))
    mit[:k] = SCORES[:k]
    cfd[:k] = SCORES[:k][::-1]
    return rows, mit, cfd
