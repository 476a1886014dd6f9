"""Truth for the Bowtie step's tests: the definition of an occurrence (include/issl_hip.h, issl_genome_occurrences)
restated in Python as a dict from 23-mer to its occurrences, and the rows that follow from it when the verdicts are
filed the way the reference reads Bowtie's output (Crackling.py:659-720).  tests/test_bowtie_host.py
pins it to the reference's own run (tests/golden/bowtie) before tests/test_bowtie_gpu.py compares the device with it."""
import csv
import gzip
import json
import pathlib

import numpy as np

import locate_util as lu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "bowtie"
PAMS = ("AGG", "CGG", "GGG", "TGG", "AAG", "CAG", "GAG", "TAG")
DTYPE = np.dtype([("pos", "<u8"), ("record", "<u4"), ("n_perfect", "<u4"), ("aligned", "u1"), ("repeated", "u1"), ("nb", "u1"),
                  ("strand", "u1"), ("owner", "u1"), ("code", "u1"), ("reserved", "u1", (2,)), ("source", "<u4"), ("reserved2", "<u4")])
FIELDS = ("pos", "record", "n_perfect", "aligned", "repeated", "nb", "strand", "owner", "code", "source")
NONE = 0xFFFFFFFF
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_COMP)


def sig(s):
    """Packed signature of a 20-mer: base p in bits 2p, 2p + 1."""
    return sum(_CODE[c] << (2 * p) for p, c in enumerate(s))


def unsig(x):
    return "".join("ACGT"[(int(x) >> (2 * p)) & 3] for p in range(20))


def occurrence_dict(records):
    """records: [(name, upper-cased sequence)] as str.  -> {23-mer read: [(record, pos, strand)] ascending}.  A window of
    23 characters A, C, G, T inside one record is an occurrence of itself on strand 0 and of its reverse complement on
    strand 1; only reads that end in [AG]G are kept, no other is ever asked for."""
    occ = {}
    for r, (_, seq) in enumerate(records):
        for pos in range(len(seq) - 22):
            w = seq[pos:pos + 23]
            if any(c not in "ACGT" for c in w):
                continue
            if w[21] in "AG" and w[22] == "G":
                occ.setdefault(w, []).append((r, pos, 0))
            if w[0] == "C" and w[1] in "CT":
                occ.setdefault(rc(w), []).append((r, pos, 1))
    return occ


class Model:
    def __init__(self, blobs):
        """blobs: the FASTA inputs as bytes, joined into records by the extraction's rules (locate_util.parse)."""
        self.records = [(n.decode(), s.decode()) for n, s in lu.parse(blobs)]
        self.occ = occurrence_dict(self.records)
        # per 20-mer of the text that has an occurrence: everything of a row but owner and code
        table = {}
        for read, where in self.occ.items():
            assert where == sorted(where)
            row = table.setdefault(sig(read[:20]), dict(n=0, aligned=0, repeated=0, first=None))
            v = PAMS.index(read[20:])
            row["n"] += len(where)
            row["aligned"] |= 1 << v
            if len(where) > 1:
                row["repeated"] |= 1 << v
            if v == 0:
                row["first"] = where[0]
        self.keys = np.array(sorted(table), dtype=np.uint64)
        self.stats = np.zeros(len(self.keys), dtype=DTYPE)
        for k, key in enumerate(self.keys):
            t = table[int(key)]
            rec, pos, strand = t["first"] if t["first"] else (NONE, 0, 0)
            self.stats[k] = (pos, rec, min(t["n"], NONE), t["aligned"], t["repeated"],
                             bin(t["aligned"]).count("1") + bin(t["repeated"]).count("1"), strand, 0, 2, 0, NONE, 0)

    def counts(self, sigs):
        """Everything of the rows that the text and the 20-mer alone decide; untested, with the 20-mer's own place."""
        sigs = np.asarray(sigs, dtype=np.uint64)
        rows = np.zeros(len(sigs), dtype=DTYPE)
        rows["record"] = rows["source"] = NONE
        rows["code"] = 2
        if len(sigs) and len(self.keys):
            at = np.minimum(np.searchsorted(self.keys, sigs), len(self.keys) - 1)
            hit = self.keys[at] == sigs
            rows[hit] = self.stats[at[hit]]
        return rows

    def rows(self, sigs, page_length=0):
        """sigs: uint64 array of packed 20-mers -> DTYPE array, one row per query.  The group of query i names the last
        query of its page with i's 20-mer -- or, when i's read 0 first occurs on strand 1 and what Bowtie then prints
        (the reverse complement: CCT and the complement of bases 19..3, then N[AG]G) starts with the 20-mer of a query of
        the page, the last query with that one.  The last group that names a query is its source."""
        sigs = np.asarray(sigs, dtype=np.uint64)
        n = len(sigs)
        rows = self.counts(sigs)
        if n == 0:
            return rows
        idx = np.arange(n, dtype=np.int64)
        page = idx // page_length if page_length else np.zeros(n, dtype=np.int64)
        if int(page[-1]) < 1 << 23:  # one stable sort of sig | page instead of three
            order = np.argsort((sigs << np.uint64(23)) | page.astype(np.uint64), kind="stable")
        else:
            order = np.lexsort((idx, page, sigs))
        s, p = sigs[order], page[order]
        last = np.ones(n, dtype=bool)
        last[:-1] = (s[1:] != s[:-1]) | (p[1:] != p[:-1])
        ends = np.nonzero(last)[0]                                   # sorted position of every group's last query
        target = np.empty(n, dtype=np.int64)
        target[order] = order[ends[np.searchsorted(ends, np.arange(n))]]
        # the few queries whose read 0 is printed reverse-complemented
        b0, b1 = sigs & np.uint64(3), (sigs >> np.uint64(2)) & np.uint64(3)
        cand = np.nonzero((rows["record"] != NONE) & (rows["strand"] == 1) & (b0 == 1) & ((b1 == 1) | (b1 == 3)))[0]
        if len(cand):
            others = {int(i): sig("CCT" + rc(unsig(sigs[i]))[:17]) for i in cand}
            wanted = np.isin(sigs, np.array(sorted(set(others.values())), dtype=np.uint64))
            filed = {}
            for j in np.nonzero(wanted)[0]:
                filed[(int(page[j]), int(sigs[j]))] = int(j)         # ascending j: the last one stays
            for i, other in others.items():
                target[i] = filed.get((int(page[i]), other), target[i])
        src = np.zeros(n, dtype=np.int64)
        np.maximum.at(src, target, idx + 1)
        named = src > 0
        from_row = rows[np.where(named, src - 1, idx)]
        for f in ("pos", "record", "strand"):
            rows[f] = from_row[f]
        rows["owner"] = named
        rows["code"] = np.where(~named, 2, np.where(from_row["nb"] > 1, 0, 1))
        rows["source"] = np.where(named, src - 1, NONE)
        return rows

    def rows_slow(self, guides20, page_length=0):
        """The same as the reference does it, line by line: the reads of a page filed in a dict, one printed sequence per
        group looked up there and then reverse-complemented.  For small inputs."""
        n = len(guides20)
        rows = np.zeros(n, dtype=DTYPE)
        own = []
        for i, g in enumerate(guides20):
            occ = [self.occ.get(g + pam, []) for pam in PAMS]
            aligned = sum(1 << v for v in range(8) if len(occ[v]) >= 1)
            repeated = sum(1 << v for v in range(8) if len(occ[v]) >= 2)
            nb = bin(aligned).count("1") + bin(repeated).count("1")
            rec, pos, strand = occ[0][0] if occ[0] else (NONE, 0, 0)
            own.append((rec, pos, strand, nb))
            rows[i] = (pos, rec, min(sum(len(o) for o in occ), NONE), aligned, repeated, nb, strand, 0, 2, 0, NONE, 0)
        step = page_length or max(n, 1)
        for a in range(0, n, step):
            b = min(n, a + step)
            filed = {}
            for k in range(a, b):
                for pam in PAMS:
                    filed[guides20[k] + pam] = k
            for k in range(a, b):
                rec, pos, strand, nb = own[k]
                printed = rc(guides20[k] + PAMS[0]) if rec != NONE and strand == 1 else guides20[k] + PAMS[0]
                t = filed[printed] if printed in filed else filed[rc(printed)]
                rows["pos"][t], rows["record"][t], rows["strand"][t] = pos, rec, strand
                rows["owner"][t], rows["code"][t], rows["source"][t] = 1, 0 if nb > 1 else 1, k
        return rows


def same_rows(got, want, fields=FIELDS):
    assert len(got) == len(want)
    for f in fields:
        bad = np.nonzero(np.asarray(got[f]) != np.asarray(want[f]))[0]
        assert len(bad) == 0, (f, bad[:5].tolist(), np.asarray(got[f])[bad[:5]].tolist(), np.asarray(want[f])[bad[:5]].tolist())


# ---- adversarial text ------------------------------------------------------------------------------------------------

def adversarial_fasta(seed=7):
    """About 2.5 kbp in six records, with what an occurrence count can get wrong (each asserted by adversarial_checks):
    a read at a record's first and at its last possible position, and one that would start one position further (its
    last character is the next record's first); overlapping occurrences (G * 30); a window that is a forward and a reverse
    occurrence at once (CCT ... AGG, which also makes the reference file one guide's verdict under the other); a read once
    per strand; a copy with an N in it; a record of 22 bases; lower case.  -> (FASTA bytes, planted reads by name)"""
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    read = lambda pam: "ACG"[rng.integers(3)] + rand(19) + pam           # noqa: E731
    p = dict(first=read("AGG"), last=read("TGG"), past=read("CGG"), both="CCT" + rand(17) + "AGG", strands=read("CGG"),
             with_n=read("GGG"), short=read("AGG"))
    r0 = p["first"] + rand(300) + "A" + "G" * 30 + "T" + rand(200) + p["both"] + rand(150) + p["strands"] + rand(100) + p["last"]
    r1 = rand(250).lower() + p["with_n"] + rand(120) + p["past"][:22]
    r2 = p["past"][22] + rand(200) + rc(p["strands"]) + rand(90) + p["with_n"][:11] + "N" + p["with_n"][12:] + rand(200) + "T" + "C" * 30 + "A"
    r3 = p["short"][:22]
    r4 = p["short"][22] + rand(350) + "NNNNNN" + rand(150) + p["past"][:5]
    text = f">r0 one\n{r0}\n>r1\n{r1}\n>r2 two\n{r2}\n>r3 of 22\n{r3}\n>r4\n{r4}\n>empty\n"
    return text.encode(), p


def adversarial_checks(model, p):
    occ, rec = model.occ, model.records
    assert occ[p["first"]] == [(0, 0, 0)] and occ[p["last"]] == [(0, len(rec[0][1]) - 23, 0)]
    assert p["past"] not in occ and (rec[1][1] + rec[2][1]).count(p["past"]) == 1
    assert [s for _, _, s in occ["G" * 23]] == [0] * 8 + [1] * 8 and "G" * 20 + "AGG" not in occ  # G * 30 in r0, C * 30 in r2
    both = occ[p["both"]][0]
    assert (both[0], both[1], 1) in occ[rc(p["both"])[:20] + "AGG"]
    assert sorted(s for _, _, s in occ[p["strands"]]) == [0, 1]
    assert len(occ[p["with_n"]]) == 1 and len(rec[3][1]) == 22 and p["short"] not in occ and rec[5][1] == ""


def adversarial_queries(model, seed=11):
    """All 20-mers of the text, their reverse complements, each of those with one base changed, and a fifth of them a
    second time; shuffled.  -> uint64 signatures"""
    rng = np.random.default_rng(seed)
    mers = []
    for _, seq in model.records:
        mers += [seq[i:i + 20] for i in range(len(seq) - 19) if all(c in "ACGT" for c in seq[i:i + 20])]
    mers += [rc(m) for m in mers]
    sigs = np.array([sig(m) for m in mers], dtype=np.uint64)
    at = rng.integers(0, 20, len(sigs)).astype(np.uint64)
    changed = sigs ^ (rng.integers(1, 4, len(sigs)).astype(np.uint64) << (np.uint64(2) * at))
    sigs = np.concatenate([sigs, changed])
    sigs = np.concatenate([sigs, sigs[rng.random(len(sigs)) < 0.2]])
    rng.shuffle(sigs)
    return sigs


_adversarial = []


def adversarial():
    """-> (FASTA bytes, Model, planted reads, queries), built once."""
    if not _adversarial:
        blob, planted = adversarial_fasta()
        model = Model([blob])
        adversarial_checks(model, planted)
        _adversarial.extend([blob, model, planted, adversarial_queries(model)])
    return tuple(_adversarial)


# ---- the goldens ------------------------------------------------------------------------------------------------------

def golden_configs():
    return json.loads((GOLDEN / "configs.json").read_text())


def golden_rows(name):
    with open(GOLDEN / f"{name}.csv", newline="") as fh:
        return list(csv.DictReader(fh))


def golden_sam(name):
    """The SAM lines the stand-in for Bowtie2 printed for the configuration, all pages."""
    return gzip.decompress((GOLDEN / f"{name}.sam.gz").read_bytes()).decode()


def golden_folds():
    """What RNAfold's stand-in printed for the configuration that folds every guide."""
    return gzip.decompress((GOLDEN / "fold.txt.gz").read_bytes()).decode()


def golden_selection(cfg, rows):
    """The rows of the CSV the reference's filter hands the Bowtie step (Crackling.py:36-149 with passedBowtie untested)."""
    if cfg["optimisation"] == "ultralow":
        return list(range(len(rows)))
    return [k for k, r in enumerate(rows) if r["isUnique"] == "1" and int(r["consensusCount"]) >= cfg["n"]]


def golden_columns(rows, selection):
    return {c: [rows[k][c] for k in selection] for c in ("passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd")}


_model = []


def golden_model():
    """The model over tests/golden/bowtie/genome.fa, built once."""
    if not _model:
        _model.append(Model([(GOLDEN / "genome.fa").read_bytes()]))
    return _model[0]
