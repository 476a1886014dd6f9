"""Truth for the transcript hit counts (include/issl_hip.h, issl_annotation_*): the rules of countHitTranscripts.py restated
as a model over dicts, written from the rules of the header, not from the reference's text.  tests/test_transcripts_model.py
pins it to the reference's own answers (tests/golden/transcripts, made by tools/make_golden_transcripts.py) before
tests/test_transcripts_gpu.py compares the device with it.  Also: random annotations and queries, and annotations built to
hit the sizes at which the kernels change shape."""
import csv
import io
import json
import pathlib
import re

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "transcripts"
DTYPE = np.dtype([("hit", "<u4"), ("total", "<u4"), ("status", "<u4"), ("first", "<u4")])
NONE = 0xFFFFFFFF
MAX_COORD = (1 << 40) - 2
_BLANKS = b" \t\n\v\f\r\x1c\x1d\x1e\x1f"  # what str.strip() removes among ASCII characters
_INT = re.compile(rb"[+-]?[0-9]+")


class FormatError(Exception):
    """Where the reference stops with a traceback."""


def to_int(text):
    raw = text if isinstance(text, bytes) else text.encode()
    if not _INT.fullmatch(raw) or not -(1 << 63) <= int(raw) < (1 << 63):
        raise FormatError(f"not an integer: {text!r}")
    return int(raw)


def cases():
    """The golden cases: dicts with name, annotation (path), crackling (path) and expected (path) or error (True)."""
    out = []
    for c in json.loads((GOLDEN / "cases.json").read_text()):
        d = dict(c)
        for key in ("annotation", "crackling", "expected"):
            if d.get(key):
                d[key] = (GOLDEN / d[key]).resolve()
        out.append(d)
    return out


class Model:
    """loadAnnotation and countTranscripts.  transcripts: {(sequence, id): ordinal} in order of first appearance."""

    def __init__(self, gff):
        self.seqs = []
        self.transcripts = {}
        self.exons = {}          # (sequence, id) -> [(start, end)]
        self.gene_of = {}        # transcript id -> Parent of the first mRNA line with that ID, anywhere in the file
        self.gene_lines = {}     # gene -> number of mRNA lines that name it
        self.n_exons = 0
        for line in gff.replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n"):
            fields = [f.strip(_BLANKS) for f in line.split(b"\t")]
            if len(fields) != 9:
                continue
            attributes = {}
            for a in fields[8].split(b";"):
                parts = a.split(b"=")
                if len(parts) < 2:
                    raise FormatError(f"attribute without '=': {a!r}")
                attributes[parts[0]] = parts[1]
            if b"ID" not in attributes or b"Parent" not in attributes or fields[2] not in (b"gene", b"mRNA", b"exon"):
                continue
            seq = fields[0].replace(b".", b"_")
            if seq not in self.seqs:
                self.seqs.append(seq)
            if fields[2] == b"mRNA":
                self.transcripts.setdefault((seq, attributes[b"ID"]), len(self.transcripts))
                self.exons.setdefault((seq, attributes[b"ID"]), [])
                self.gene_lines[attributes[b"Parent"]] = self.gene_lines.get(attributes[b"Parent"], 0) + 1
                self.gene_of.setdefault(attributes[b"ID"], attributes[b"Parent"])
            elif fields[2] == b"exon":
                key = (seq, attributes[b"Parent"])
                self.transcripts.setdefault(key, len(self.transcripts))
                self.exons.setdefault(key, []).append((to_int(fields[3]), to_int(fields[4])))
                self.n_exons += 1
        # per sequence: the exons as arrays, for queries by the thousand
        self._arrays = {}
        for seq in self.seqs:
            rows = [(s, e, self.transcripts[k]) for k in self.transcripts if k[0] == seq for s, e in self.exons[k]]
            self._arrays[seq] = np.array(rows, dtype=np.int64).reshape(-1, 3)
        self._ids = [k[1] for k in self.transcripts]

    @property
    def info(self):
        return {"n_seqs": len(self.seqs), "n_transcripts": len(self.transcripts), "n_genes": len(self.gene_lines),
                "n_exons": self.n_exons, "n_segments": sum(max(0, len(self.breakpoints(s, merged=True)) - 1) for s in self.seqs)}

    def breakpoints(self, seq, merged=False):
        """Where the answer can change on a sequence: the starts (raised to 0) and the ends + 1 of the exons that can hold
        a position >= 0, ascending.  merged: of every transcript's exons joined where they overlap -- the stretches the
        library counts as segments; a subset of the former."""
        pts = set()
        for k, exons in self.exons.items():
            if k[0] == seq:
                spans = sorted((max(s, 0), e) for s, e in exons if s <= e and e >= 0)
                if merged:
                    joined = []
                    for s, e in spans:
                        if joined and s <= joined[-1][1]:
                            joined[-1][1] = max(joined[-1][1], e)
                        else:
                            joined.append([s, e])
                    spans = joined
                for s, e in spans:
                    pts.update((s, e + 1))
        return sorted(pts)

    def query(self, name, start):
        """(hit, total, status, first) for bowtieChr `name` (taken as it stands) and bowtieStart `start`."""
        name = name if isinstance(name, bytes) else name.encode()
        if name not in self._arrays or start < 0:    # a negative start is answered 0/0 directly
            return (0, 0, 0, NONE)
        a = self._arrays[name]
        hit = np.unique(a[(a[:, 0] <= start) & (start <= a[:, 1]), 2]).tolist()  # ascending ordinals: the sequence's order
        if not hit:
            return (0, 0, 0, NONE)
        genes = {self.gene_of[self._ids[t]] for t in hit if self._ids[t] in self.gene_of}
        if len(genes) > 1:
            return (len(hit), 0, 2, hit[0])
        if self._ids[hit[0]] not in self.gene_of:
            return (len(hit), 0, 3, hit[0])
        return (len(hit), self.gene_lines[self.gene_of[self._ids[hit[0]]]], 0, hit[0])

    def rows(self, names, starts):
        return np.array([self.query(n, int(s)) for n, s in zip(names, starts)], dtype=DTYPE).reshape(-1)


def hits_text(row):
    return f"{row[0]}/{row[1]}" if row[2] == 0 else "?/?"


def process(gff, crackling):
    """The output file of the reference for a GFF3 annotation and Crackling's output file, both as bytes -> bytes.
    FormatError where the reference stops."""
    model = Model(gff)
    text = crackling.decode().replace("\r\n", "\n").replace("\r", "\n")  # universal newlines
    out = io.StringIO(newline="")
    writer = csv.writer(out, delimiter=",", quotechar='"', dialect="unix", quoting=csv.QUOTE_MINIMAL)
    col = None
    for n, row in enumerate(csv.reader(io.StringIO(text, newline=""), delimiter=",", quotechar='"')):
        if n == 0:
            if any(c not in row for c in ("seq", "bowtieChr", "bowtieStart", "bowtieEnd")):
                raise FormatError("the header lacks a column")
            col = [row.index(c) for c in ("seq", "bowtieChr", "bowtieStart", "bowtieEnd")]
            row = row + ["hits"]
        else:
            if len(row) <= col[1]:
                raise FormatError("a row without bowtieChr")
            if row[col[1]] == "?":
                row = row + ["?/?"]
            else:
                if len(row) <= max(col):
                    raise FormatError("a row that is too short")
                start, _ = to_int(row[col[2]]), to_int(row[col[3]])
                row = row + [hits_text(model.query(row[col[1]], start))]
        writer.writerow(row)
    return out.getvalue().encode()


# ---- generated annotations ---------------------------------------------------------------------------------------------

def gff_line(seq, kind, start, end, attributes):
    return f"{seq}\tmodel\t{kind}\t{start}\t{end}\t.\t+\t.\t{attributes}\n".encode()


def random_annotation(rng, n_seqs, n_exons, span=200_000):
    """GFF3 bytes: genes of 1..6 transcripts with 1..12 exons each, laid over `n_seqs` sequences so that genes overlap now
    and then; some transcripts without an mRNA line, some exons repeated or overlapping within their transcript, some
    with start > end, a dotted sequence name, a duplicated mRNA line here and there."""
    lines = []
    made = 0
    gene = 0
    while made < n_exons:
        seq = f"chr{int(rng.integers(n_seqs))}" + (".1" if rng.random() < 0.1 else "")
        at = int(rng.integers(0, span))
        gene += 1
        lines.append(gff_line(seq, "gene", at, at + 5000, f"ID=g{gene}"))
        for t in range(int(rng.integers(1, 7))):
            tid = f"g{gene}.t{t}"
            if rng.random() < 0.9:
                lines.append(gff_line(seq, "mRNA", at, at + 5000, f"ID={tid};Parent=g{gene}"))
                if rng.random() < 0.05:
                    lines.append(gff_line(seq, "mRNA", at, at + 5000, f"ID={tid};Parent=g{gene}"))
            p = at + int(rng.integers(0, 300))
            for x in range(int(rng.integers(1, 13))):
                length = int(rng.integers(0, 400))
                s, e = p, p + length
                if rng.random() < 0.03:
                    s, e = e + 1, s                  # contains nothing
                lines.append(gff_line(seq, "exon", s, e, f"ID={tid}.e{x};Parent={tid}"))
                made += 1
                if rng.random() < 0.1:               # the same stretch again, shifted a little: overlap inside the transcript
                    lines.append(gff_line(seq, "exon", s + 3, e + 3, f"ID={tid}.e{x}b;Parent={tid}"))
                    made += 1
                p = e + int(rng.integers(-50, 300))
                p = max(p, 0)
    return b"".join(lines)


def random_queries(rng, model, n):
    """(names, starts): most near a breakpoint of a known sequence, the rest anywhere: negative starts, starts past the
    last breakpoint and sequences the annotation lacks among them."""
    names, starts = [], []
    points = {s: model.breakpoints(s) for s in model.seqs}
    known = [s for s in model.seqs if points[s]]
    for _ in range(n):
        r = rng.random()
        if r < 0.05 or not known:
            names.append(b"absent" if rng.random() < 0.5 else b"*")
            starts.append(int(rng.integers(0, 1000)))
            continue
        seq = known[int(rng.integers(len(known)))]
        pts = points[seq]
        if r < 0.1:
            starts.append(-int(rng.integers(1, 1000)))
        elif r < 0.15:
            starts.append(pts[-1] + int(rng.integers(0, 1 << 41)))
        else:
            starts.append(pts[int(rng.integers(len(pts)))] + int(rng.integers(-2, 3)))
        # a dotted name never matches: the annotation's names carry '_'
        names.append(seq.replace(b"_", b".") if b"_" in seq and rng.random() < 0.1 else seq)
    return names, starts


def long_exon_annotation(k):
    """One exon of transcript `long` that covers exactly k segments: k - 1 one-base exons of other transcripts of the same
    gene start inside it at every other position (each adds a start and an end + 1: two breakpoints) -- so k is odd or,
    with one of them ending at the long exon's end, even."""
    lines = [gff_line("chrL", "mRNA", 1, 10, "ID=long;Parent=g")]
    # inner one-base exons at 102, 104, ...: breakpoints 102, 103, 104, ... -> two more segments each
    inner = (k - 1) // 2
    end = 100 + 2 * inner + 2
    lines.append(gff_line("chrL", "exon", 100, end, "ID=e;Parent=long"))
    for i in range(inner):
        lines.append(gff_line("chrL", "mRNA", 1, 10, f"ID=t{i};Parent=g"))
        lines.append(gff_line("chrL", "exon", 102 + 2 * i, 102 + 2 * i, f"ID=e{i};Parent=t{i}"))
    if (k - 1) % 2:                                   # one more breakpoint: an exon that starts inside and ends with the long one
        lines.append(gff_line("chrL", "mRNA", 1, 10, "ID=tail;Parent=g"))
        lines.append(gff_line("chrL", "exon", end, end, "ID=etail;Parent=tail"))
    return b"".join(lines)


def deep_segment_annotation(k, twice=False):
    """A position that k transcripts of one gene cover (each with a second, overlapping exon when `twice`), beside a
    shallow stretch; the transcripts' exons start at different places, so the lists around it differ in length."""
    lines = []
    for i in range(k):
        lines.append(gff_line("chrD", "mRNA", 1, 10, f"ID=t{i};Parent=g"))
        lines.append(gff_line("chrD", "exon", 1000 - (i % 7), 2000 + (i % 5), f"ID=e{i};Parent=t{i}"))
        if twice:
            lines.append(gff_line("chrD", "exon", 1500 - (i % 3), 2100, f"ID=f{i};Parent=t{i}"))
    return b"".join(lines)
