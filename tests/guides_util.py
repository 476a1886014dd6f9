"""Expected guide sets for the guide-extraction tests: the record rules and the two patterns of Crackling.py:151-252
restated as plain character tests, with a dictionary for the first-seen order.  Written for the tests; shares no code
with the library."""
import csv
import json
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "guides"
BLANK = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"  # what str.strip() removes from ASCII text
ACGT = frozenset(b"ACGT")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ROW_DTYPE = np.dtype([("guide23", "S23"), ("record", "<u4"), ("start", "<u8"), ("strand", "<u4"), ("seen", "<u4")])


class BlankLine(ValueError):
    """The input the reference dies on (IndexError, Crackling.py:196): .args = (input index, 1-based line)."""


def _lines(data):
    """Python's text mode: "\\n", "\\r\\n" and a lone "\\r" each end a line."""
    out, p = [], 0
    while p < len(data):
        e = p
        while e < len(data) and data[e] not in (10, 13):
            e += 1
        nxt = min(e + 1, len(data))
        if data[e:e + 2] == b"\r\n":
            nxt = e + 2
        out.append(data[p:e])
        p = nxt
    return out


def parse(blobs):
    """The records that count, over all inputs in the order given -> [(name, sequence)].  A finished record counts when
    the next header arrives and its name is new (or it has no name but a sequence); the last record of an input always
    counts and its name is not remembered.  Text ahead of the first header is a record without a name; no text there is
    no record."""
    out, recorded = [], set()
    for f, data in enumerate(blobs):
        name, seq, headed = b"", [], False
        for n, raw in enumerate(_lines(bytes(data))):
            line = raw.strip(BLANK)
            if not line:
                raise BlankLine(f, n + 1)
            if line[:1] == b">":
                s = b"".join(seq)
                if name not in recorded or (name == b"" and s):
                    recorded.add(name)
                    if headed or s:
                        out.append((name, s))
                name, seq, headed = line[1:], [], True
            else:
                seq.append(line)
        s = b"".join(seq)
        if headed or s:
            out.append((name, s))
    return out


def matches(seq):
    """[(start, strand, guide)] of one record: all forward matches by position, then all reverse matches."""
    n = len(seq) - 22
    if n <= 0:
        return []
    c = np.frombuffer(seq, dtype=np.uint8)
    bad = np.concatenate([[0], np.cumsum(~np.isin(c, np.frombuffer(b"ACGT", dtype=np.uint8)))])  # bad[k]: not-ACGT in seq[:k]
    i = np.arange(n)
    g, cc = c == ord("G"), c == ord("C")
    fwd = (bad[i + 21] == bad[i]) & g[21:21 + n] & g[22:22 + n]
    rev = cc[:n] & cc[1:n + 1] & (bad[i + 23] == bad[i + 2])
    return [(int(k), 0, seq[k:k + 23]) for k in np.flatnonzero(fwd)] + \
           [(int(k), 1, seq[k:k + 23].translate(_COMP)[::-1]) for k in np.flatnonzero(rev)]


def brute_force(records):
    """Distinct guides in first-seen order with the place of their first occurrence and how often they were seen."""
    first, seen = {}, {}
    for r, (_, seq) in enumerate(records):
        for start, strand, guide in matches(seq):
            if guide in first:
                seen[guide] += 1
            else:
                first[guide] = (r, start, strand)
                seen[guide] = 1
    rows = np.zeros(len(first), dtype=ROW_DTYPE)
    for k, (guide, (r, start, strand)) in enumerate(first.items()):
        rows[k] = (guide, r, start, strand, seen[guide])
    return rows


def reference_rows(records, rows):
    """What the reference writes per guide: [seq, header, start, end, strand, isUnique] as text."""
    out = []
    for g in rows:
        if g["seen"] == 1:
            out.append([g["guide23"].decode(), records[int(g["record"])][0].decode(), str(int(g["start"])), str(int(g["start"]) + 23),
                        "-" if g["strand"] else "+", "1"])
        else:
            out.append([g["guide23"].decode(), "-", "-", "-", "-", "0"])
    return out


def golden_cases():
    """[(case, [paths in the order the reference reads them], input is the directory, what the reference did, rows)]"""
    out = []
    for c in json.loads((GOLDEN / "cases.json").read_text()):
        with open(GOLDEN / f"{c['case']}.guides.csv", newline="") as fh:
            rows = list(csv.reader(fh))[1:]
        assert len(rows) == c["rows"]
        out.append((c["case"], [GOLDEN / c["case"] / i for i in c["inputs"]], c["directory"], c["reference"], rows))
    return out


def check_set(gs, records, want):
    """A crackling_amd.GuideSet against parse() / brute_force() of the same input, field by field."""
    assert [(n, ln) for n, ln in gs.records] == [(n, len(s)) for n, s in records]
    got = gs.guides
    assert len(got) == len(want)
    assert gs.strings() == [g.decode() for g in want["guide23"]]
    for f in ("record", "start", "strand", "seen"):
        assert np.array_equal(got[f], want[f]), f
    assert not got["reserved"].any()
    assert gs.n_matches == int(want["seen"].sum(dtype=np.uint64))
    assert gs.n_unique == int((want["seen"] == 1).sum())
