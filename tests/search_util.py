"""Expected rows for the genome search tests: a numpy brute force written from the definitions of include/issl_hip.h
(pattern, query, window, strand, hit, row fields), not from the kernel.  Every window of every record is taken as a row of
characters per strand; the pattern is a set of allowed bases per position, the distance a count of differing characters."""
import numpy as np

from crackling_amd import SEARCH_HIT_DTYPE
import locate_util as lu

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
_CODE = np.full(256, 4, dtype=np.int8)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k


def _text(x):
    return x.decode() if isinstance(x, (bytes, bytearray)) else x


def candidates(records, pattern):
    """Every (record, pos, strand) whose characters the pattern admits, in that order, with the characters t as codes
    0..3: -> (record, pos, strand, t[S, L])."""
    pattern = _text(pattern).upper()
    L = len(pattern)
    allowed = np.zeros((L, 4), dtype=bool)
    for i, ch in enumerate(pattern):
        for b in IUPAC[ch]:
            allowed[i, "ACGT".index(b)] = True
    recs, poss, strands, ts = [], [], [], []
    for r, (_, seq) in enumerate(records):
        if len(seq) < L:
            continue
        c = _CODE[np.frombuffer(seq, dtype=np.uint8)]
        w = np.lib.stride_tricks.sliding_window_view(c, L)
        clean = np.flatnonzero((w < 4).all(axis=1))
        w = w[clean]
        for strand, t in ((0, w), (1, 3 - w[:, ::-1])):
            ok = np.ones(len(t), dtype=bool)
            for i in range(L):
                ok &= allowed[i][t[:, i]]
            recs.append(np.full(int(ok.sum()), r, dtype=np.int64))
            poss.append(clean[ok])
            strands.append(np.full(int(ok.sum()), strand, dtype=np.int64))
            ts.append(np.ascontiguousarray(t[ok]))
    if not recs:
        return (np.zeros(0, np.int64),) * 3 + (np.zeros((0, L), np.int8),)
    rec, pos, strand, t = np.concatenate(recs), np.concatenate(poss), np.concatenate(strands), np.concatenate(ts)
    order = np.lexsort((strand, pos, rec))
    return rec[order], pos[order], strand[order], t[order]


def brute_force(records, pattern, queries, max_dist):
    """-> (offsets uint64[n + 1], rows in SEARCH_HIT_DTYPE, profile uint64[n, max_dist + 1])."""
    L = len(pattern)
    rec, pos, strand, t = candidates(records, pattern)
    site = np.zeros(len(t), dtype=np.uint64)
    for i in range(L):
        site |= t[:, i].astype(np.uint64) << np.uint64(2 * i)
    offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    profile = np.zeros((len(queries), max_dist + 1), dtype=np.uint64)
    parts = []
    for k, q in enumerate(queries):
        q = _text(q).upper()
        assert len(q) == L and set(q) <= set("ACGTN")
        differs = np.zeros((len(t), L), dtype=bool)
        for i, ch in enumerate(q):
            if ch != "N":
                differs[:, i] = t[:, i] != "ACGT".index(ch)
        dist = differs.sum(axis=1)
        hit = np.flatnonzero(dist <= max_dist)
        part = np.zeros(len(hit), dtype=SEARCH_HIT_DTYPE)
        part["site"], part["pos"], part["record"], part["query"] = site[hit], pos[hit], rec[hit], k
        part["strand"], part["dist"] = strand[hit], dist[hit]
        mism = np.zeros(len(hit), dtype=np.uint64)
        for i in range(L):
            mism |= differs[hit, i].astype(np.uint64) << np.uint64(i)
        part["mism"] = mism
        parts.append(part)
        offsets[k + 1] = offsets[k] + np.uint64(len(hit))
        profile[k] = np.bincount(dist[hit], minlength=max_dist + 1)
    rows = np.concatenate(parts) if parts else np.zeros(0, dtype=SEARCH_HIT_DTYPE)
    return offsets, rows, profile


def brute_force_fasta(datas, pattern, queries, max_dist):
    return brute_force(lu.parse(datas), pattern, queries, max_dist)


def site_text(site, L, mism=0):
    """Packed site -> text, the positions of `mism` in lower case."""
    out = ""
    for i in range(L):
        ch = "ACGT"[(int(site) >> (2 * i)) & 3]
        out += ch.lower() if (int(mism) >> i) & 1 else ch
    return out


def as_tuples(rows, L):
    """Rows -> [(query, record, pos, strand, dist, site text with mismatches in lower case)]."""
    return [(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["dist"]), site_text(r["site"], L, r["mism"]))
            for r in rows]


def format_rows(records, queries, rows):
    """What bin/isslSearchGenome prints for these rows."""
    out = []
    for r in rows:
        q = _text(queries[int(r["query"])])
        out.append(b"%s\t%s\t%d\t%s\t%d\t%s\n" % (q.encode(), records[int(r["record"])][0], int(r["pos"]),
                                                   b"-" if r["strand"] else b"+", int(r["dist"]),
                                                   site_text(r["site"], len(q), r["mism"]).encode()))
    return b"".join(out)


def format_profile(queries, profile):
    return b"".join(b"%s\t%s\n" % (_text(q).encode(), b"\t".join(b"%d" % int(c) for c in row)) for q, row in zip(queries, profile))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))
