"""Expected locations for the locate tests: the records of FASTA inputs as the extraction joins them, restated in Python,
and a brute-force pass over their text with the two patterns of extractOfftargets.py:23-24 as plain character tests."""
import numpy as np

BLANK = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"  # what str.strip() removes from ASCII text
_CODE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k


def _lines(data):
    """Python's text mode: "\\n", "\\r\\n" and a lone "\\r" each end a line.  -> [(line without its end, has an end)]"""
    out, p = [], 0
    while p < len(data):
        e = p
        while e < len(data) and data[e] not in (10, 13):
            e += 1
        nxt = min(e + 1, len(data))
        if data[e:e + 2] == b"\r\n":
            nxt = e + 2
        out.append((data[p:e], e < len(data)))
        p = nxt
    return out


def parse_single(data):
    """One input: every line is stripped, a stripped line that starts with '>' opens a record (str.strip() / '>'); text
    ahead of the first header is a record with an empty name; blank lines are skipped.  -> [(name, sequence)]"""
    recs = []
    for line, _ in _lines(data):
        st = line.strip(BLANK)
        if not st:
            continue
        if st[:1] == b">":
            recs.append([line[line.index(b">") + 1:], b""])
        else:
            if not recs:
                recs.append([b"", b""])
            recs[-1][1] += st.upper()
    return [(n, s) for n, s in recs]


def parse_multi(datas):
    """Several inputs: a line is a header when its first raw character is '>', other lines lose their trailing blanks
    only; of the records of one file with the same header line the last one survives; the lines ahead of the first
    header are a record with an empty name when they hold text."""
    out = []
    for data in datas:
        recs, cur = [], None
        for line, ended in _lines(data):
            if line[:1] == b">":
                cur = [(line[1:], ended), line[1:], b""]
                recs.append(cur)
            else:
                if cur is None:
                    cur = [None, b"", b""]
                    recs.append(cur)
                cur[2] += line.rstrip(BLANK).upper()
        last = {r[0]: i for i, r in enumerate(recs) if r[0] is not None}
        for i, r in enumerate(recs):
            if r[0] is None:
                if r[2]:
                    out.append((r[1], r[2]))
            elif last[r[0]] == i:
                out.append((r[1], r[2]))
    return out


def parse(datas):
    datas = list(datas)
    return parse_single(datas[0]) if len(datas) == 1 else parse_multi(datas)


LOC_DTYPE = np.dtype([("site", "<u8"), ("record", "<u4"), ("pos", "<u8"), ("strand", "<u4")])


def brute_force(records):
    """Every match of the forward pattern [ACG][ACGT]{19}[ACGT][AG]G (strand 0, site = seq[i:i+20]) and of the reverse
    pattern C[CT][ACGT][ACGT]{19}[TGC] (strand 1, site = reverse complement of seq[i:i+20]) at every start i of every
    record, as packed signatures (base p in bits 2p, 2p + 1).  Sorted by (record, pos, strand)."""
    parts = []
    for r, (_, seq) in enumerate(records):
        n = len(seq) - 22
        if n <= 0:
            continue
        c = _CODE[np.frombuffer(seq, dtype=np.uint8)]
        bad = np.concatenate([[0], np.cumsum(c >= 4)])
        i = np.arange(n)
        body = (bad[i + 21] - bad[i + 1]) == 0  # characters 1..20 are [ACGT] in both patterns
        c0, c1, c21, c22 = c[:n], c[1:n + 1], c[21:21 + n], c[22:22 + n]
        fwd = body & (c0 < 3) & ((c21 == 0) | (c21 == 2)) & (c22 == 2)
        rev = body & (c0 == 1) & ((c1 == 1) | (c1 == 3)) & (c21 < 4) & ((c22 == 3) | (c22 == 2) | (c22 == 1))
        for strand, hit in ((0, fwd), (1, rev)):
            at = np.flatnonzero(hit)
            sig = np.zeros(len(at), dtype=np.uint64)
            for p in range(20):
                base = c[at + p] if strand == 0 else 3 - c[at + 19 - p]
                sig |= base.astype(np.uint64) << np.uint64(2 * p)
            part = np.zeros(len(at), dtype=LOC_DTYPE)
            part["site"], part["record"], part["pos"], part["strand"] = sig, r, at, strand
            parts.append(part)
    if not parts:
        return np.zeros(0, dtype=LOC_DTYPE)
    out = np.concatenate(parts)
    return out[np.lexsort((out["strand"], out["pos"], out["record"]))]


def sig_text(sigs):
    """Packed signatures -> 20-mers (bytes)."""
    sigs = np.asarray(sigs, dtype=np.uint64)
    chars = np.empty((len(sigs), 20), dtype=np.uint8)
    for p in range(20):
        chars[:, p] = np.frombuffer(b"ACGT", dtype=np.uint8)[((sigs >> np.uint64(2 * p)) & np.uint64(3)).astype(np.int64)]
    return [bytes(row) for row in chars]


def expected_by_site(truth):
    """brute_force() output -> {site: array of (record, pos, strand) rows in that order}."""
    order = np.argsort(truth["site"], kind="stable")
    srt = truth[order]
    cuts = np.flatnonzero(np.diff(srt["site"])) + 1
    return {int(g["site"][0]): g for g in np.split(srt, cuts) if len(g)}


def check_locate(genome_records, offsets, locs, sites, truth):
    """Everything the contract says about one locate call: complete offsets, per site the brute force's list in
    (record, pos, strand) order, empty ranges for sites that do not occur."""
    by_site = expected_by_site(truth)
    assert len(offsets) == len(sites) + 1 and int(offsets[0]) == 0 and int(offsets[-1]) == len(locs)
    assert np.all(np.diff(offsets.astype(np.int64)) >= 0)
    for k, s in enumerate(np.asarray(sites, dtype=np.uint64)):
        got = locs[int(offsets[k]):int(offsets[k + 1])]
        want = by_site.get(int(s))
        if want is None:
            assert len(got) == 0, (k, hex(int(s)))
            continue
        assert len(got) == len(want), (k, len(got), len(want))
        assert np.array_equal(got["record"], want["record"]) and np.array_equal(got["pos"], want["pos"]) and \
            np.array_equal(got["strand"], want["strand"]), k
    if genome_records is not None:
        assert len(locs) == 0 or int(locs["record"].max()) < len(genome_records)
