"""Expected rows for the tests of the bulge search on a variant-aware text, from the definition of
issl_genome_search_bulges_variants in include/issl_hip.h: the bulge search with issl_genome_search_variants in the place of
issl_genome_search.  So the brute force is the loop of bulge_util.brute_force around variant_util.brute_force: for every
bulge b and break point i the derived pair is built and searched; the rows are merged by (query, record, pos, strand, b),
taking the least distance and then the smallest i; `mism` is mapped back to query coordinates."""
import numpy as np

from crackling_amd import BULGE_VARIANT_HIT_DTYPE
import bulge_util as bu
import locate_util as lu
import search_util as su
import variant_util as vu


def brute_force(records, pattern, queries, span, max_dist, max_dna, max_rna, max_variants, ties=None):
    """-> (offsets uint64[n + 1], rows in BULGE_VARIANT_HIT_DTYPE, profile uint64[n, R + D + 1, max_dist + 1]).  ties (a
    list): the keys (query, record, pos, strand, b) whose minimum two or more break points reach are appended."""
    pattern = su._text(pattern).upper()
    queries = [su._text(q).upper() for q in queries]
    found = {}  # (query, record, pos, strand, b) -> (dist, i, site, mism, n_var)
    reached = {}  # key -> the break points at the key's minimum so far
    for b, i in bu.alignments(span, max_dna, max_rna):
        _, rows, _ = vu.brute_force(records, bu.derived(pattern, span, b, i), [bu.derived(q, span, b, i) for q in queries], max_dist,
                                    max_variants)
        for r in rows:
            key = (int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), b)
            value = (int(r["dist"]), i, tuple(int(x) for x in r["site"]), bu.query_mism(r["mism"], span, b, i), int(r["n_var"]))
            if key in found and value[0] == found[key][0]:
                reached[key] += 1
            if key not in found or value[:2] < found[key][:2]:
                if key not in found or value[0] < found[key][0]:
                    reached[key] = 1
                found[key] = value
    if ties is not None:
        ties += sorted(k for k, c in reached.items() if c > 1)
    keys = sorted(found)
    rows = np.zeros(len(keys), dtype=BULGE_VARIANT_HIT_DTYPE)
    offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    profile = np.zeros((len(queries), max_rna + max_dna + 1, max_dist + 1), dtype=np.uint64)
    for k, key in enumerate(keys):
        dist, i, site, mism, n_var = found[key]
        rows[k] = (key[2], site, key[1], key[0], mism, key[3], dist, n_var, key[4], i, (0,) * 7)
        offsets[key[0] + 1] += 1
        profile[key[0], key[4] + max_rna, dist] += 1
    offsets = np.cumsum(offsets).astype(np.uint64)
    return offsets, rows, profile


def brute_force_fasta(datas, pattern, queries, span, max_dist, max_dna, max_rna, max_variants):
    return brute_force(lu.parse(datas), pattern, queries, span, max_dist, max_dna, max_rna, max_variants)


def from_bulges(rows, L):
    """Rows of the bulge search (BULGE_HIT_DTYPE) as this search gives them: site one-hot over L + bulge positions, n_var = 0."""
    out = np.zeros(len(rows), dtype=BULGE_VARIANT_HIT_DTYPE)
    for f in ("pos", "record", "query", "mism", "strand", "dist", "bulge", "at"):
        out[f] = rows[f]
    width = L + rows["bulge"].astype(np.int64)
    for i in range(32):
        code = (rows["site"] >> np.uint64(2 * i)) & np.uint64(3)
        for b in range(4):
            out["site"][:, b] |= ((code == b) & (i < width)).astype(np.uint32) << np.uint32(i)
    return out


def from_variants(rows):
    """Rows of the variant search (VARIANT_HIT_DTYPE) as this search gives them with D = R = 0: bulge = at = 0."""
    out = np.zeros(len(rows), dtype=BULGE_VARIANT_HIT_DTYPE)
    for f in ("pos", "site", "record", "query", "mism", "strand", "dist", "n_var"):
        out[f] = rows[f]
    return out


def aligned(query, row, span):
    """(query aligned, site aligned) as bin/isslSearchGenome prints them: the site in IUPAC letters, lower case where a
    paired position does not match, '-' at an RNA bulge."""
    L, b, brk = len(query), int(row["bulge"]), span[0] + int(row["at"])
    d, r = max(b, 0), max(-b, 0)
    letters = vu.site_text(row["site"], L + b)
    site = ""
    for s in range(L + b):
        if s < brk:
            j = s
        elif s < brk + d:
            j = None  # an unpaired base of the site: upper case
        else:
            j = s - b
        site += letters[s].lower() if j is not None and (int(row["mism"]) >> j) & 1 else letters[s]
    return query[:brk] + "-" * d + query[brk:], site[:brk] + "-" * r + site[brk:]


def as_tuples(rows, L):
    """Rows -> [(query, record, pos, strand, dist, bulge, at, n_var, site text, mism)]."""
    return [(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["dist"]), int(r["bulge"]), int(r["at"]),
             int(r["n_var"]), vu.site_text(r["site"], L + int(r["bulge"])), int(r["mism"])) for r in rows]


def format_rows(records, queries, rows, span):
    """What bin/isslSearchGenome --guide .. --guide-variants prints for these rows."""
    out = []
    for r in rows:
        q, site = aligned(su._text(queries[int(r["query"])]), r, span)
        out.append(b"%s\t%s\t%d\t%s\t%d\t%s\t%s\n" % (q.encode(), records[int(r["record"])][0], int(r["pos"]),
                                                       b"-" if r["strand"] else b"+", int(r["dist"]),
                                                       bu.bulge_name(int(r["bulge"])).encode(), site.encode()))
    return b"".join(out)


format_profile = bu.format_profile
of_queries = bu.of_queries
