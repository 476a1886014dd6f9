"""Expected rows for the variant-aware genome search tests: a numpy brute force written from the definition of
issl_genome_search_variants in include/issl_hip.h (window, strand, hit, row), not from the kernel, in the style of
tests/search_util.py.  Every window of every record is a row of SETS of bases per strand (a set is a 4-bit mask, bit b =
base b of ACGT); the pattern is a set per position, a position matches when the query's base lies in the intersection.
Beside it a character-level VCF reader and SNP applier for issl_vcf_snps / issl_genome_apply_snps."""
import numpy as np

from crackling_amd import SNP_DTYPE, VARIANT_HIT_DTYPE
import locate_util as lu
from search_util import IUPAC

SET_OF = {code: sum(1 << "ACGT".index(b) for b in bases) for code, bases in IUPAC.items()}
LETTER_OF = {mask: code for code, mask in SET_OF.items()}
TEXT_CODES = "ACGTRYSWKMBDHV"  # what a window may hold: N is none of them
_SET = np.zeros(256, dtype=np.uint8)
for _c in TEXT_CODES:
    _SET[ord(_c)] = SET_OF[_c]
_COMP = np.array([sum(1 << (3 - b) for b in range(4) if m >> b & 1) for m in range(16)], dtype=np.uint8)  # A<->T, C<->G
_SIZE = np.array([bin(m).count("1") for m in range(16)], dtype=np.int64)
BLANKS = b" \t\n\v\f\r"


def _text(x):
    return x.decode() if isinstance(x, (bytes, bytearray)) else x


def candidates(records, pattern, max_variants):
    """Every (record, pos, strand) the pattern admits, in that order: -> (record, pos, strand, n_var, T[S, L] the sets the
    strand reads, A[S, L] the same cut by the pattern)."""
    pattern = _text(pattern).upper()
    L = len(pattern)
    allowed = np.array([SET_OF[ch] for ch in pattern], dtype=np.uint8)
    recs, poss, strands, nvars, ts = [], [], [], [], []
    for r, (_, seq) in enumerate(records):
        if len(seq) < L:
            continue
        w = np.lib.stride_tricks.sliding_window_view(_SET[np.frombuffer(seq, dtype=np.uint8)], L)
        n_var = (_SIZE[w] > 1).sum(axis=1)
        keep = np.flatnonzero((w != 0).all(axis=1) & (n_var <= max_variants))
        w = w[keep]
        for strand, t in ((0, w), (1, _COMP[w[:, ::-1]])):
            ok = ((t & allowed) != 0).all(axis=1)
            recs.append(np.full(int(ok.sum()), r, dtype=np.int64))
            poss.append(keep[ok])
            strands.append(np.full(int(ok.sum()), strand, dtype=np.int64))
            nvars.append(n_var[keep][ok])
            ts.append(np.ascontiguousarray(t[ok]))
    if not recs:
        return (np.zeros(0, np.int64),) * 4 + (np.zeros((0, L), np.uint8),) * 2
    rec, pos, strand, n_var, t = (np.concatenate(x) for x in (recs, poss, strands, nvars, ts))
    order = np.lexsort((strand, pos, rec))
    return rec[order], pos[order], strand[order], n_var[order], t[order], t[order] & allowed


def brute_force(records, pattern, queries, max_dist, max_variants):
    """-> (offsets uint64[n + 1], rows in VARIANT_HIT_DTYPE, profile uint64[n, max_dist + 1])."""
    L = len(pattern)
    rec, pos, strand, n_var, t, a = candidates(records, pattern, max_variants)
    site = np.zeros((len(t), 4), dtype=np.uint32)
    for b in range(4):
        for i in range(L):
            site[:, b] |= ((t[:, i] >> b) & 1).astype(np.uint32) << np.uint32(i)
    offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    profile = np.zeros((len(queries), max_dist + 1), dtype=np.uint64)
    parts = []
    for k, q in enumerate(queries):
        q = _text(q).upper()
        assert len(q) == L and set(q) <= set("ACGTN")
        differs = np.zeros((len(t), L), dtype=bool)
        for i, ch in enumerate(q):
            if ch != "N":
                differs[:, i] = (a[:, i] & SET_OF[ch]) == 0
        dist = differs.sum(axis=1)
        hit = np.flatnonzero(dist <= max_dist)
        part = np.zeros(len(hit), dtype=VARIANT_HIT_DTYPE)
        part["pos"], part["site"], part["record"], part["query"] = pos[hit], site[hit], rec[hit], k
        part["strand"], part["dist"], part["n_var"] = strand[hit], dist[hit], n_var[hit]
        mism = np.zeros(len(hit), dtype=np.uint64)
        for i in range(L):
            mism |= differs[hit, i].astype(np.uint64) << np.uint64(i)
        part["mism"] = mism
        parts.append(part)
        offsets[k + 1] = offsets[k] + np.uint64(len(hit))
        profile[k] = np.bincount(dist[hit], minlength=max_dist + 1)
    rows = np.concatenate(parts) if parts else np.zeros(0, dtype=VARIANT_HIT_DTYPE)
    return offsets, rows, profile


def brute_force_fasta(datas, pattern, queries, max_dist, max_variants):
    return brute_force(lu.parse(datas), pattern, queries, max_dist, max_variants)


def from_plain(rows, L):
    """Rows of the plain search (SEARCH_HIT_DTYPE) as the variant search gives them: site one-hot, n_var = 0."""
    out = np.zeros(len(rows), dtype=VARIANT_HIT_DTYPE)
    for f in ("pos", "record", "query", "mism", "strand", "dist"):
        out[f] = rows[f]
    for i in range(L):
        code = (rows["site"] >> np.uint64(2 * i)) & np.uint64(3)
        for b in range(4):
            out["site"][:, b] |= (code == b).astype(np.uint32) << np.uint32(i)
    return out


def site_text(site, L, mism=0):
    """The four masks of a row -> IUPAC letters, the positions of `mism` in lower case."""
    out = ""
    for i in range(L):
        ch = LETTER_OF[sum(((int(site[b]) >> i) & 1) << b for b in range(4))]
        out += ch.lower() if (int(mism) >> i) & 1 else ch
    return out


def as_tuples(rows, L):
    """Rows -> [(query, record, pos, strand, dist, n_var, site text with mismatches in lower case)]."""
    return [(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["dist"]), int(r["n_var"]),
             site_text(r["site"], L, r["mism"])) for r in rows]


def format_rows(records, queries, rows):
    """What bin/isslSearchGenome --variants prints for these rows."""
    out = []
    for r in rows:
        q = _text(queries[int(r["query"])])
        out.append(b"%s\t%s\t%d\t%s\t%d\t%s\n" % (q.encode(), records[int(r["record"])][0], int(r["pos"]),
                                                   b"-" if r["strand"] else b"+", int(r["dist"]),
                                                   site_text(r["site"], len(q), r["mism"]).encode()))
    return b"".join(out)


def format_profile(queries, profile):
    return b"".join(b"%s\t%s\n" % (_text(q).encode(), b"\t".join(b"%d" % int(c) for c in row)) for q, row in zip(queries, profile))


# ---- SNPs ---------------------------------------------------------------------------------------------------------------

# a file with one line of every kind, and the records it is read against
VCF = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\n"
       b"chr1\t3\t.\tG\tA\t.\n"              # a SNP
       b"chr1\t5\trs1\ta\tc,G\t.\tPASS\r\n"  # multi-allelic, lower case, \r\n
       b"chr1\t7\t.\tAT\tA\t.\n"             # a deletion: REF is not one base
       b"chr1\t8\t.\tC\tCT,<DEL>,*,.,T\n"    # four alleles skipped, T taken
       b"chr1\t9\t.\tC\t<DEL>\n"             # no usable allele
       b"chrX\t1\t.\tA\tC\n"                 # unknown CHROM
       b"\n"
       b"chr2\t11\t.\tA\tC\n"                # POS past the end of chr2 (10 bases)
       b"chr2\t0\t.\tA\tC\n"                 # POS 0
       b"chr2\t10\t.\tT\tG")                 # the last base, no line end
VCF_RECORDS = [(b"chr1 the first", 20), (b"chr2\tsecond", 10), (b"chr1", 5)]


class Malformed(Exception):
    def __init__(self, line):
        super().__init__("line %d" % line)
        self.line = line


def vcf_snps(vcf, records):
    """issl_vcf_snps character by character.  records: [(name, sequence or length)].  -> (SNP_DTYPE array, counts dict);
    raises Malformed(line number, 1-based)."""
    names, lengths = {}, []
    for r, (name, seq) in enumerate(records):
        short = bytes(name)
        for i, ch in enumerate(short):
            if ch in BLANKS:
                short = short[:i]
                break
        names.setdefault(short, r)
        lengths.append(seq if isinstance(seq, int) else len(seq))
    counts = dict(lines=0, snps=0, alleles_skipped=0, no_allele=0, unknown_chrom=0, beyond_record=0)
    out = []
    lines = bytes(vcf).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b"#"):
            continue
        fields = line.split(b"\t")
        if len(fields) < 5 or not fields[1] or any(ch not in b"0123456789" for ch in fields[1]):
            raise Malformed(no)
        counts["lines"] += 1
        chrom, pos, ref, alts = fields[0], int(fields[1]), fields[3].upper(), fields[4].upper().split(b",")
        if chrom not in names:
            counts["unknown_chrom"] += 1
            continue
        r = names[chrom]
        if pos == 0 or pos > lengths[r]:
            counts["beyond_record"] += 1
            continue
        ref_ok = len(ref) == 1 and ref in b"ACGT"
        alt = 0
        for allele in alts:
            if ref_ok and len(allele) == 1 and allele in b"ACGT":
                alt |= 1 << b"ACGT".index(allele)
            else:
                counts["alleles_skipped"] += 1
        if not alt:
            counts["no_allele"] += 1
            continue
        out.append((pos - 1, r, 1 << b"ACGT".index(ref), alt, (0, 0)))
    counts["snps"] = len(out)
    return np.array(out, dtype=SNP_DTYPE) if out else np.zeros(0, dtype=SNP_DTYPE), counts


class Refused(Exception):
    def __init__(self, index):
        super().__init__("snp %d" % index)
        self.index = index


def apply_snps(records, snps):
    """issl_genome_apply_snps on [(name, upper-case sequence)]: -> (the new records, the number of places changed); raises
    Refused(the smallest failing input index) and changes nothing."""
    seqs = [bytearray(s) for _, s in records]
    for k, s in enumerate(snps):
        if int(s["record"]) >= len(seqs) or int(s["pos"]) >= len(seqs[int(s["record"])]) or int(s["ref"]) not in (1, 2, 4, 8) \
                or not 1 <= int(s["alt"]) <= 15:
            raise Refused(k)
    places = {}
    for k, s in enumerate(snps):
        at = (int(s["record"]), int(s["pos"]))
        if at in places and places[at][0] != int(s["ref"]):
            raise Refused(k)
        first = places.get(at, (int(s["ref"]), 0, k))
        places[at] = (first[0], first[1] | int(s["alt"]), first[2])
    failed = [k for (r, p), (ref, alt, k) in places.items() if not int(_SET[seqs[r][p]]) & ref or int(_SET[seqs[r][p]]) | alt == 15]
    if failed:
        raise Refused(min(failed))
    changed = 0
    for (r, p), (ref, alt, k) in places.items():
        new = ord(LETTER_OF[int(_SET[seqs[r][p]]) | alt])
        changed += new != seqs[r][p]
        seqs[r][p] = new
    return [(name, bytes(s)) for (name, _), s in zip(records, seqs)], changed
