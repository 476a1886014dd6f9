"""Expected rows for the search on the ALT haplotypes of indels (issl_haplotypes_* of include/issl_hip.h), in the style of
tests/variant_util.py.  whole_record() is the definition: one indel applied to its whole record, the variant search's
brute force on that one record, the windows that overlap the edit, mapped back to the reference.  strips() is the model of
what the library builds -- the strip of every indel as a record of a second text -- for cases too large for
whole_record(); tests/test_haplotypes_model.py pins it to the definition.  Beside them a character-level issl_vcf_indels."""
import numpy as np

from crackling_amd import HAPLOTYPE_HIT_DTYPE, INDEL_DTYPE
import variant_util as vu

MAX_ALLELE = 65535  # ISSL_INDEL_MAX_ALLELE


def _bytes(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def trim(ref, alt):
    """The common suffix first, then the common prefix of what is left.  -> (prefix removed, REF', ALT')"""
    ref, alt = _bytes(ref).upper(), _bytes(alt).upper()
    s = 0
    while s < min(len(ref), len(alt)) and ref[len(ref) - 1 - s] == alt[len(alt) - 1 - s]:
        s += 1
    ref, alt = ref[:len(ref) - s], alt[:len(alt) - s]
    p = 0
    while p < min(len(ref), len(alt)) and ref[p] == alt[p]:
        p += 1
    return p, ref[p:], alt[p:]


def make_indels(entries):
    """[(record, pos, REF, ALT)] -> (INDEL_DTYPE array, allele text): REF then ALT of every entry, as given."""
    out = np.zeros(len(entries), dtype=INDEL_DTYPE)
    text = b""
    for k, (record, pos, ref, alt) in enumerate(entries):
        ref, alt = _bytes(ref), _bytes(alt)
        out[k] = (pos, record, len(ref), len(alt), len(text), len(text) + len(ref), 0)
        text += ref + alt
    return out, text


def edits(indels, alleles):
    """-> [(record, p, REF', ALT')] of the entries, trimmed."""
    out = []
    for d in indels:
        ref = alleles[int(d["ref_at"]):int(d["ref_at"]) + int(d["ref_len"])]
        alt = alleles[int(d["alt_at"]):int(d["alt_at"]) + int(d["alt_len"])]
        cut, r, a = trim(ref, alt)
        assert r or a, "an entry that changes nothing"
        out.append((int(d["record"]), int(d["pos"]) + cut, r, a))
    return out


def _assemble(n_queries, max_dist, per_indel):
    """per_indel: [(offsets, rows in HAPLOTYPE_HIT_DTYPE)] in input order -> rows by (query, indel, ...), offsets, profile."""
    offsets = np.zeros(n_queries + 1, dtype=np.uint64)
    profile = np.zeros((n_queries, max_dist + 1), dtype=np.uint64)
    parts = []
    for k in range(n_queries):
        count = 0
        for off, rows in per_indel:
            part = rows[int(off[k]):int(off[k + 1])]
            parts.append(part)
            count += len(part)
            profile[k] += np.bincount(part["dist"], minlength=max_dist + 1).astype(np.uint64)
        offsets[k + 1] = offsets[k] + np.uint64(count)
    rows = np.concatenate(parts) if parts else np.zeros(0, dtype=HAPLOTYPE_HIT_DTYPE)
    return offsets, rows, profile


def _rows(found, record, indel, pos, edit_at):
    out = np.zeros(len(found), dtype=HAPLOTYPE_HIT_DTYPE)
    for f in ("site", "query", "mism", "strand", "dist", "n_var"):
        out[f] = found[f]
    out["record"], out["indel"], out["pos"], out["edit_at"] = record, indel, pos, edit_at
    return out


def whole_record(records, indels, alleles, pattern, queries, max_dist, max_variants):
    """THE DEFINITION.  records: [(name, upper-case sequence)], the text as it stands at the open (codes of applied SNPs
    included).  -> (offsets uint64[n + 1], rows in HAPLOTYPE_HIT_DTYPE, profile uint64[n, max_dist + 1])."""
    W = len(pattern)
    per_indel = []
    for k, (record, p, r, a) in enumerate(edits(indels, alleles)):
        seq = bytes(records[record][1])
        assert p + len(r) <= len(seq)
        hap = seq[:p] + a + seq[p + len(r):]
        off, found, _ = vu.brute_force([(b"", hap)], pattern, queries, max_dist, max_variants)
        s = found["pos"].astype(np.int64)
        if a:
            keep = (s < p + len(a)) & (s + W > p)       # holds at least one base of ALT'
        else:
            keep = (s < p) & (s + W > p)                # holds the base ahead of the junction and the base behind it
        pos = np.where(s < p, s, np.where(s < p + len(a), p, p + len(r) + s - p - len(a)))
        kept = np.concatenate([[0], np.cumsum(keep)])
        per_indel.append((kept[off.astype(np.int64)], _rows(found[keep], record, k, pos[keep], (p - s)[keep])))
    return _assemble(len(queries), max_dist, per_indel)


def strip_texts(records, indels, alleles, W):
    """-> [(left flank length, strip bytes)] per entry: min(W - 1, p) bases ahead of the edit, ALT', min(W - 1, what is
    left) bases behind REF'."""
    out = []
    for record, p, r, a in edits(indels, alleles):
        seq = bytes(records[record][1])
        left = min(W - 1, p)
        right = min(W - 1, len(seq) - p - len(r))
        out.append((left, seq[p - left:p] + a + seq[p + len(r):p + len(r) + right]))
    return out


def strips(records, indels, alleles, pattern, queries, max_dist, max_variants):
    """The model of the library: the strips as the records of a second text, one brute force over all of them, every row
    mapped through the strip's table entry.  Same result as whole_record()."""
    W = len(pattern)
    ed = edits(indels, alleles)
    texts = strip_texts(records, indels, alleles, W)
    off, found, profile = vu.brute_force([(b"", t) for _, t in texts], pattern, queries, max_dist, max_variants)
    k = found["record"].astype(np.int64)
    s = found["pos"].astype(np.int64)
    rec = np.array([e[0] for e in ed], dtype=np.int64)[k] if len(ed) else k
    p = np.array([e[1] for e in ed], dtype=np.int64)[k] if len(ed) else k
    r_len = np.array([len(e[2]) for e in ed], dtype=np.int64)[k] if len(ed) else k
    a_len = np.array([len(e[3]) for e in ed], dtype=np.int64)[k] if len(ed) else k
    left = np.array([t[0] for t in texts], dtype=np.int64)[k] if len(ed) else k
    pos = np.where(s < left, p - left + s, np.where(s < left + a_len, p, p + r_len + (s - left - a_len)))
    return off, _rows(found, rec, k, pos, left - s), profile


def format_rows(records, queries, rows, indels, alleles):
    """What bin/isslSearchGenome --indel-vcf prints for these rows."""
    ed = edits(indels, alleles)
    out = []
    for r in rows:
        line = vu.format_rows(records, queries, np.array([r])[["pos", "site", "record", "query", "mism", "strand", "dist"]])
        _, p, ref, alt = ed[int(r["indel"])]
        out.append(line[:-1] + b"\t%d:%s>%s\t%d\n" % (p + 1, ref or b"-", alt or b"-", int(r["edit_at"])))
    return b"".join(out)


# ---- the VCF reader -----------------------------------------------------------------------------------------------------

# a file with one line of every kind, and the records it is read against
VCF = (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\n"
       b"chr1\t3\t.\tGA\tG\t.\n"                   # a deletion
       b"chr1\t5\trs1\ta\tacc,AG\t.\tPASS\r\n"     # two insertions, lower case, \r\n
       b"chr1\t7\t.\tAT\tCG,aT,At\t.\n"            # a two-base substitution; ALT equal to REF ignoring case, twice
       b"chr1\t8\t.\tC\tT,CT,<DEL>,*,.,CTT\n"      # a SNP (the other reader's), an indel, three skipped, an indel
       b"chr1\t9\t.\tC\t<DEL>\n"                   # nothing usable
       b"chr1\t9\t.\tC\tG\n"                       # a SNP alone
       b"chr1\t10\t.\tCN\tC,CTT\n"                 # REF not all ACGT: both alleles skipped
       b"chr1\t11\t.\t\tC\n"                       # an empty REF
       b"chr1\t12\t.\tACG\tT,\n"                   # a complex allele and an empty one
       b"chrX\t1\t.\tAC\tA\n"                      # unknown CHROM
       b"\n"
       b"chr2\t11\t.\tAC\tA\n"                     # POS past the end of chr2 (10 bases)
       b"chr2\t0\t.\tAC\tA\n"                      # POS 0
       b"chr2\t9\t.\tACG\tA\n"                     # REF runs past the record's end
       b"chr2\t9\t.\tAC\tA,ACGTACGT")              # the last bases, no line end
VCF_RECORDS = [(b"chr1 the first", 20), (b"chr2\tsecond", 10), (b"chr1", 5)]


def vcf_indels(vcf, records):
    """issl_vcf_indels character by character.  records: [(name, sequence or length)].  -> (INDEL_DTYPE array, the allele
    text, counts dict); raises variant_util.Malformed(line number, 1-based)."""
    names, lengths = {}, []
    for r, (name, seq) in enumerate(records):
        short = bytes(name)
        for i, ch in enumerate(short):
            if ch in vu.BLANKS:
                short = short[:i]
                break
        names.setdefault(short, r)
        lengths.append(seq if isinstance(seq, int) else len(seq))
    counts = dict(lines=0, indels=0, alleles_skipped=0, no_allele=0, unknown_chrom=0, beyond_record=0, too_long=0)
    out, text = [], b""
    lines = bytes(vcf).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()

    def bases(x):
        return len(x) >= 1 and all(ch in b"ACGTacgt" for ch in x)

    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b"#"):
            continue
        fields = line.split(b"\t")
        if len(fields) < 5 or not fields[1] or any(ch not in b"0123456789" for ch in fields[1]):
            raise vu.Malformed(no)
        counts["lines"] += 1
        chrom, pos, ref, alts = fields[0], int(fields[1]), fields[3], fields[4].split(b",")
        if chrom not in names:
            counts["unknown_chrom"] += 1
            continue
        r = names[chrom]
        if pos == 0 or pos > lengths[r]:
            counts["beyond_record"] += 1
            continue
        if not bases(ref):
            counts["alleles_skipped"] += len(alts)
            counts["no_allele"] += 1
            continue
        if pos - 1 + len(ref) > lengths[r]:
            counts["beyond_record"] += 1
            continue
        gave = False
        for alt in alts:
            if not bases(alt) or alt.upper() == ref.upper() or (len(ref) == 1 and len(alt) == 1):
                counts["alleles_skipped"] += 1
            elif len(ref) > MAX_ALLELE or len(alt) > MAX_ALLELE:
                counts["too_long"] += 1
            else:
                out.append((pos - 1, r, len(ref), len(alt), len(text), len(text) + len(ref), 0))
                text += ref + alt
                gave = True
        if not gave:
            counts["no_allele"] += 1
    counts["indels"] = len(out)
    return (np.array(out, dtype=INDEL_DTYPE) if out else np.zeros(0, dtype=INDEL_DTYPE)), text, counts
