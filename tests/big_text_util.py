"""A genome text beyond 2^32 positions that costs a model nothing (tests/test_big_text_model.py, tests/test_big_text_gpu.py).

No reader of a genome handle admits a window that holds a byte outside its alphabet, and `N` is outside every reader's.  A
text that is `N` everywhere but for small ISLANDS of real sequence has its rows inside the islands, wherever they lie: the
device walks all 2^20 tiles of 4096 positions with 64-bit addresses, the models look at the islands alone.

The layout is data: three records r0 (64 KiB), r1 (2^32 + 64 KiB) and r2 (64 KiB).  The resident text holds the records one
behind the other with one '\\n' behind each (crackling_amd/csrc/issl_locate.hip), so r1 starts at text position 65 537, the
text position 2^32 is r1's position 2^32 - 65 537, r1's own position 2^32 lies 65 537 text positions later, and r2 starts at
2^32 + 131 074.  The text is 2^32 + 196 611 bytes long: pos_bits = 33.

    big()          the Layout of that text
    shrunk(gap)    the same records and islands with every run of N cut to `gap` bytes: small enough for the whole-record
                   models, which is how the construction is checked without a device
    Layout.twin()  the small genome the models run on: one record per island, 64 N on either side, in text order; a row of
                   it becomes a row of the layout's text by translate_*()

The map (twin record, pos) -> (record, pos) is monotone in (record, pos), so the order (query, record, pos, strand) of every
row type survives the translation.  One reader's order does not: the guide extraction lists the forward matches of a whole
record ahead of its reverse matches, which no per-island order can say -- guide_rows() merges the islands' matches into that
order itself."""
import functools

import numpy as np

import guides_util as gu
import haplotype_util as hu

TILE = 4096          # kPosPerBlock: text positions per workgroup of every scan
T32 = 1 << 32
PAD = 64             # N on either side of an island in the twin; the widest window of a reader is 32 + 3
NAMES = (b"r0 sixty-four KiB", b"r1 across both crossings", b"r2")
LENGTHS = (1 << 16, T32 + (1 << 16), 1 << 16)
NONE = 0xFFFFFFFF
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def _starts(lengths):
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += n + 1
    return out, at


# ---- the islands ---------------------------------------------------------------------------------------------------------
# (name, record, where, length): `where` is a record position, ("text", p) for a text position of the big layout, or
# ("end", 0) for an island that ends on its record's last base.  Names that start with "snp" are reserved for the test that
# changes the text.
_S1 = LENGTHS[0] + 1
_PLAN = [
    ("r0-a", 0, 1000, 300),
    ("snp-r0", 0, 20000, 300),
    ("r0-b", 0, 40000, 250),
    ("low", 1, (1 << 30) + 12345, 300),                       # below 2^31
    ("high", 1, 3 * (1 << 30) + 777, 320),                    # between 2^31 and 2^32
    ("text-crossing", 1, ("text", T32 - 150), 300),           # windows start at every text position 2^32 - 150 .. 2^32 + 149
    ("snp-text", 1, ("text", T32 + 1000), 300),               # text position >= 2^32, record position < 2^32
    ("tile-start", 1, ("text", T32 + 2 * TILE), 260),         # starts on a tile border above 2^32
    ("tile-end", 1, ("text", T32 + 5 * TILE - 280), 280),     # ends on one
    ("record-crossing", 1, T32 - 150, 300),                   # the same straddle around r1's own position 2^32
    ("snp-record", 1, T32 + 2000, 300),                       # record position >= 2^32
    ("r1-end", 1, ("end", 0), 300),
    ("r2-start", 2, 0, 300),
    ("snp-r2", 2, 30000, 300),
    ("r2-end", 2, ("end", 0), 330),
]
# A crossing island holds, around the crossing c (its offset 150): a forward site of the extraction in the window c - 15
# (A at c - 15, AGG at c + 5), a reverse site in the window c - 12 (CC at c - 12, T at c + 10) and TTTA at c - 3 for the
# 5' pattern TTTV + 20 N.  Every one of these windows covers c - 1 and c.
_CROSSING = ((-15, b"A"), (5, b"AGG"), (-12, b"CC"), (10, b"T"), (-3, b"TTTA"))
# Words planted twice, (name, island and offset and strand of either copy): a word is 23 bases, a forward site with AGG.
# A copy on strand 1 is the word's reverse complement, which the occurrence calls read at its start, with AAC behind it:
# locate's reverse pattern reports the reverse complement of the FIRST 20 matched characters (extractOfftargets.py), so
# the word's site lies three bases further on, and the word ends in AG AGG to be admitted there.
# The copies of "B" and "E" would change their order if positions were compared in 32 bits.
_WORDS = [
    ("B", ("high", 40, 0), ("tile-start", 60, 0)),            # below and above 2^32, both forward
    ("C", ("r0-a", 50, 1), ("record-crossing", 200, 0)),      # below on the reverse strand, above forward
    ("D", ("tile-end", 30, 1), ("r2-start", 100, 0)),         # both above 2^32, in two records
    ("E", ("low", 200, 0), ("r2-end", 250, 1)),               # forward below 2^31, reverse in r2
    ("F", ("text-crossing", 250, 0), ("r1-end", 40, 1)),      # text position >= 2^32 < record position 2^32, and beyond
]


class Island:
    def __init__(self, name, record, start, seq):
        self.name, self.record, self.start, self.seq = name, record, start, seq

    @property
    def end(self):
        return self.start + len(self.seq)


@functools.lru_cache(maxsize=None)
def _island_texts(seed=20):
    rng = np.random.default_rng(seed)
    texts = {name: bytearray(_ACGT[rng.integers(0, 4, size=length)].tobytes()) for name, _, _, length in _PLAN}
    words = {}
    for name, *copies in _WORDS:
        word = b"G" + _ACGT[rng.integers(0, 4, size=17)].tobytes() + b"AGAGG"
        words[name] = word
        for island, at, strand in copies:
            plant = revcomp(word) + b"AAC" if strand else word
            texts[island][at:at + len(plant)] = plant
    for island in ("text-crossing", "record-crossing"):
        for at, what in _CROSSING:
            texts[island][150 + at:150 + at + len(what)] = what
    return {k: bytes(v) for k, v in texts.items()}, words


def words():
    """{name: the 23-mer planted twice}"""
    return dict(_island_texts()[1])


class Layout:
    """Records of N with islands in them.  lengths: the records' lengths; islands: in text order, at least PAD N between two
    of one record."""

    def __init__(self, lengths, islands):
        self.lengths, self.islands = tuple(lengths), list(islands)
        self.starts, self.text_len = _starts(self.lengths)
        for a, b in zip(self.islands, self.islands[1:]):
            assert (a.record, a.end + PAD) <= (b.record, b.start) or a.record < b.record, (a.name, b.name)
        for i in self.islands:
            assert 0 <= i.start and i.end <= self.lengths[i.record], i.name
        self.island_record = np.array([i.record for i in self.islands], dtype=np.int64)
        self.island_start = np.array([i.start for i in self.islands], dtype=np.int64)
        self.pos_bits = max(1, (max(2, self.text_len) - 1).bit_length())  # bits_for() of issl_locate.hip

    def index(self, name):
        return [i.name for i in self.islands].index(name)

    def island(self, name):
        return self.islands[self.index(name)]

    def text_pos(self, record, pos):
        """Position in the resident text of position `pos` of record `record` (arrays or numbers)."""
        return np.asarray(self.starts, dtype=np.int64)[np.asarray(record, dtype=np.int64)] + np.asarray(pos, dtype=np.int64)

    def with_texts(self, texts):
        """The same places with other island texts (of the same lengths): the text after SNPs."""
        assert [len(t) for t in texts] == [len(i.seq) for i in self.islands]
        return Layout(self.lengths, [Island(i.name, i.record, i.start, bytes(t)) for i, t in zip(self.islands, texts)])

    # -- the small genome the models run on
    def twin(self):
        """-> [(name, N * PAD + island + N * PAD)] in text order."""
        return [(b"twin %d %s" % (k, i.name.encode()), b"N" * PAD + i.seq + b"N" * PAD) for k, i in enumerate(self.islands)]

    def to_twin(self, record, pos):
        """(record, pos) inside an island -> (twin record, pos)."""
        for k, i in enumerate(self.islands):
            if i.record == record and i.start <= pos < i.end:
                return k, pos - i.start + PAD
        raise KeyError((record, pos))

    def from_twin(self, twin_record, pos):
        t = np.asarray(twin_record, dtype=np.int64)
        return self.island_record[t], np.asarray(pos, dtype=np.int64) - PAD + self.island_start[t]

    def translate(self, rows, pos="pos"):
        """Rows of the twin -> rows of this text: `record` and `pos` rewritten, every other field as it is."""
        out = rows.copy()
        if len(rows):
            out["record"], out[pos] = self.from_twin(rows["record"], rows[pos])
        return out

    # -- the whole text, for layouts small enough
    def whole_records(self):
        out = []
        for r, n in enumerate(self.lengths):
            seq = bytearray(b"N" * n)
            for i in self.islands:
                if i.record == r:
                    seq[i.start:i.end] = i.seq
            out.append((NAMES[r], bytes(seq)))
        return out

    def fasta_buffers(self, line=1 << 20):
        """One uint8 buffer per record: '>name\\n' and the record in lines of `line` bases.  Filled with N once; headers,
        line ends and islands are written into the buffer itself (joining bytes objects of this size costs several times
        the fill).  The lines are there for the host's FASTA pass, which hands whole lines to its threads: r1 on one line
        of 4 GiB is parsed by one of them, in 10 s instead of 1.5 s."""
        out = []
        for r, n in enumerate(self.lengths):
            head = b">" + NAMES[r] + b"\n"
            full = n // line
            buf = np.full(len(head) + n + (n + line - 1) // line, ord("N"), dtype=np.uint8)
            buf[:len(head)] = np.frombuffer(head, dtype=np.uint8)
            buf[len(head):len(head) + full * (line + 1)].reshape(full, line + 1)[:, line] = ord("\n")
            buf[-1] = ord("\n")
            for i in self.islands:
                if i.record == r:
                    at = np.arange(i.start, i.end)
                    buf[len(head) + at + at // line] = np.frombuffer(i.seq, dtype=np.uint8)
            out.append(buf)
        return out


@functools.lru_cache(maxsize=None)
def big():
    texts, _ = _island_texts()
    starts, _ = _starts(LENGTHS)
    islands = []
    for name, record, where, length in _PLAN:
        if isinstance(where, tuple):
            where = where[1] - starts[record] if where[0] == "text" else LENGTHS[record] - length
        islands.append(Island(name, record, where, texts[name]))
    return Layout(LENGTHS, islands)


@functools.lru_cache(maxsize=None)
def shrunk(gap):
    """big() with every run of N cut to `gap` bytes (shorter runs stay)."""
    b = big()
    lengths, islands = [], []
    for r in range(len(LENGTHS)):
        at, prev_end = 0, 0
        for i in b.islands:
            if i.record != r:
                continue
            at += min(gap, i.start - prev_end)
            islands.append(Island(i.name, r, at, i.seq))
            at += len(i.seq)
            prev_end = i.end
        lengths.append(at + min(gap, LENGTHS[r] - prev_end))
    return Layout(lengths, islands)


# ---- one translation per row type ------------------------------------------------------------------------------------------

def translate_locations(layout, locs):
    """LOCATION_DTYPE rows, and locate_util.brute_force's (site, record, pos, strand)."""
    return layout.translate(locs)


def translate_occurrences(layout, rows):
    """Occurrence rows: a row without a first occurrence (record 0xFFFFFFFF) stays as it is."""
    out = rows.copy()
    has = rows["record"] != NONE
    if has.any():
        rec, pos = layout.from_twin(rows["record"][has], rows["pos"][has])
        out["record"][has], out["pos"][has] = rec, pos
    return out


def translate_search(layout, rows):
    return layout.translate(rows)


translate_bulges = translate_variants = translate_bulge_variants = translate_landings = translate_search


def translate_haplotypes(layout, rows):
    """Haplotype rows: `record` and `pos` are the reference record and position; `indel` and `edit_at` stay."""
    return layout.translate(rows)


def translate_guides(layout, rows):
    return layout.translate(rows, "start")


def indels_to_twin(layout, indels):
    """INDEL_DTYPE entries of the layout's text -> the same entries on the twin."""
    out = indels.copy()
    for k, d in enumerate(indels):
        out["record"][k], out["pos"][k] = layout.to_twin(int(d["record"]), int(d["pos"]))
    return out


def snps_to_twin(layout, snps):
    out = snps.copy()
    for k, s in enumerate(snps):
        out["record"][k], out["pos"][k] = layout.to_twin(int(s["record"]), int(s["pos"]))
    return out


def haplotypes(layout, indels, alleles, pattern, queries, max_dist, max_variants):
    """haplotype_util.whole_record on the twin, translated: the indels are given in the layout's coordinates."""
    off, rows, prof = hu.whole_record(layout.twin(), indels_to_twin(layout, indels), alleles, pattern, queries, max_dist, max_variants)
    return off, translate_haplotypes(layout, rows), prof


def guide_rows(layout):
    """guides_util.brute_force of the layout's text from the islands: per record the forward matches of all its islands by
    position, then the reverse ones -- the order the reference meets them in."""
    met = []
    for k, (_, seq) in enumerate(layout.twin()):
        for start, strand, guide in gu.matches(seq):
            rec, pos = layout.from_twin(k, start)
            met.append((int(rec), strand, int(pos), guide))
    met.sort(key=lambda m: m[:3])
    first, seen = {}, {}
    for rec, strand, pos, guide in met:
        if guide in first:
            seen[guide] += 1
        else:
            first[guide], seen[guide] = (rec, pos, strand), 1
    rows = np.zeros(len(first), dtype=gu.ROW_DTYPE)
    for k, (guide, (rec, pos, strand)) in enumerate(first.items()):
        rows[k] = (guide, rec, pos, strand, seen[guide])
    return rows


# ---- what the rows of a reader are meant to contain ------------------------------------------------------------------------

def classes(layout, record, pos, width, strand=None):
    """Which of the classes the big text exists for the rows (record, pos, window width) fall into.  -> {name: count}"""
    record, pos = np.asarray(record, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    width = np.broadcast_to(np.asarray(width, dtype=np.int64), pos.shape)
    t = layout.text_pos(record, pos)
    out = {
        "text>=2^32,record<2^32": int(((t >= T32) & (pos < T32)).sum()),
        "record>=2^32": int((pos >= T32).sum()),
        "r2": int((record == 2).sum()),
        "covers the text crossing": int(((t < T32) & (t + width > T32)).sum()),
        "covers the record crossing": int(((record == 1) & (pos < T32) & (pos + width > T32)).sum()),
    }
    if strand is not None:
        strand = np.asarray(strand)
        out["strand 0"], out["strand 1"] = int((strand == 0).sum()), int((strand == 1).sum())
    return out


def assert_classes(layout, record, pos, width, strand=None, but=()):
    got = classes(layout, record, pos, width, strand)
    missing = [k for k, v in got.items() if v == 0 and k not in but]
    assert not missing, (missing, got)
    return got


def masked_lookup(layout, record, pos):
    """What (record, pos) would read if the text position were cut to 32 bits ahead of the search in the record table."""
    starts = np.asarray(layout.starts, dtype=np.int64)
    t = layout.text_pos(record, pos) & (T32 - 1)
    rec = np.searchsorted(starts, t, "right") - 1
    return rec, t - starts[rec]


# ---- the text after SNPs, and the indels ---------------------------------------------------------------------------------

# (island, offset, alt bases as a step from the reference base: 1..3, or two steps for two alleles)
_SNPS = [(island, at, alt) for island in ("snp-r0", "snp-text", "snp-record", "snp-r2")
         for at, alt in ((3, (1,)), (31, (2,)), (33, (1, 3)), (90, (3,)), (91, (1,)), (140, (2,)), (199, (1, 2)), (260, (3,)), (299, (1,)))]


def snps(layout):
    """The SNPs of the reserved islands in the layout's coordinates, as crackling_amd.SNP_DTYPE rows in text order."""
    from crackling_amd import SNP_DTYPE
    out = np.zeros(len(_SNPS), dtype=SNP_DTYPE)
    for k, (name, at, alts) in enumerate(_SNPS):
        i = layout.island(name)
        ref = b"ACGT".index(i.seq[at])
        out[k] = (i.start + at, i.record, 1 << ref, sum(1 << ((ref + a) % 4) for a in alts), (0, 0))
    return out


def snps_vcf(layout, rows):
    """SNP rows as the lines of a VCF."""
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for s in rows:
        alts = b",".join(b"ACGT"[b:b + 1] for b in range(4) if int(s["alt"]) >> b & 1)
        lines.append(b"r%d\t%d\t.\t%s\t%s" % (int(s["record"]), int(s["pos"]) + 1, b"ACGT"[int(s["ref"]).bit_length() - 1:][:1], alts))
    return b"\n".join(lines) + b"\n"


def after_snps(layout, rows):
    """The layout whose islands hold the codes variant_util.apply_snps writes for `rows` (in the layout's coordinates)."""
    import variant_util as vu
    records, changed = vu.apply_snps(layout.twin(), snps_to_twin(layout, rows))
    return layout.with_texts([seq[PAD:-PAD] for _, seq in records]), changed


# (island, offset, length of REF, ALT): REF is read off the island; a deletion, an insertion and a complex allele at the
# text crossing, at the record crossing and in r2, and two ordinary ones.
_INDELS = [
    ("text-crossing", 147, 5, b"{0}"),          # deletion of four bases across text position 2^32
    ("text-crossing", 150, 1, b"{0}ACG"),       # insertion behind the base at 2^32
    ("record-crossing", 149, 1, b"{0}TTGCA"),   # insertion behind the last base below record position 2^32
    ("record-crossing", 148, 4, b"GA"),         # complex
    ("record-crossing", 152, 3, b"{0}"),        # deletion beyond it
    ("r2-start", 2, 3, b"CT"),                  # complex, three bases into r2
    ("r2-end", 320, 2, b"{0}"),                 # deletion nine bases ahead of the text's end
    ("r0-a", 100, 1, b"{0}GG"),
    ("high", 10, 6, b"{0}"),
]


def indels(layout):
    """-> (INDEL_DTYPE array in the layout's coordinates, allele text)"""
    entries = []
    for name, at, ref_len, alt in _INDELS:
        i = layout.island(name)
        ref = i.seq[at:at + ref_len]
        alt = alt.replace(b"{0}", ref[:1])
        if alt == ref or (len(alt) == len(ref)):
            alt = alt[:-1] + b"ACGT"[(b"ACGT".index(alt[-1:]) + 1) % 4:][:1]
        entries.append((i.record, i.start + at, ref, alt))
    return hu.make_indels(entries)


# ---- what the readers are asked --------------------------------------------------------------------------------------------

def _window_queries(pattern, wanted, seed):
    """Queries read off the candidates of `pattern` on big()'s twin: up to `wanted` per class of place, some with a base
    changed, and the all-N query last."""
    import search_util as su
    b = big()
    L = len(pattern)
    rec, pos, strand, t = su.candidates(b.twin(), pattern)
    R, P = b.from_twin(rec, pos)
    tp = b.text_pos(R, P)
    groups = [(tp < T32) & (tp + L > T32), (R == 1) & (P < T32) & (P + L > T32), R == 2, (R == 1) & (P >= T32),
              (tp >= T32) & (P < T32), R == 0, (R == 1) & (tp < T32)]
    rng = np.random.default_rng(seed)
    out = []
    for g in groups:
        for s in (0, 1):
            at = np.flatnonzero(g & (strand == s))
            for k in at[:wanted]:
                q = ["ACGT"[c] for c in t[k]]
                if len(out) % 3 == 1:
                    j = int(rng.integers(0, L))
                    q[j] = "ACGT"[("ACGT".index(q[j]) + 1) % 4]
                out.append("".join(q))
    out = list(dict.fromkeys(out))
    return out + ["N" * L]


NGG = "N" * 21 + "GG"
TTTV = "TTTV" + "N" * 20
SPAN = (0, 20)


@functools.lru_cache(maxsize=None)
def search_cases():
    """[(pattern, queries, max_dist)]: NGG and the 5' pattern at max_dist 0, 2 and L, and the lengths 1 and 32."""
    ngg, tttv, n32 = _window_queries(NGG, 2, 1), _window_queries(TTTV, 1, 2), _window_queries("N" * 32, 1, 3)
    return [(NGG, ngg, 0), (NGG, ngg, 2), (NGG, ngg[:4] + ngg[-1:], 23), (TTTV, tttv, 2), (TTTV, tttv[:3], 24),
            ("N", ["A", "N"], 0), ("N", ["G", "T"], 1), ("N" * 32, n32, 0), ("N" * 32, n32, 2), ("N" * 32, n32[:2], 32)]


@functools.lru_cache(maxsize=None)
def bulge_queries():
    """Queries of the crossing islands: two windows NGG admits at either crossing as they are, the same with a base left out
    (a DNA bulge of the text) and with a base put in (an RNA bulge); behind them two of the planted words and one of them
    with a base left out."""
    b = big()
    out = []
    for name in ("text-crossing", "record-crossing"):
        seq = b.island(name).seq.decode()
        fwd, rev = seq[135:155], revcomp(seq[138:161].encode()).decode()[:20]  # the planted windows c - 15 and c - 12
        out += [fwd + "NNN", fwd[:9] + fwd[10:] + seq[155] + "NNN", rev[:12] + "A" + rev[12:19] + "NNN", rev + "NNN"]
    d, f = words()["D"].decode(), words()["F"].decode()  # r2 and, on the reverse strand, the end of r1
    out += [d[:20] + "NNN", f[:20] + "NNN", d[:6] + d[7:20] + "GNNN"]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def locate_sites(n_absent=8, seed=5):
    """Sites of big()'s text: the planted words, every site whose window covers a crossing, the first and the last site of
    every island, every seventh of the rest, some that do not occur, a few named twice."""
    import locate_util as lu
    import bowtie_util as bwu
    b = big()
    truth = translate_locations(b, lu.brute_force(b.twin()))
    tp = b.text_pos(truth["record"], truth["pos"])
    crossing = ((tp < T32) & (tp + 23 > T32)) | ((truth["record"] == 1) & (truth["pos"] < T32) & (truth["pos"] + 23 > T32))
    edge = np.zeros(len(truth), dtype=bool)
    for i in b.islands:
        inside = np.flatnonzero((truth["record"] == i.record) & (truth["pos"] >= i.start) & (truth["pos"] < i.end))
        if len(inside):
            edge[inside[[0, -1]]] = True
    planted = np.array([bwu.sig(w[:20].decode()) for w in words().values()] +
                       [bwu.sig(revcomp(w)[:20].decode()) for w in words().values()], dtype=np.uint64)
    rng = np.random.default_rng(seed)
    sites = np.concatenate([planted, truth["site"][crossing], truth["site"][edge], truth["site"][::7],
                            rng.integers(0, 1 << 40, size=n_absent, dtype=np.uint64)])
    sites = sites[np.sort(np.unique(sites, return_index=True)[1])]
    sites = np.concatenate([sites, sites[:5]])
    rng.shuffle(sites)
    return sites


@functools.lru_cache(maxsize=None)
def variant_queries():
    """Windows NGG admits on the reference that hold a place of snps(), two per reserved island and strand, as the
    reference spells them; two of the crossing islands' queries; the all-N query."""
    import search_util as su
    b = big()
    rec, pos, strand, t = su.candidates(b.twin(), NGG)
    out = []
    for name in ("snp-r0", "snp-text", "snp-record", "snp-r2"):
        k = b.index(name)
        places = np.array([at + PAD for island, at, _ in _SNPS if island == name])
        over = ((places[None, :] >= pos[:, None]) & (places[None, :] < pos[:, None] + 23)).any(axis=1)
        for s in (0, 1):
            for j in np.flatnonzero((rec == k) & over & (strand == s))[:2]:
                out.append("".join("ACGT"[c] for c in t[j][:20]) + "NNN")
    return list(dict.fromkeys(out + bulge_queries()[:2])) + ["N" * 23]


def haplotype_queries(layout, W):
    """Per indel of indels(layout) the window of W bases that starts five bases ahead of the entry on its ALT haplotype (N
    where the island ends: not compared), every third with a base changed; the all-N query."""
    entries, alleles = indels(layout)
    twin = layout.twin()
    out = []
    for k, d in enumerate(indels_to_twin(layout, entries)):
        seq, p = twin[int(d["record"])][1], int(d["pos"])
        alt = alleles[int(d["alt_at"]):int(d["alt_at"]) + int(d["alt_len"])]
        hap = (seq[:p] + alt + seq[p + int(d["ref_len"]):]).decode()
        q = list(hap[p - 5:p - 5 + W])
        if k % 3 == 2:
            q[W // 2] = "ACGT"[("ACGTN".index(q[W // 2]) + 1) % 4]
        out.append("".join(q))
    return list(dict.fromkeys(out)) + ["N" * W]


@functools.lru_cache(maxsize=None)
def landing_guides():
    """Guides for the landings: the planted words (their sites occur twice), the sites of the windows planted on the
    crossings, the first site of r2 and one that is far from every site."""
    import bowtie_util as bwu
    b = big()
    out = [bwu.sig(w[:20].decode()) for w in words().values()]
    for name in ("text-crossing", "record-crossing"):
        seq = b.island(name).seq
        out += [bwu.sig(seq[135:155].decode()), bwu.sig(revcomp(seq[138:161])[:20].decode())]
    out += [bwu.sig(b.island("r2-start").seq[100:120].decode()), bwu.sig("ACGT" * 5)]
    return np.array(list(dict.fromkeys(out)), dtype=np.uint64)


def annotation():
    """GFF3 for big(): exons over one island on either side of each crossing and over the crossings themselves; e4 has
    coordinates above 2^32 in r1; t3 has no mRNA line."""
    import transcripts_util as tu
    b = big()
    one = lambda name, a, z: (b.island(name).start + a + 1, b.island(name).start + z)  # noqa: E731 (1-based, inclusive)
    return b"".join([
        tu.gff_line("r0", "mRNA", 1, 10, "ID=t0;Parent=g0"), tu.gff_line("r0", "exon", *one("r0-a", 0, 300), "ID=e0;Parent=t0"),
        tu.gff_line("r1", "mRNA", 1, 10, "ID=t1;Parent=g1"), tu.gff_line("r1", "exon", *one("high", 0, 320), "ID=e1;Parent=t1"),
        tu.gff_line("r1", "exon", *one("text-crossing", 100, 160), "ID=e2;Parent=t1"),
        tu.gff_line("r1", "exon", *one("tile-start", 0, 200), "ID=e3;Parent=t1"),
        tu.gff_line("r1", "mRNA", 1, 10, "ID=t2;Parent=g2"), tu.gff_line("r1", "exon", *one("record-crossing", 140, 300), "ID=e4;Parent=t2"),
        tu.gff_line("r1", "exon", *one("r1-end", 0, 300), "ID=e5;Parent=t2"),
        tu.gff_line("r2", "exon", *one("r2-start", 0, 150), "ID=e6;Parent=t3"),
    ])
