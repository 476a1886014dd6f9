"""Every reader of a genome handle against its model on ANY text (tests/test_genome_after_snps.py): issl_genome_apply_snps and
issl_genome_apply_vcf write IUPAC codes into the text that locate, the occurrence calls, the searches and the landings read.
The models answer for arbitrary text already -- locate_util.brute_force, bowtie_util.Model, search_util / bulge_util /
variant_util.brute_force, landing_util.join -- so a helper here takes (records with codes, genome handle), asks one reader,
compares it with its model on those records and returns the reader's bytes, which two handles that hold the same text must
agree on whatever way the codes got there.  No device is needed to import this file or to build a Truth."""
import numpy as np

import crackling_amd as ca
import batches_util as bt
import bowtie_util as bwu
import bulge_util as bu
import landing_util as ldu
import locate_util as lu
import search_util as su
import variant_util as vu

NGG = "N" * 21 + "GG"
SPAN = (0, 20)


def fasta(records):
    return b"".join(b">%s\n%s\n" % (name, seq) for name, seq in records)


class Truth:
    """The models of one text, each computed once."""
    _of = {}

    def __init__(self, records):
        self.records = [(bytes(n), bytes(s)) for n, s in records]
        self.blob = fasta(self.records)
        assert lu.parse([self.blob]) == self.records  # the coded FASTA reads back as these records
        self.locate = lu.brute_force(self.records)
        self._bowtie, self._rows = None, {}

    @classmethod
    def of(cls, records):
        key = tuple((bytes(n), bytes(s)) for n, s in records)
        if key not in cls._of:
            cls._of[key] = cls(records)
        return cls._of[key]

    @property
    def bowtie(self):
        if self._bowtie is None:
            self._bowtie = bwu.Model([self.blob])
        return self._bowtie

    def _cached(self, key, make):
        if key not in self._rows:
            self._rows[key] = make()
        return self._rows[key]

    def search(self, pattern, queries, max_dist):
        return self._cached(("search", pattern, tuple(queries), max_dist), lambda: su.brute_force(self.records, pattern, list(queries), max_dist))

    def bulges(self, pattern, queries, span, max_dist, D, R):
        return self._cached(("bulges", pattern, tuple(queries), span, max_dist, D, R),
                            lambda: bu.brute_force(self.records, pattern, list(queries), span, max_dist, D, R))

    def variants(self, pattern, queries, max_dist, max_variants):
        return self._cached(("variants", pattern, tuple(queries), max_dist, max_variants),
                            lambda: vu.brute_force(self.records, pattern, list(queries), max_dist, max_variants))


def ragged_starts(n):
    """Page boundaries of lengths 1, 0, 7, 13, 64, 3, 1, ... up to n."""
    starts, k = [0], 0
    while starts[-1] < n:
        starts.append(min(n, starts[-1] + (1, 0, 7, 13, 64, 3)[k % 6]))
        k += 1
    return np.array(starts, dtype=np.uint64)


# ---- one reader against its model; -> the reader's bytes ----------------------------------------------------------------

def check_locate(records, g, sites):
    t = Truth.of(records)
    sites = np.ascontiguousarray(sites, dtype=np.uint64)
    offsets, locs = g.locate(sites)
    lu.check_locate(g.records, offsets, locs, sites, t.locate)
    return offsets.tobytes() + locs.tobytes()


def check_occurrences(records, g, sigs):
    t = Truth.of(records)
    sigs = np.ascontiguousarray(sigs, dtype=np.uint64)
    plain = g.occurrences(sigs)
    bwu.same_rows(plain, t.bowtie.rows(sigs))
    out = plain.tobytes()
    for page_length in (0, 7):
        got = g.occurrences(sigs, page_length)
        bwu.same_rows(got, t.bowtie.rows(sigs, page_length))
        out += got.tobytes()
    starts = ragged_starts(len(sigs))
    got = g.occurrences(sigs, page_starts=starts)
    bwu.same_rows(got, bt.paged_rows(t.bowtie, sigs, starts))
    return out + got.tobytes()


def _same_rows(got, want, dtype):
    off, rows, prof = got
    want_off, want_rows, want_prof = want
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == dtype and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    return off.tobytes() + rows.tobytes() + prof.tobytes()


def check_search(records, g, queries, max_dist=2, pattern=NGG):
    want = Truth.of(records).search(pattern, queries, max_dist)
    return _same_rows(g.search(pattern, queries, max_dist) + (g.search_profile(pattern, queries, max_dist),), want, ca.SEARCH_HIT_DTYPE)


def check_bulges(records, g, queries, max_dist=2, pattern=NGG, span=SPAN, D=1, R=1):
    want = Truth.of(records).bulges(pattern, queries, span, max_dist, D, R)
    got = g.search_bulges(pattern, queries, span, max_dist, D, R) + (g.search_bulges_profile(pattern, queries, span, max_dist, D, R),)
    return _same_rows(got, want, ca.BULGE_HIT_DTYPE)


def check_variants(records, g, queries, max_dist=2, max_variants=2, pattern=NGG):
    want = Truth.of(records).variants(pattern, queries, max_dist, max_variants)
    got = g.search_variants(pattern, queries, max_dist, max_variants) + (g.search_variants_profile(pattern, queries, max_dist, max_variants),)
    return _same_rows(got, want, ca.VARIANT_HIT_DTYPE)


def landing_model(records, guides, offs, recs):
    """landing_util.join and .profile fed with the truth of `records`; offs, recs: the off-target records of the guides.
    -> (offsets, rows, profile, landings per off-target record)"""
    offsets, rows, cnt = ldu.join(len(guides), offs, recs, Truth.of(records).locate, None)
    return offsets, rows, ldu.profile(len(guides), recs, cnt, rows), cnt


def check_landings(records, g, ix, guides, max_dist=2):
    """ix: an index of the REFERENCE text; its off-targets land where the text of `records` still holds them."""
    guides = np.ascontiguousarray(guides, dtype=np.uint64)
    offs, recs = ix.offtargets(guides, max_dist=max_dist)
    want_off, want, want_prof, _ = landing_model(records, guides, offs, recs)
    offsets, rows = ix.landings(guides, g, None, max_dist=max_dist)
    assert offsets.dtype == np.uint64 and rows.dtype == ca.LANDING_DTYPE
    assert offsets.tobytes() == want_off.tobytes() and len(rows) == len(want) and rows.tobytes() == want.tobytes()
    prof = ix.landing_profile(guides, g, None, max_dist=max_dist)
    assert prof.tobytes() == want_prof.tobytes()
    return offsets.tobytes() + rows.tobytes() + prof.tobytes()


def model_offtargets(ref_records, guides, max_dist):
    """What an index of ref_records reports for the guides, as far as the join needs it: per guide the distinct sites of the
    text within max_dist substitutions, with their number of occurrences (in site order; IsslIndex.offtargets has its own
    order and more fields).  -> (offsets, records in OFFTARGET_DTYPE).  No device needed."""
    sites, occ = np.unique(Truth.of(ref_records).locate["site"], return_counts=True)
    low = np.uint64(0x5555555555)
    parts, offs = [], [0]
    for k, guide in enumerate(np.asarray(guides, dtype=np.uint64)):
        x = sites ^ guide
        x = (x | (x >> np.uint64(1))) & low
        dist = np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)
        near = np.flatnonzero(dist <= max_dist)
        part = np.zeros(len(near), dtype=ca.OFFTARGET_DTYPE)
        part["site"], part["guide"], part["dist"], part["occ"] = sites[near], k, dist[near], occ[near]
        parts.append(part)
        offs.append(offs[-1] + len(near))
    return np.array(offs, dtype=np.uint64), np.concatenate(parts) if parts else np.zeros(0, dtype=ca.OFFTARGET_DTYPE)


# ---- what is asked -----------------------------------------------------------------------------------------------------

def sites_of(*record_lists, extra=0, seed=1):
    """The distinct sites of the texts, some random 20-mers behind them, a tenth of all named a second time."""
    rng = np.random.default_rng(seed)
    sites = np.unique(np.concatenate([Truth.of(r).locate["site"] for r in record_lists]))
    sites = np.concatenate([sites, rng.integers(0, 1 << 40, size=extra, dtype=np.uint64)])
    sites = np.concatenate([sites, sites[rng.random(len(sites)) < 0.1]])
    rng.shuffle(sites)
    return sites


def queries_of(ref_records, rng, n_sites=6):
    """Queries that the plain and the bulge search answer on the reference text: windows NGG admits there as they are, one
    with a base changed, one with a base left out of a window of 21 (a DNA bulge) and one with a base put into a window of 19
    (an RNA bulge)."""
    text = ref_records[0][1].decode()
    at = [p for p in range(1, len(text) - 23) if text[p + 21:p + 23] == "GG"]
    out = []
    for k, p in enumerate(rng.choice(at, size=n_sites, replace=False)):
        p = int(p)
        q = text[p:p + 20]
        if k % 3 == 1:
            q = q[:7] + "ACGT"[("ACGT".index(q[7]) + 1) % 4] + q[8:]
        out.append(q + "NNN")
    a, b = (int(p) for p in rng.choice(at, size=2, replace=False))
    out.append(text[a - 1:a + 8] + text[a + 9:a + 20] + "NNN")
    out.append(text[b + 1:b + 10] + "ACGT"[int(rng.integers(0, 4))] + text[b + 10:b + 20] + "NNN")
    return out


# ---- a text with repeats -----------------------------------------------------------------------------------------------

def repeat_case(seed=41):
    """6 000 bases in two records with six copies of a 240-base element (two of them reverse-complemented), and SNPs in
    three of the copies and at one base in 40 of the rest: a site of the element occurs four times in the reference (twice
    when it is read off a reversed copy) and, once the SNPs are applied, in some of its places only.  -> (ref_records, snps, records)"""
    rng = np.random.default_rng(seed)
    text = list("".join("ACGT"[c] for c in rng.integers(0, 4, size=6000)))
    element = "".join("ACGT"[c] for c in rng.integers(0, 4, size=240))
    starts = [300, 1100, 2200, 3400, 4300, 5200]
    for k, s in enumerate(starts):
        text[s:s + 240] = element if k % 3 else su.revcomp(element)
    text = "".join(text)
    inside = np.zeros(6000, dtype=bool)
    for s in starts:
        inside[s:s + 240] = True
    places = np.flatnonzero(~inside & (rng.random(6000) < 1.0 / 40)).tolist()
    for s in starts[:3]:
        places += list(range(s + 5 + int(rng.integers(0, 20)), s + 240, 37))
    places = np.array(sorted(places))
    snps = np.zeros(len(places), dtype=ca.SNP_DTYPE)
    snps["pos"], snps["record"] = places % 3000, places // 3000
    for k, p in enumerate(places):
        r = "ACGT".index(text[p])
        snps["ref"][k] = 1 << r
        snps["alt"][k] = 1 << ((r + 1 + int(rng.integers(0, 3))) % 4)
    ref_records = [(b"rep0 some text", text[:3000].encode()), (b"rep1", text[3000:].encode())]
    records, changed = vu.apply_snps(ref_records, snps)
    assert changed == len(snps)
    return ref_records, snps, records
