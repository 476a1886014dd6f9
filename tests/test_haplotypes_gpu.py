"""GPU: issl_haplotypes_* and bin/isslSearchGenome --indel-vcf against the definition of tests/haplotype_util.py
(whole_record: one indel applied to its whole record, the variant search's brute force, the windows that overlap the
edit), byte for byte: rows, offsets, profile."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import haplotype_util as hu
import search_util as su
import variant_util as vu

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslSearchGenome")
NGG = "N" * 21 + "GG"
TILE = 4096  # kPosPerBlock of the strip search: text positions per workgroup; its planes are words of 32 positions


def random_text(rng, n, codes="ACGT"):
    return "".join(codes[i] for i in rng.integers(0, len(codes), size=n))


def records_of(seqs):
    return [(b"rec%d some text" % k, s.encode()) for k, s in enumerate(seqs)]


def fasta_of(records):
    return b"".join(b">%s\n%s\n" % (name, seq) for name, seq in records)


def drawn_queries(rng, records, indels, alleles, W, count):
    """Windows of the strips, some as the other strand reads them, some with a base changed, and N x W."""
    texts = [t for _, t in hu.strip_texts(records, indels, alleles, W) if len(t) >= W]
    out = ["N" * W]
    while texts and len(out) < count:
        t = texts[int(rng.integers(0, len(texts)))]
        s = int(rng.integers(0, len(t) - W + 1))
        q = "".join(ch if ch in "ACGT" else "ACGT"[int(rng.integers(0, 4))] for ch in t[s:s + W].decode())
        if rng.random() < 0.4:
            q = su.revcomp(q)
        if rng.random() < 0.4:
            i = int(rng.integers(0, W))
            q = q[:i] + "ACGTN"[int(rng.integers(0, 5))] + q[i + 1:]
        out.append(q)
    return out


def check(g, records, entries, pattern, queries, max_dist, max_variants, model=hu.whole_record):
    """One open, one search and one profile on the device equal the model, byte for byte.  -> (offsets, rows)"""
    indels, alleles = entries if isinstance(entries, tuple) else hu.make_indels(entries)
    want_off, want_rows, want_prof = model(records, indels, alleles, pattern, queries, max_dist, max_variants)
    with g.haplotypes(indels, alleles, len(pattern)) as h:
        info = h.info()
        assert info["n_indels"] == len(indels) and info["window"] == len(pattern)
        assert info["text_bytes"] == sum(len(t) + 1 for _, t in hu.strip_texts(records, indels, alleles, len(pattern)))
        off, rows = h.search(pattern, queries, max_dist, max_variants)
        prof = h.search_profile(pattern, queries, max_dist, max_variants)
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == ca.HAPLOTYPE_HIT_DTYPE and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    return off, rows


# ---- every kind of edit ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_record():
    rng = np.random.default_rng(41)
    seq = random_text(rng, 120)
    records = records_of([seq])
    ins40 = random_text(rng, 40)

    def other(ch):
        return "ACGT"[("ACGT".index(ch) + 1) % 4]

    entries = [(0, 10, seq[10:12], seq[10]),                                   # a 1-base deletion behind its anchor
               (0, 25, seq[25:29], seq[25]),                                   # a 3-base deletion
               (0, 40, seq[40], seq[40] + other(seq[41])),                     # a 1-base insertion
               (0, 55, seq[55], seq[55] + "GATTA"[:4] + other(seq[56])),       # a 5-base insertion
               (0, 70, seq[70], seq[70] + ins40[:39] + other(seq[71])),        # 40 bases: longer than any window
               (0, 85, seq[85:87], other(seq[85]) + other(seq[86])),           # AC > GT
               (0, 100, seq[100:103], next(ch for ch in "ACGT" if ch not in (seq[100], seq[102])))]  # ACG > T
    with ca.Genome.open([fasta_of(records)]) as g:
        yield g, records, entries


@pytest.mark.parametrize("W", [1, 2, 23, 32])
def test_every_kind_of_edit(one_record, W):
    g, records, entries = one_record
    rng = np.random.default_rng(W)
    indels, alleles = hu.make_indels(entries)
    assert [(len(r), len(a)) for _, _, r, a in hu.edits(indels, alleles)] == [(1, 0), (3, 0), (0, 1), (0, 5), (0, 40), (2, 2), (3, 1)]
    queries = drawn_queries(rng, records, indels, alleles, W, 24)
    off, rows = check(g, records, entries, "N" * W, queries, min(W, 2), W)
    every = rows[:int(off[1])]  # N x W: every window of every strip, both strands
    assert set(every["strand"].tolist()) == {0, 1} and len(every) == 2 * sum(
        max(0, len(t) - W + 1) for _, t in hu.strip_texts(records, indels, alleles, W))
    if W == 1:
        assert set(every["indel"].tolist()) == {2, 3, 4, 5, 6}  # a deletion has no window of one base
    else:
        assert set(every["indel"].tolist()) == set(range(7)) and int(every["edit_at"].min()) < 0
        assert int((rows["dist"] == 0).sum()) > len(every)
        check(g, records, entries, ("N" * W + "RG")[-W:], queries, 2, 0)
    if W == 23:  # windows wholly inside the 40 bases: no base of the reference in them
        inside = every[(every["indel"] == 4) & (every["edit_at"] <= 0) & (W - every["edit_at"].astype(np.int64) <= 40)]
        assert len(inside) == 2 * (40 - W) + 2 and set(inside["pos"].tolist()) == {hu.edits(indels, alleles)[4][1]}


# ---- edges ----------------------------------------------------------------------------------------------------------------

def test_edges_of_a_record():
    rng = np.random.default_rng(42)
    a, short, tiny = random_text(rng, 57) + "ACG", random_text(rng, 10), random_text(rng, 5)
    records = records_of([a, short, tiny, "ACGTACGT"])
    W = 8
    entries = [(0, 0, a[0], "GT" + a[0]),                      # an insertion ahead of the first base: p = 0, no left flank
               (0, 0, a[0:2], a[1]),                           # a deletion of the first base: p = 0, nothing ahead of the junction
               (0, 57, a[57:60], a[57]),                       # a deletion of the record's last bases: nothing behind it
               (0, 59, a[59], a[59] + "GT"),                   # an insertion behind the last base's anchor
               (1, 5, short[5], short[5] + "ACGTTGCA"),        # a record shorter than W - 1 on both sides
               (2, 2, tiny[2:4], "TG" if tiny[2:4] != "TG" else "CA"),  # a record shorter than W: no window
               (2, 2, tiny[2], tiny[2] + "ACGT"),              # the same record, long enough with 4 bases more
               (3, 0, "ACGTACGT", "T"),                        # a whole record but its last base goes
               (0, 59, a[59], a[59] + "GT"), (0, 59, a[59], a[59] + "GT")]  # the same indel given twice more
    with ca.Genome.open([fasta_of(records)]) as g:
        indels, alleles = hu.make_indels(entries)
        queries = drawn_queries(rng, records, indels, alleles, W, 12)
        off, rows = check(g, records, entries, "N" * W, queries, 2, 0)
        every = rows[:int(off[1])]
        assert set(every["indel"].tolist()) == {0, 3, 4, 6, 8, 9}  # 1, 2, 5, 7: strips shorter than the window
        assert [len(t) for _, t in hu.strip_texts(records, indels, alleles, W)] == [9, 7, 7, 9, 18, 5, 9, 1, 9, 9]
        W = 4
        queries = drawn_queries(rng, records, indels, alleles, W, 12)
        off, rows = check(g, records, entries, "N" * W, queries, 1, 0)
        every = rows[:int(off[1])]
        assert set(every["indel"].tolist()) == {0, 3, 4, 5, 6, 8, 9}  # 1, 2: nothing on one side of the junction; 7: one base is left
        for k in (8, 9):  # an indel given twice gives its rows twice
            for f in ("pos", "site", "mism", "strand", "dist", "edit_at", "record"):
                assert every[f][every["indel"] == k].tolist() == every[f][every["indel"] == 3].tolist()
        # W = 1 with deletions alone: every strip is empty
        dels = [entries[1], entries[2], entries[7]]
        off, rows = check(g, records, dels, "N", ["N", "A"], 0, 0)
        assert off.tolist() == [0, 0, 0] and len(rows) == 0
        with g.haplotypes(*hu.make_indels(dels), 1) as h:
            assert h.info() == {"n_indels": 3, "text_bytes": 3, "window": 1}
        # n == 0, of indels and of queries
        none = (np.zeros(0, dtype=ca.INDEL_DTYPE), b"")
        off, rows = check(g, records, none, "N" * W, queries, 1, 0)
        assert off.tolist() == [0] * (len(queries) + 1) and len(rows) == 0
        with g.haplotypes(*hu.make_indels(entries), W) as h:
            off, rows = h.search("N" * W, [], 1, 0)
            assert off.tolist() == [0] and len(rows) == 0 and h.search_profile("N" * W, [], 1, 0).shape == (0, 2)


# ---- tile and plane-word borders of the strip text -------------------------------------------------------------------------

@pytest.mark.parametrize("end", [TILE - 1, TILE, TILE + 1])
def test_a_strip_ends_at_the_tile_border(end):
    """About 250 strips across bytes 4096 and 8192 of the strip text; the allele lengths put the separator of one strip at
    `end`, so that a strip's last windows, its separator and the next strip's first windows meet the border of a workgroup's
    tile and of a plane word in every way."""
    W = 23
    rng = np.random.default_rng(end)
    seq = random_text(rng, 1400)
    records = records_of([seq])
    entries, at, placed = [], 0, False
    for k in range(250):
        pos = 30 + 5 * k  # closer than a window: never combined
        room = end - at
        if not placed and 50 <= room <= 110:
            ins = room - 2 * (W - 1)  # strip = 22 + ins + 22 bytes, its separator at `end`
            placed = True
        else:
            ins = int(rng.integers(0, 12))
        if ins == 0:
            entries.append((0, pos, seq[pos:pos + 3], seq[pos]))  # a deletion: 22 + 22 bytes
            at += 2 * (W - 1) + 1
        else:
            entries.append((0, pos, seq[pos], seq[pos] + random_text(rng, ins)))  # (however it is trimmed, `ins` bases go in)
            at += 2 * (W - 1) + ins + 1
    indels, alleles = hu.make_indels(entries)
    ends = np.cumsum([len(t) + 1 for _, t in hu.strip_texts(records, indels, alleles, W)]) - 1
    assert end in ends.tolist() and int(ends[-1]) > 2 * TILE + 100
    k = ends.tolist().index(end)
    texts = hu.strip_texts(records, indels, alleles, W)
    queries = ["N" * W, texts[k][1][-W:].decode(), su.revcomp(texts[k + 1][1][:W].decode()), texts[k + 1][1][1:W + 1].decode()]
    k2 = int(np.searchsorted(ends, 2 * TILE))
    queries += [texts[k2][1][-W:].decode(), texts[k2 + 1][1][:W].decode()] + drawn_queries(rng, records, indels, alleles, W, 6)[1:]
    with ca.Genome.open([fasta_of(records)]) as g:
        off, rows = check(g, records, entries, "N" * W, queries, 1, 0)
    assert len(rows[:int(off[1])]) == 2 * int(sum(len(t) - W + 1 for _, t in texts))
    for q in range(1, 6):
        assert int((rows[int(off[q]):int(off[q + 1])]["dist"] == 0).sum()) >= 1


# ---- more than 4096 strips --------------------------------------------------------------------------------------------------

def test_five_thousand_indels_on_one_record():
    """More than 4096 strips -- 5 000 records of the strip text for the finish pass's record lookup -- against strips():
    tests/test_haplotypes_model.py pins that model to the definition."""
    W = 23
    rng = np.random.default_rng(43)
    seq = random_text(rng, 10040)
    records = records_of([seq])
    entries = []
    for k in range(5000):
        pos = 2 * k + int(rng.integers(0, 2))
        if k % 3 == 0:
            entries.append((0, pos, seq[pos:pos + 2 + k % 4], seq[pos]))
        else:
            entries.append((0, pos, seq[pos], seq[pos] + random_text(rng, 1 + k % 5)))
    indels, alleles = hu.make_indels(entries)
    queries = drawn_queries(rng, records, indels, alleles, W, 8)
    with ca.Genome.open([fasta_of(records)]) as g:
        off, rows = check(g, records, (indels, alleles), ("N" * W + "RG")[-W:], queries, 2, 0, model=hu.strips)
    assert len(set(rows["indel"].tolist())) > 4096 and int(rows["indel"].max()) == 4999 and int(off[1]) > 20000


# ---- SNPs and indels together ---------------------------------------------------------------------------------------------

def test_snps_and_indels_together():
    W = 12
    rng = np.random.default_rng(44)
    seq = random_text(rng, 200, "ACT")  # (no G: a SNP to G makes R, K or S, never all four bases)
    ref_records = records_of([seq])

    def snp(pos, alt="G"):
        return (pos, 0, 1 << "ACGT".index(seq[pos]), 1 << "ACGT".index(alt), (0, 0))

    before = np.array([snp(45), snp(50), snp(58), snp(120)], dtype=ca.SNP_DTYPE)
    records, changed = vu.apply_snps(ref_records, before)
    assert changed == 4
    entries = [(0, 52, seq[52:55], seq[52]),                    # codes in both flanks (45, 50; 58)
               (0, 49, seq[49:52], seq[49]),                    # the REF covers the code at 50: a base its set holds
               (0, 120, seq[120], seq[120] + "GG"),             # the anchor is a code
               (0, 150, seq[150], seq[150] + "TG")]             # no code near
    indels, alleles = hu.make_indels(entries)
    with ca.Genome.open([fasta_of(ref_records)]) as g:
        assert g.apply_snps(before) == 4
        flank = hu.strip_texts(records, indels, alleles, W)[0][1]
        assert sum(ch in b"RKS" for ch in flank) == 3
        w = flank[:W].decode()  # a window over two of the codes
        assert sum(ch in "RKS" for ch in w) == 2
        alt_q = "".join("G" if ch in "RKS" else ch for ch in w)          # what the ALT alleles of the SNPs spell
        ref_q = "".join({"R": "A", "K": "T", "S": "C"}.get(ch, ch) for ch in w)  # what the reference spells
        queries = ["N" * W, alt_q, ref_q] + drawn_queries(rng, records, indels, alleles, W, 8)[1:]
        off, rows = check(g, records, entries, "N" * W, queries, 1, W)
        assert int(rows["n_var"].max()) == 3
        for q in (1, 2):  # a code widens the hits: both spellings at distance 0, two variants counted
            mine = rows[int(off[q]):int(off[q + 1])]
            assert ((mine["dist"] == 0) & (mine["n_var"] == 2) & (mine["indel"] == 0)).any()
        off0, rows0 = check(g, records, entries, "N" * W, queries, 1, 0)  # max_variants = 0 drops every window over a code
        assert len(rows0) < len(rows) and int(rows0["n_var"].max()) == 0 and not (rows0["indel"] == 0).any()
        assert (rows0["indel"] == 3).sum() == (rows["indel"] == 3).sum()
        check(g, records, entries, "N" * W, queries, 1, 1)
        # SNPs applied after the open change nothing in the handle's rows
        with g.haplotypes(indels, alleles, W) as h:
            first = h.search("N" * W, queries, 1, W)
            assert g.apply_snps(np.array([snp(56), snp(151), snp(148)], dtype=ca.SNP_DTYPE)) == 3
            again = h.search("N" * W, queries, 1, W)
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes() == rows.tobytes()
        later, _ = vu.apply_snps(records, np.array([snp(56), snp(151), snp(148)], dtype=ca.SNP_DTYPE))
        off2, rows2 = check(g, later, entries, "N" * W, queries, 1, W)  # a handle opened now sees them
        assert rows2.tobytes() != rows.tobytes()


# ---- the point of it all ----------------------------------------------------------------------------------------------------

def test_a_deletion_makes_a_pam_on_either_strand():
    proto = "ACGTACGATCGATGCATGCA"  # no GG and no CC in it, nor in its reverse complement
    rng = np.random.default_rng(45)
    f1, f2, f3 = (random_text(rng, 30, "AT") for _ in range(3))
    seq = f1 + proto + "AGAG" + f2 + "CTCT" + su.revcomp(proto) + f3
    assert "GG" not in seq and "CC" not in seq
    records = records_of([seq])
    mirror = len(f1) + 20 + 4 + len(f2)
    entries = [(0, 51, "GA", "G"),            # ...proto A G|A|G: the A between the two G goes, proto + AGG stands there
               (0, mirror, "CT", "C")]        # C|T|C T + rc(proto): its mirror image, CCT + rc(proto), for strand 1
    query = proto + "NNN"
    with ca.Genome.open([fasta_of(records)]) as g:
        off, rows = g.search_variants(NGG, [query], 4, 23)
        assert off.tolist() == [0, 0] and len(rows) == 0  # the reference has no PAM anywhere
        off, rows = check(g, records, entries, NGG, [query], 0, 0)
    got = [(int(r["indel"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["dist"]), int(r["edit_at"]),
            vu.site_text(r["site"], 23, r["mism"])) for r in rows]
    assert got == [(0, 0, 30, 0, 0, 22, proto + "AGG"), (1, 0, mirror, 1, 0, 1, proto + "AGG")]


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals():
    rng = np.random.default_rng(46)
    seq = random_text(rng, 300)
    records = records_of([seq])

    def other(ch):
        return "ACGT"[("ACGT".index(ch) + 2) % 4]

    good = [(0, 20 * k + 5, seq[20 * k + 5:20 * k + 7], seq[20 * k + 5]) for k in range(10)]
    bad = list(good)
    bad[7] = (0, 145, seq[145] + other(seq[146]), seq[145])        # the second REF base is not the text's
    bad[3] = (0, 65, seq[65:67] + other(seq[67]), other(seq[67]))   # the last REF base, which the trim removes: the untrimmed REF counts
    with ca.Genome.open([fasta_of(records)]) as g:
        with pytest.raises(ca.IsslError) as e:
            g.haplotypes(*hu.make_indels(bad), 23)
        assert e.value.code == -1 and "indel 3:" in e.value.message and "REF" in e.value.message, e.value.message
        with pytest.raises(ca.IsslError) as e:
            g.haplotypes(*hu.make_indels(bad[:3] + good[3:7] + bad[7:]), 23)
        assert "indel 7:" in e.value.message
        for window in (0, 33, -1):
            with pytest.raises(ca.IsslError) as e:
                g.haplotypes(*hu.make_indels(good), window)
            assert e.value.code == -1 and "window" in e.value.message
        for entries, what in (([(1, 5, "AC", "A")], "record"), ([(0, 299, "AC", "A")], "beyond"), ([(0, 5, "AC", "AC")], "nothing"),
                              ([(0, 5, "AC", "aC")], "nothing"), ([(0, 5, "AN", "A")], "ACGT"), ([(0, 5, "AC", "A-")], "ACGT")):
            with pytest.raises(ca.IsslError) as e:
                g.haplotypes(*hu.make_indels(good + entries), 23)
            assert e.value.code == -1 and "indel 10:" in e.value.message and what in e.value.message, e.value.message
        indels, alleles = hu.make_indels(good)
        outside = indels.copy()
        outside["alt_at"][4] = len(alleles)
        with pytest.raises(ca.IsslError) as e:
            g.haplotypes(outside, alleles, 23)
        assert "indel 4:" in e.value.message and "outside" in e.value.message
        with g.haplotypes(indels, alleles, 23) as h:
            queries = ["N" * 23, seq[0:5] + seq[7:25]]
            for pattern in ("N" * 22, "N" * 24, "N"):  # pat.length != window
                with pytest.raises(ca.IsslError) as e:
                    h.search(pattern, ["N" * len(pattern)], 1, 1)
                assert e.value.code == -1 and "window" in e.value.message
                with pytest.raises(ca.IsslError):
                    h.search_profile(pattern, ["N" * len(pattern)], 1, 1)
            for max_variants in (24, -1):  # max_variants > L
                with pytest.raises(ca.IsslError) as e:
                    h.search("N" * 23, queries, 1, max_variants)
                assert "max_variants" in e.value.message
            with pytest.raises(ca.IsslError) as e:
                h.search("N" * 23, queries, 24, 1)
            assert "max_dist" in e.value.message
            # cap < n_total writes nothing and reports the total
            want_off, want_rows, _ = hu.whole_record(records, indels, alleles, "N" * 23, queries, 1, 0)
            total = len(want_rows)
            assert total > 100
            pat, q = ca.search_prepare("N" * 23, queries)
            offs = np.zeros(len(queries) + 1, dtype=np.uint64)
            poison = np.full(total * 48, 0xA5, dtype=np.uint8)
            n = C.c_size_t()
            args = (h._h, C.byref(pat), q.ctypes.data, len(queries), 1, 0, offs.ctypes.data, poison.ctypes.data)
            assert _lib.lib.issl_haplotypes_search(*args, total - 1, C.byref(n)) == 0
            assert n.value == total and (poison == 0xA5).all() and offs.tobytes() == want_off.tobytes()
            assert _lib.lib.issl_haplotypes_search(*args, total, C.byref(n)) == 0 and poison.tobytes() == want_rows.tobytes()


# ---- device forms -----------------------------------------------------------------------------------------------------------

def test_device_forms_give_the_host_forms_bytes(one_record):
    import torch
    g, records, entries = one_record
    W = 23
    indels, alleles = hu.make_indels(entries)
    queries = drawn_queries(np.random.default_rng(47), records, indels, alleles, W, 16)
    pat, q = ca.search_prepare("N" * W, queries)
    with g.haplotypes(indels, alleles, W) as h:
        want_off, want_rows = h.search(pat, q, 2, 2)
        want_prof = h.search_profile(pat, q, 2, 2)
        total = len(want_rows)
        assert total > 200
        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda")
        assert h.search_device(pat, d_q, d_off, None, 2, 2) == total  # the counting call
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * 48,), 0xA5, dtype=torch.uint8, device="cuda")
        assert h.search_device(pat, d_q, d_off, d_hits[:(total - 1) * 48], 2, 2) == total
        assert bool((d_hits == 0xA5).all())
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert h.search_device("N" * W, d_q, d_off, d_hits, 2, 2, stream=stream.cuda_stream) == total
        assert d_hits.cpu().numpy().view(ca.HAPLOTYPE_HIT_DTYPE).tobytes() == want_rows.tobytes()
        d_counts = torch.full((len(queries) * 3,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        h.search_profile_device(pat, d_q, d_counts, 2, 2, stream=stream.cuda_stream)
        assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes()
        assert h.search_device(pat, d_q[:0], d_off[:1], None, 2, 2) == 0 and int(d_off[0]) == 0  # n == 0
        with pytest.raises(ca.IsslError):
            h.search_device("N" * 22, d_q, d_off, None, 2, 2)


# ---- the executable and the VCF entry point -----------------------------------------------------------------------------------

def test_cli_and_open_vcf_print_the_model(tmp_path):
    rng = np.random.default_rng(48)
    seqs = [random_text(rng, 400), random_text(rng, 150)]
    ref_records = records_of(seqs)
    snp_lines, snps = [], []
    for r, pos in ((0, 60), (0, 131), (1, 40)):
        alt = "ACGT"[("ACGT".index(seqs[r][pos]) + 1) % 4]
        snp_lines.append(b"rec%d\t%d\t.\t%s\t%s" % (r, pos + 1, seqs[r][pos].encode(), alt.encode()))
        snps.append((pos, r, 1 << "ACGT".index(seqs[r][pos]), 1 << "ACGT".index(alt), (0, 0)))
    records, _ = vu.apply_snps(ref_records, np.array(snps, dtype=ca.SNP_DTYPE))
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for k in range(12):
        r, pos = (0, 50 + 30 * k) if k < 9 else (1, 30 + 30 * (k - 9))
        s = seqs[r]
        last = "ACGT"[("ACGT".index(s[pos + 1]) + 1) % 4]
        alts = [s[pos], s[pos] + "ACG"[:k % 3] + last, "<DEL>", last.lower() if k % 2 else "*"]  # a deletion, an insertion, two skipped
        lines.append(b"rec%d\t%d\t.\t%s\t%s\t50\tPASS" % (r, pos + 1, s[pos:pos + 3].encode(), ",".join(alts).encode()))
    lines += [b"chrUn\t5\t.\tAC\tA", b"rec1\t149\t.\tACG\tA", b"rec1\t9\t.\tA\tC"]
    vcf_text = b"\r\n".join(lines[:6]) + b"\r\n" + b"\n".join(lines[6:])
    indels, alleles, counts = hu.vcf_indels(vcf_text, ref_records)
    assert counts == dict(lines=15, indels=29, alleles_skipped=20, no_allele=1, unknown_chrom=1, beyond_record=1, too_long=0)
    texts = hu.strip_texts(records, indels, alleles, 23)
    queries = drawn_queries(rng, records, indels, alleles, 23, 14) + [texts[0][1][:21].decode().lower() + "nn"]
    fasta, snp_vcf, vcf, qfile = (tmp_path / n for n in ("genome.fa", "snps.vcf", "indels.vcf", "queries.txt"))
    fasta.write_bytes(fasta_of(ref_records))
    snp_vcf.write_bytes(b"\n".join(snp_lines) + b"\n")
    vcf.write_bytes(vcf_text)
    qfile.write_text("\r\n".join(queries[:5]) + "\r\n" + "\n".join(queries[5:]) + "\n\n")
    counts_line = (b"indel-vcf: lines 15 indels 29 alleles_skipped 20 no_allele 1 unknown_chrom 1 beyond_record 1 too_long 0\n")
    for mv in (1, 23):
        want_off, want_rows, want_prof = hu.whole_record(records, indels, alleles, NGG, queries, 3, mv)
        assert len(want_rows) > 50 and int(want_rows["n_var"].max()) == 1
        options = ["--vcf", str(snp_vcf), "--indel-vcf", str(vcf)] + (["--variants", str(mv)] if mv != 23 else [])
        r = subprocess.run([EXE] + options + [NGG, str(qfile), "3", str(fasta)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == hu.format_rows(records, queries, want_rows, indels, alleles)
        assert r.stderr.count(b"\n") == 2 and r.stderr.startswith(b"vcf: lines 3 snps 3 ") and r.stderr.endswith(counts_line)
        r = subprocess.run([EXE, "--profile"] + options + [NGG.lower(), str(qfile), "3", str(fasta)], capture_output=True)
        assert r.returncode == 0 and r.stdout == vu.format_profile(queries, want_prof), r.stderr
    # without --vcf the flanks are the reference's, and N = L is implied
    want_off, want_rows, _ = hu.whole_record(ref_records, indels, alleles, NGG, queries, 3, 23)
    r = subprocess.run([EXE, "--indel-vcf", str(vcf), NGG, str(qfile), "3", str(fasta)], capture_output=True)
    assert r.returncode == 0 and r.stderr == counts_line and r.stdout == hu.format_rows(ref_records, queries, want_rows, indels, alleles)
    line = r.stdout.split(b"\n")[0].split(b"\t")
    assert len(line) == 8 and b":" in line[6] and b">" in line[6]
    r = subprocess.run([EXE, "--indel-vcf", str(vcf), "--guide", "0:20", NGG, str(qfile), "3", str(fasta)], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    # issl_haplotypes_open_vcf: the same handle from the text, and from a path
    with ca.Genome.open([fasta_of(ref_records)]) as g:
        for source in (vcf_text, vcf):
            h, got_counts = g.haplotypes_vcf(source, 23)
            with h:
                assert got_counts == counts and h.info()["n_indels"] == 29
                off, rows = h.search(NGG, queries, 3, 23)
                assert off.tobytes() == want_off.tobytes() and rows.tobytes() == want_rows.tobytes()
        with pytest.raises(ca.IsslError) as e:
            g.haplotypes_vcf(vcf_text + b"\nrec0\t7\n", 23)
        assert "line 18:" in e.value.message
        with pytest.raises(ca.IsslError) as e:
            g.haplotypes_vcf(b"rec0\t7\t.\t%s\tA\n" % (("ACGT"[("ACGT".index(seqs[0][6]) + 1) % 4]) + seqs[0][7]).encode(), 23)
        assert "indel 0:" in e.value.message
