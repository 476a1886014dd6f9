"""The island model IS the whole-text model (tests/big_text_util.py), shown without a device: on the big layout shrunk to
N runs of a few thousand bytes every model the device tests use -- locate, the occurrence rows and events, the plain, bulge,
variant and bulge-variant searches, the haplotype search, the landings with and without an annotation, the guide extraction
-- runs once on the whole records and once on the twin followed by the translation, and the two results are the same bytes.
Two gaps, so that the islands meet the tiles of 4096 at other phases.  Then what the big layout is meant to say: 33 position
bits, and for every reader rows beyond 2^32 of every class the text exists for, which a position cut to 32 bits would move."""
import functools

import numpy as np
import pytest

import big_text_util as bt
import batches_util as ba
import bowtie_util as bwu
import bulge_util as bu
import bulge_variant_util as bvu
import genome_text_util as gt
import guides_util as gu
import haplotype_util as hu
import landing_util as ldu
import locate_util as lu
import runlog_model as rm
import search_util as su
import transcripts_util as tu
import variant_util as vu

GAPS = (5000, 4173)
BULGE_CASES = [(2, 3, 3), (0, 1, 2)]            # (max_dist, max_dna, max_rna) on the crossing islands' queries
VARIANT_CASES = [(2, 0), (2, 1), (1, 2)]        # (max_dist, max_variants)
BULGE_VARIANT_CASES = [(1, 2, 1, 0), (1, 1, 1, 1), (2, 1, 2, 2)]  # (max_dist, max_dna, max_rna, max_variants)
HAPLOTYPE_CASES = [(23, 2, 2), (32, 3, 1)]      # (W, max_dist, max_variants)
LANDING_DIST = 2


def BULGE_VARIANT_QUERIES():
    return bt.variant_queries()[0:16:2] + bt.bulge_queries()[:2] + bt.bulge_queries()[4:5] + bt.bulge_queries()[-3:]


def coded(layout):
    """The layout after the SNPs of the reserved islands."""
    out, changed = bt.after_snps(layout, bt.snps(layout))
    assert changed == len(bt.snps(layout))
    return out


def paged(model, sigs):
    starts = gt.ragged_starts(len(sigs))
    events, codes = rm.bowtie_events(model, [bwu.unsig(s) for s in sigs], starts)
    return ba.paged_rows(model, sigs, starts), np.array(events, dtype=np.int32), codes


def occurrence_model(layout, sigs, on_twin):
    """-> rows at page lengths 0 and 7, rows of ragged pages, their events and codes."""
    model = bwu.Model([gt.fasta(layout.twin() if on_twin else layout.whole_records())])
    out = [model.rows(sigs, 0), model.rows(sigs, 7)] + list(paged(model, sigs))
    return [bt.translate_occurrences(layout, x) if on_twin and x.dtype == bwu.DTYPE else x for x in out]


def landing_model(layout, truth, guides, gff, on_twin):
    """truth: locate_util.brute_force of the twin or of the whole records.  -> offsets, rows, profile"""
    offs, recs = gt.model_offtargets(bt.big().twin(), guides, LANDING_DIST)  # the index is built from the reference's sites
    names = [(n, b"") for n in bt.NAMES]
    hits = None
    if gff is not None:
        hits = ldu.location_hits(names, bt.translate_locations(layout, truth) if on_twin else truth, tu.Model(gff))
    offsets, rows, cnt = ldu.join(len(guides), offs, recs, truth, hits)
    prof = ldu.profile(len(guides), recs, cnt, rows)
    return offsets, bt.translate_landings(layout, rows) if on_twin else rows, prof


def every_model(layout, on_twin, gff=None):
    """{reader: [arrays]} for the layout, from its whole records or from its twin with the translation."""
    plain, snp = layout, coded(layout)
    rec = (lambda lay: lay.twin()) if on_twin else (lambda lay: lay.whole_records())
    tr = (lambda lay, f, rows: f(lay, rows)) if on_twin else (lambda lay, f, rows: rows)
    sites = bt.locate_sites()
    out = {}
    for tag, lay in (("", plain), (" after SNPs", snp)):
        truth = lu.brute_force(rec(lay))
        out["locate" + tag] = [tr(lay, bt.translate_locations, truth)]
        out["occurrences" + tag] = occurrence_model(lay, sites, on_twin)
        out["landings" + tag] = list(landing_model(lay, truth, bt.landing_guides(), None, on_twin))
        if gff is not None:
            out["landings annotated" + tag] = list(landing_model(lay, truth, bt.landing_guides(), gff, on_twin))
    out["search"] = []
    for pattern, queries, max_dist in bt.search_cases():
        off, rows, prof = su.brute_force(rec(plain), pattern, list(queries), max_dist)
        out["search"] += [off, tr(plain, bt.translate_search, rows), prof]
    out["bulges"] = []
    for max_dist, D, R in BULGE_CASES:
        off, rows, prof = bu.brute_force(rec(plain), bt.NGG, bt.bulge_queries(), bt.SPAN, max_dist, D, R)
        out["bulges"] += [off, tr(plain, bt.translate_bulges, rows), prof]
    out["variants"] = []
    for max_dist, max_variants in VARIANT_CASES:
        off, rows, prof = vu.brute_force(rec(snp), bt.NGG, bt.variant_queries(), max_dist, max_variants)
        out["variants"] += [off, tr(snp, bt.translate_variants, rows), prof]
    out["bulge variants"] = []
    for max_dist, D, R, max_variants in BULGE_VARIANT_CASES:
        off, rows, prof = bvu.brute_force(rec(snp), bt.NGG, BULGE_VARIANT_QUERIES(), bt.SPAN, max_dist, D, R,
                                          max_variants)
        out["bulge variants"] += [off, tr(snp, bt.translate_bulge_variants, rows), prof]
    out["haplotypes"] = []
    entries, alleles = bt.indels(snp)
    for W, max_dist, max_variants in HAPLOTYPE_CASES:
        queries = bt.haplotype_queries(snp, W)
        if on_twin:
            out["haplotypes"] += list(bt.haplotypes(snp, entries, alleles, "N" * W, queries, max_dist, max_variants))
        else:
            out["haplotypes"] += list(hu.whole_record(rec(snp), entries, alleles, "N" * W, queries, max_dist, max_variants))
    out["guides"] = [bt.guide_rows(plain) if on_twin else gu.brute_force(rec(plain))]
    return out


@pytest.mark.parametrize("gap", GAPS)
def test_the_island_model_is_the_whole_text_model(gap):
    layout = bt.shrunk(gap)
    assert [i.seq for i in layout.islands] == [i.seq for i in bt.big().islands]
    whole, twin = every_model(layout, False, bt.annotation()), every_model(layout, True, bt.annotation())
    assert whole.keys() == twin.keys()
    for reader in whole:
        assert len(whole[reader]) == len(twin[reader])
        for k, (a, b) in enumerate(zip(whole[reader], twin[reader])):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (reader, k)
        assert sum(len(a) for a in whole[reader]) > 0, reader


@pytest.mark.parametrize("line", [1000, 4173, 1 << 20])
def test_the_fasta_buffers_read_back_as_the_records(line):
    """Lines that end inside an island, on its first base and behind the record's last base."""
    layout = bt.shrunk(GAPS[1])
    buffers = [b.tobytes() for b in layout.fasta_buffers(line)]
    assert lu.parse(buffers) == layout.whole_records() and gu.parse(buffers) == layout.whole_records()
    assert lu.parse([b"".join(buffers)]) == layout.whole_records()
    assert all(b.endswith(b"\n") and not b.endswith(b"\n\n") for b in buffers)


def test_the_gaps_move_the_tile_phases():
    phase = lambda layout: [int(layout.text_pos(i.record, i.start)) % bt.TILE for i in layout.islands]  # noqa: E731
    a, b, big = phase(bt.shrunk(GAPS[0])), phase(bt.shrunk(GAPS[1])), phase(bt.big())
    assert sum(x != y for x, y in zip(a, b)) >= len(a) - 3 and sum(x != y for x, y in zip(a, big)) >= len(a) - 3


def test_the_layout_says_what_it_is_meant_to():
    b = bt.big()
    assert b.text_len == bt.T32 + 3 * 65536 + 3 and b.text_len > bt.T32 and b.pos_bits == 33
    assert b.starts == [0, 65537, bt.T32 + 131074]
    name = lambda n: b.island(n)  # noqa: E731
    t = lambda n: int(b.text_pos(name(n).record, name(n).start))  # noqa: E731
    assert t("text-crossing") == bt.T32 - 150 and name("record-crossing").start == bt.T32 - 150
    assert t("tile-start") % bt.TILE == 0 and t("tile-start") > bt.T32
    assert (t("tile-end") + len(name("tile-end").seq)) % bt.TILE == 0 and t("tile-end") > bt.T32
    assert name("low").end < 1 << 31 < name("high").start and t("high") + 320 < bt.T32
    assert name("r1-end").end == b.lengths[1] and name("r2-start").start == 0
    assert t("r2-end") + len(name("r2-end").seq) + 1 == b.text_len  # the last base of the text ('\n' behind it)
    for x, y in zip(b.islands, b.islands[1:]):
        assert x.record != y.record or y.start - x.end >= 64
    assert all(200 <= len(i.seq) <= 400 for i in b.islands)
    # the planted words lie where they are said to, once below and once above 2^32, or twice above
    truth = bt.translate_locations(b, lu.brute_force(b.twin()))
    tp = b.text_pos(truth["record"], truth["pos"])
    for w, word in bt.words().items():
        at = np.flatnonzero(truth["site"] == np.uint64(bwu.sig(word[:20].decode())))
        assert len(at) == 2 and int(tp[at[1]]) >= bt.T32, w
        low = (tp[at] & (bt.T32 - 1))
        if w in "BE":
            assert int(tp[at[0]]) < bt.T32 and low[0] > low[1]  # 32 bits would order them the other way round
    assert len({tuple(truth["strand"][truth["site"] == np.uint64(bwu.sig(word[:20].decode()))].tolist())
                for word in bt.words().values()}) >= 3  # (0, 0), (1, 0), (0, 1)


@functools.lru_cache(maxsize=None)
def expected_big():
    """Every reader's expected rows on the big text, as (record, pos, window width, strand)."""
    b = bt.big()
    m = every_model(b, True, bt.annotation())
    out = {}
    for reader, parts in m.items():
        rows = [p for p in parts if p.dtype.names and "record" in p.dtype.names and len(p)]
        if not rows:
            continue
        rec = np.concatenate([r["record"] for r in rows]).astype(np.int64)
        pos = np.concatenate([r["start" if "start" in r.dtype.names else "pos"] for r in rows]).astype(np.int64)
        strand = np.concatenate([r["strand"] for r in rows])
        width = np.full(len(rec), 23)
        if reader == "search":
            width = np.concatenate([np.full(len(parts[3 * k + 1]), len(c[0])) for k, c in enumerate(bt.search_cases())])
        elif reader.startswith("bulge"):
            width = 23 + np.concatenate([r["bulge"] for r in rows]).astype(np.int64)
        elif reader == "haplotypes":
            width = np.concatenate([np.full(len(parts[3 * k + 1]), c[0]) for k, c in enumerate(HAPLOTYPE_CASES)])
        keep = rec != bt.NONE
        out[reader] = (rec[keep], pos[keep], width[keep], strand[keep])
    return m, out


def test_every_reader_has_rows_of_every_class():
    b = bt.big()
    m, exp = expected_big()
    assert set(exp) == set(m)
    for reader, (rec, pos, width, strand) in exp.items():
        # an occurrence row names the FIRST place of a read, so no read's first place need lie on a crossing
        but = ("covers the text crossing", "covers the record crossing") if reader.startswith("occurrences") else ()
        bt.assert_classes(b, rec, pos, width, strand, but=but)
        r32, p32 = bt.masked_lookup(b, rec, pos)
        assert ((r32 != rec) | (p32 != pos)).any(), reader
    # a bulged window of every length 20 .. 26 starts below and ends above either crossing
    off, rows, _ = m["bulges"][:3]
    tp = b.text_pos(rows["record"], rows["pos"])
    for bulge in range(-3, 4):
        sel = rows["bulge"] == bulge
        w = 23 + bulge
        assert ((tp[sel] < bt.T32) & (tp[sel] + w > bt.T32)).any(), bulge
        assert ((rows["record"][sel] == 1) & (rows["pos"][sel] < bt.T32) & (rows["pos"][sel] + np.uint64(w) > bt.T32)).any(), bulge
    # the variant readers have rows that hold a code in every class of place
    for reader in ("variants", "bulge variants"):
        rows = np.concatenate([p for p in m[reader] if p.dtype.names and len(p)])
        rows = rows[rows["n_var"] > 0]
        bt.assert_classes(b, rows["record"], rows["pos"], 23, rows["strand"],
                          but=("covers the text crossing", "covers the record crossing"))
    # the haplotype rows: every indel has rows, with edits on either side of the window's start
    rows = m["haplotypes"][1]
    assert set(rows["indel"].tolist()) == set(range(len(bt.indels(b)[0])))
    assert (rows["edit_at"] < 0).any() and (rows["edit_at"] > 0).any()
    # the annotated landings: places in an exon on either side of both crossings, in r2, and places outside every exon
    rows = m["landings annotated"][1]
    cut = rows[rows["hits"]["hit"] > 0]
    tp = b.text_pos(cut["record"], cut["pos"])
    assert (tp < bt.T32).any() and ((tp >= bt.T32) & (cut["pos"] < bt.T32)).any() and (cut["pos"] >= bt.T32).any()
    assert (rows["hits"]["hit"] == 0).any() and (rows["hits"]["status"] != 0).any()
    # the guide extraction: a guide seen below and above 2^32 whose first place lies below
    g = m["guides"][0]
    twice = g[g["seen"] > 1]
    assert len(twice) >= 3 and (b.text_pos(twice["record"], twice["start"]) < bt.T32).any()


def test_a_wrong_ref_is_refused_by_the_models():
    b = bt.big()
    bad = bt.snps(b)[[10, 20]]
    bad["ref"][1] = 1 if int(bad["ref"][1]) != 1 else 2
    assert int(bt.big().text_pos(bad["record"][1], bad["pos"][1])) >= bt.T32
    with pytest.raises(vu.Refused) as e:
        bt.after_snps(b, bad)
    assert e.value.index == 1
