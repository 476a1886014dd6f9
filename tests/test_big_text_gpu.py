"""Every reader of a resident genome on a text of 2^32 + 196 611 positions (pos_bits = 33): locate, the occurrence calls, the
plain, bulge, variant and bulge-variant searches with their profiles, apply_snps / apply_vcf, the haplotype strips, the
landings with and without an annotation and the two extraction calls, host and device forms, each against its model on the
islands of tests/big_text_util.py translated to the big text -- bytes, no tolerance.  tests/test_big_text_model.py shows
without a device that the island model is the whole-text model and that the expected rows hold every class of place the text
exists for; every test here asserts those classes again on the rows it GOT, so none can pass on a smaller text.

One handle for the module.  The text changes once (the SNP test, on islands reserved for it); the handle's owner keeps the
layout the text stands for, and every test takes its model from that, so no test depends on the order.

Measured on one MI355X machine (16 CPUs), nothing of it asserted:
    the three FASTA buffers (fill with N, headers, line ends, islands, one copy to bytes)     1.3 s
    Genome.open (the host's FASTA pass on 16 threads, its join, 0.4 s of upload)               4.4 s   7.3 s for the fixture
    peak host RSS 13.0 GiB after the open (buffers 4 GiB, the pass's pieces and the joined text 8 GiB), 14.2 GiB at the
    module's end (the extraction calls); free HBM 287.2 GiB before the open, 283.2 GiB after it (the text is 4.0 GiB), and
    283.1 GiB at the least behind any test (sampled when a test returns: the calls free their scratch themselves)
    test_locate 1.8 - 4.6 s (the first kernels of the process load in it), test_snps_and_the_variant_searches 3.3 s,
    test_guide_extraction 3.2 s and test_site_extraction 5.3 s (a FASTA pass of their own each), test_landings 1.3 s,
    test_search_bulges 0.7 and 0.3 s, test_occurrences 0.4 s, test_search 0.05 - 0.2 s a case, test_haplotypes 0.02 s;
    the module 29 s.  With r1 on ONE line the open takes 10.7 s and the site extraction 10.7 s: the pass hands whole lines
    to its threads, and one thread manages 0.4 GB/s -- which is why the buffers hold lines of 2^20 bases.  DESIGN section 5
    has 3.1 Gbp of wrapped FASTA at about 3 s for the same pass."""
import resource
import time

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd._lib import check
import big_text_util as bt
import batches_util as ba
import bowtie_util as bwu
import bulge_util as bu
import bulge_variant_util as bvu
import genome_text_util as gt
import landing_util as ldu
import locate_util as lu
import runlog_model as rm
import search_util as su
import transcripts_util as tu
import variant_util as vu
from test_big_text_model import (BULGE_CASES, BULGE_VARIANT_CASES, BULGE_VARIANT_QUERIES, HAPLOTYPE_CASES, LANDING_DIST,
                                 VARIANT_CASES)
from test_extract import oracle_extract

pytestmark = pytest.mark.gpu
T32 = bt.T32
CROSSINGS = ("covers the text crossing", "covers the record crossing")


def rss_gib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / (1 << 20)


class Big:
    """The big text on the device and the layout it stands for."""

    def __init__(self):
        import torch
        self.layout = bt.big()
        t = [time.perf_counter()]
        buffers = self.layout.fasta_buffers()
        self.blobs = [b.tobytes() for b in buffers]  # what Genome.open and the extraction calls take without a further copy
        del buffers
        t.append(time.perf_counter())
        free0 = torch.cuda.mem_get_info()[0]
        self.g = ca.Genome.open(self.blobs)
        t.append(time.perf_counter())
        self.figures = {"blob_s": t[1] - t[0], "open_s": t[2] - t[1], "rss_gib": rss_gib(), "hbm_free_before_gib": free0 / 2**30,
                        "hbm_free_after_gib": torch.cuda.mem_get_info()[0] / 2**30}
        print("\n[big text] " + " ".join("%s=%.2f" % kv for kv in self.figures.items()), flush=True)

    @property
    def twin(self):
        return self.layout.twin()

    def truth(self):
        return bt.translate_locations(self.layout, lu.brute_force(self.twin))


@pytest.fixture(scope="module")
def big():
    import torch
    b = Big()
    assert b.g.n_bases == sum(bt.LENGTHS) and b.g.records == list(zip(bt.NAMES, bt.LENGTHS))
    assert b.layout.text_len > T32 and b.layout.pos_bits == 33
    yield b
    print("\n[big text] at the end: rss_gib=%.2f hbm_free_low_gib=%.2f" % (rss_gib(), b.figures["hbm_free_low_gib"]), flush=True)
    b.g.close()


@pytest.fixture(autouse=True)
def hbm_low_water(big):
    """Free HBM as it stands behind every test (the calls free their scratch before they return: a sample, not a peak)."""
    import torch
    yield
    big.figures["hbm_free_low_gib"] = min(big.figures.get("hbm_free_low_gib", 1e9), torch.cuda.mem_get_info()[0] / 2**30)


def classes(big, rows, width=23, but=(), pos="pos"):
    """The rows a reader RETURNED hold every class of place (tests/test_big_text_model.py)."""
    keep = rows["record"] != bt.NONE
    return bt.assert_classes(big.layout, rows["record"][keep], rows[pos][keep], width if np.isscalar(width) else width[keep],
                             rows["strand"][keep], but=but)


def same(got, want, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1))[0])
        bad //= got.dtype.itemsize
        raise AssertionError(f"{what} row {bad}: got {got[bad]}, want {want[bad]}")


def on_stream():
    import torch
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    return stream


# ---- 1. locate ---------------------------------------------------------------------------------------------------------------

def expected_locations(truth, sites):
    by_site = lu.expected_by_site(truth)
    offsets, parts = [0], []
    for s in sites:
        rows = by_site.get(int(s))
        n = 0 if rows is None else len(rows)
        offsets.append(offsets[-1] + n)
        if n:
            part = np.zeros(n, dtype=ca.LOCATION_DTYPE)
            part["pos"], part["record"], part["strand"] = rows["pos"], rows["record"], rows["strand"]
            parts.append(part)
    return np.array(offsets, dtype=np.uint64), np.concatenate(parts)


def check_locate(big):
    import torch
    sites, truth = bt.locate_sites(), big.truth()
    want_off, want = expected_locations(truth, sites)
    offsets, locs = big.g.locate(sites)
    classes(big, locs)
    lu.check_locate(big.g.records, offsets, locs, sites, truth)
    assert offsets.tobytes() == want_off.tobytes()
    same(locs, want, "locate")
    assert (np.diff(want_off.astype(np.int64)) == 0).any() and (np.diff(want_off.astype(np.int64)) == 2).any()
    stream = on_stream()
    d_sites = torch.from_numpy(sites.view(np.int64)).cuda()
    d_offs = torch.zeros(len(sites) + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = big.g.locate_device(d_sites, d_offs, None, stream=stream.cuda_stream)
    assert total == len(want)
    d_locs = torch.full((16 * total,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert big.g.locate_device(d_sites, d_offs, d_locs, stream=stream.cuda_stream) == total
    assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
    same(d_locs.cpu().numpy().view(ca.LOCATION_DTYPE), want, "locate_device")
    return offsets.tobytes() + locs.tobytes()


def test_locate(big):
    check_locate(big)
    # the planted words: both places, in text order, whichever side of 2^32 and whichever strand
    for name, word in bt.words().items():
        offsets, locs = big.g.locate(np.array([bwu.sig(word[:20].decode())], dtype=np.uint64))
        assert offsets.tolist() == [0, 2], name
        tp = big.layout.text_pos(locs["record"], locs["pos"])
        assert tp[0] < tp[1] and tp[1] >= T32


# ---- 2. occurrences ----------------------------------------------------------------------------------------------------------

def check_occurrences(big):
    import torch
    sites = bt.locate_sites()
    model = bwu.Model([gt.fasta(big.twin)])
    tr = lambda rows: bt.translate_occurrences(big.layout, rows)  # noqa: E731
    out = b""
    for page_length in (0, 7):
        got, want = big.g.occurrences(sites, page_length), tr(model.rows(sites, page_length))
        bwu.same_rows(got, want)
        same(got, want, "occurrences")
        classes(big, got, but=CROSSINGS)
        out += got.tobytes()
    starts = gt.ragged_starts(len(sites))
    want = tr(ba.paged_rows(model, sites, starts))
    got = big.g.occurrences(sites, page_starts=starts)
    same(got, want, "occurrences, page_starts")
    events, codes = rm.bowtie_events(model, [bwu.unsig(s) for s in sites], starts)
    stream = on_stream()
    d_sigs = torch.from_numpy(sites.view(np.int64)).cuda()
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    d_rows = torch.full((len(sites), 32), 0xAB, dtype=torch.uint8, device="cuda")
    d_events = torch.full((len(starts) - 1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    big.g.occurrences_device(d_sigs, d_rows, stream=stream.cuda_stream, page_starts=d_starts, page_events=d_events)
    torch.cuda.synchronize()
    same(d_rows.cpu().numpy().view(bwu.DTYPE).reshape(-1), want, "occurrences_device, page_starts")
    assert d_events.cpu().numpy().tolist() == events and want["code"].tolist() == codes.tolist()
    big.g.occurrences_device(d_sigs, d_rows, 7, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    same(d_rows.cpu().numpy().view(bwu.DTYPE).reshape(-1), tr(model.rows(sites, 7)), "occurrences_device")
    return out + got.tobytes()


def test_occurrences(big):
    check_occurrences(big)
    # the planted words, each asked alone: the first place of read 0 is the smaller TEXT position, on its strand
    first = {"B": ("high", 40, 0), "C": ("r0-a", 50, 1), "D": ("tile-end", 30, 1), "E": ("low", 200, 0), "F": ("text-crossing", 250, 0)}
    sigs = np.array([bwu.sig(bt.words()[w][:20].decode()) for w in first], dtype=np.uint64)
    rows = big.g.occurrences(sigs)
    for row, (w, (island, at, strand)) in zip(rows, first.items()):
        i = big.layout.island(island)
        assert (int(row["record"]), int(row["pos"]), int(row["strand"])) == (i.record, i.start + at, strand), w
        assert int(row["n_perfect"]) == 2 and int(row["aligned"]) == 1 and int(row["repeated"]) == 1, w
    d = rows[list(first).index("D")]
    assert int(big.layout.text_pos(d["record"], d["pos"])) >= T32  # a read that occurs beyond 2^32 only


# ---- 3. search ---------------------------------------------------------------------------------------------------------------

def host_rows(fn, fn_profile, args, want, dtype, what):
    want_off, want_rows, want_prof = want
    off, rows = fn(*args)
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes(), what
    assert rows.dtype == dtype
    same(rows, want_rows, what)
    prof = fn_profile(*args)
    assert prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes(), what
    return rows


def device_rows(fn, fn_profile, pattern, queries, rest, want, dtype, what, small_first=False):
    """The _device forms on a stream of their own: the counting call, (a capacity one row short, which writes nothing,) the
    exact capacity, the profile."""
    import torch
    want_off, want_rows, want_prof = want
    pat, q = ca.search_prepare(pattern, list(queries))
    d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_off = torch.full((len(q) + 1,), -1, dtype=torch.int64, device="cuda")
    size = dtype.itemsize
    d_hits = torch.full((len(want_rows) * size,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = on_stream()
    assert fn(pat, d_q, d_off, None, *rest, stream=stream.cuda_stream) == len(want_rows), what
    if small_first and len(want_rows):
        assert fn(pat, d_q, d_off, d_hits[:(len(want_rows) - 1) * size], *rest, stream=stream.cuda_stream) == len(want_rows)
        torch.cuda.synchronize()
        assert bool((d_hits == 0xA5).all()), what
    assert fn(pat, d_q, d_off, d_hits, *rest, stream=stream.cuda_stream) == len(want_rows), what
    torch.cuda.synchronize()
    assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes(), what
    same(d_hits.cpu().numpy().view(dtype), want_rows, what + " (device)")
    d_counts = torch.full((want_prof.size,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn_profile(pat, d_q, d_counts, *rest, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes(), what


def translated(layout, model):
    off, rows, prof = model
    return off, layout.translate(rows), prof


@pytest.mark.parametrize("case", range(len(bt.search_cases())))
def test_search(big, case):
    pattern, queries, max_dist = bt.search_cases()[case]
    queries = list(queries)
    want = translated(big.layout, su.brute_force(big.twin, pattern, queries, max_dist))
    what = "search %s max_dist %d" % (pattern, max_dist)
    rows = host_rows(big.g.search, big.g.search_profile, (pattern, queries, max_dist), want, ca.SEARCH_HIT_DTYPE, what)
    classes(big, rows, len(pattern), but=CROSSINGS if len(pattern) == 1 else ())  # (no window of one base covers two)
    device_rows(big.g.search_device, big.g.search_profile_device, pattern, queries, (max_dist,), want, ca.SEARCH_HIT_DTYPE, what,
                small_first=case == 1)
    if case == 1:  # the capacity rule of the host entry point: too small first (nothing written, the total reported), then exact
        import ctypes as C
        pat, q = ca.search_prepare(pattern, queries)
        offsets, n = np.zeros(len(q) + 1, dtype=np.uint64), C.c_size_t()
        hits = np.full(len(rows), 0xA5, dtype=np.uint8).repeat(32).view(ca.SEARCH_HIT_DTYPE)
        args = (big.g._h, C.byref(pat), q.ctypes.data, len(q), max_dist, offsets.ctypes.data, hits.ctypes.data)
        check(ca.lib.issl_genome_search(*args, len(rows) - 1, C.byref(n)))
        assert n.value == len(rows) and bool((hits.view(np.uint8) == 0xA5).all())
        check(ca.lib.issl_genome_search(*args, len(rows), C.byref(n)))
        same(hits, want[1], what + " (cap)")


# ---- 4. bulges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(BULGE_CASES)))
def test_search_bulges(big, case):
    max_dist, D, R = BULGE_CASES[case]
    queries = bt.bulge_queries()
    want = translated(big.layout, bu.brute_force(big.twin, bt.NGG, queries, bt.SPAN, max_dist, D, R))
    what = "bulges max_dist %d dna %d rna %d" % (max_dist, D, R)
    rows = host_rows(big.g.search_bulges, big.g.search_bulges_profile, (bt.NGG, queries, bt.SPAN, max_dist, D, R), want,
                     ca.BULGE_HIT_DTYPE, what)
    classes(big, rows, 23 + rows["bulge"].astype(np.int64))
    tp = big.layout.text_pos(rows["record"], rows["pos"])
    for bulge in range(-R, D + 1) if case == 0 else ():  # a window of every length starts below and ends above either crossing
        sel, w = rows["bulge"] == bulge, 23 + bulge
        assert ((tp[sel] < T32) & (tp[sel] + w > T32)).any(), bulge
        assert ((rows["record"][sel] == 1) & (rows["pos"][sel] < T32) & (rows["pos"][sel].astype(np.int64) + w > T32)).any(), bulge
    device_rows(big.g.search_bulges_device, big.g.search_bulges_profile_device, bt.NGG, queries, (bt.SPAN, max_dist, D, R), want,
                ca.BULGE_HIT_DTYPE, what, small_first=case == 0)


# ---- 5. SNPs and the variant searches ------------------------------------------------------------------------------------------

def test_snps_and_the_variant_searches(big):
    g = big.g
    snps = bt.snps(big.layout)
    tp = big.layout.text_pos(snps["record"], snps["pos"])
    assert ((tp >= T32) & (snps["pos"] < T32)).any() and (snps["pos"] >= T32).any() and (snps["record"] == 2).any() and (tp < T32).any()
    already = big.layout.island("snp-r2").seq != bt.big().island("snp-r2").seq  # (the text was changed by an earlier run)
    if not already:
        before = check_locate(big)
        # a wrong REF beyond 2^32, between two good entries: refused, and no byte of the text changes
        bad = snps[[1, 12, 30]].copy()
        bad["ref"][1] = 1 if int(bad["ref"][1]) != 1 else 2
        assert int(big.layout.text_pos(bad["record"][1], bad["pos"][1])) >= T32
        with pytest.raises(ca.IsslError) as e:
            g.apply_snps(bad)
        assert e.value.code == -1 and "snp 1:" in e.value.message, e.value.message
        assert check_locate(big) == before
        half = len(snps) // 2
        layout, changed = bt.after_snps(big.layout, snps[:half])
        assert g.apply_snps(snps[:half]) == changed == half
        big.layout = layout
        layout, changed = bt.after_snps(big.layout, snps[half:])
        counts = g.apply_vcf(bt.snps_vcf(big.layout, snps[half:]))
        assert counts["changed"] == changed == len(snps) - half and counts["snps"] == changed
        big.layout = layout
        assert check_locate(big) != before
    twin = big.twin
    coded_places = sum(sum(c not in b"ACGT" for c in i.seq) for i in big.layout.islands)
    assert coded_places == len(snps)
    # locate and the occurrence calls on the changed islands
    check_locate(big)
    check_occurrences(big)
    for max_dist, max_variants in VARIANT_CASES:
        queries = bt.variant_queries()
        want = translated(big.layout, vu.brute_force(twin, bt.NGG, queries, max_dist, max_variants))
        what = "variants max_dist %d max_variants %d" % (max_dist, max_variants)
        rows = host_rows(g.search_variants, g.search_variants_profile, (bt.NGG, queries, max_dist, max_variants), want,
                         ca.VARIANT_HIT_DTYPE, what)
        classes(big, rows)
        assert int(rows["n_var"].max()) == max_variants
        if max_variants:
            classes(big, rows[rows["n_var"] > 0], but=CROSSINGS)
        device_rows(g.search_variants_device, g.search_variants_profile_device, bt.NGG, queries, (max_dist, max_variants), want,
                    ca.VARIANT_HIT_DTYPE, what)
    for max_dist, D, R, max_variants in BULGE_VARIANT_CASES:
        queries = BULGE_VARIANT_QUERIES()
        want = translated(big.layout, bvu.brute_force(twin, bt.NGG, queries, bt.SPAN, max_dist, D, R, max_variants))
        what = "bulge variants max_dist %d dna %d rna %d max_variants %d" % (max_dist, D, R, max_variants)
        rows = host_rows(g.search_bulges_variants, g.search_bulges_variants_profile, (bt.NGG, queries, bt.SPAN, max_dist, D, R, max_variants),
                         want, ca.BULGE_VARIANT_HIT_DTYPE, what)
        classes(big, rows, 23 + rows["bulge"].astype(np.int64))
        if max_variants == 2:
            classes(big, rows[rows["n_var"] > 0], but=CROSSINGS)
        device_rows(g.search_bulges_variants_device, g.search_bulges_variants_profile_device, bt.NGG, queries,
                    (bt.SPAN, max_dist, D, R, max_variants), want, ca.BULGE_VARIANT_HIT_DTYPE, what)


# ---- 6. haplotypes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(HAPLOTYPE_CASES)))
def test_haplotypes(big, case):
    W, max_dist, max_variants = HAPLOTYPE_CASES[case]
    entries, alleles = bt.indels(big.layout)
    tp = big.layout.text_pos(entries["record"], entries["pos"])
    assert ((tp < T32) & (tp + entries["ref_len"] > T32)).any() and (entries["pos"] == T32 - 1).any() and (entries["record"] == 2).any()
    # a wrong REF beyond 2^32 is refused
    k = int(np.flatnonzero(entries["pos"] >= T32)[0])
    wrong = bytearray(alleles)
    at = int(entries["ref_at"][k]) + int(entries["ref_len"][k]) - 1
    wrong[at] = b"ACGT"[(b"ACGT".index(wrong[at]) + 1) % 4]
    with pytest.raises(ca.IsslError) as e:
        big.g.haplotypes(entries, bytes(wrong), W)
    assert e.value.code == -1 and "indel %d:" % k in e.value.message and "REF" in e.value.message, e.value.message
    queries = bt.haplotype_queries(big.layout, W)
    want = bt.haplotypes(big.layout, entries, alleles, "N" * W, queries, max_dist, max_variants)
    what = "haplotypes W %d" % W
    with big.g.haplotypes(entries, alleles, W) as h:
        assert h.info()["n_indels"] == len(entries) and h.info()["window"] == W
        rows = host_rows(h.search, h.search_profile, ("N" * W, queries, max_dist, max_variants), want, ca.HAPLOTYPE_HIT_DTYPE, what)
        classes(big, rows, W)
        assert set(rows["indel"].tolist()) == set(range(len(entries)))
        assert (rows["edit_at"] < 0).any() and (rows["edit_at"] > 0).any()
        device_rows(h.search_device, h.search_profile_device, "N" * W, queries, (max_dist, max_variants), want, ca.HAPLOTYPE_HIT_DTYPE, what)


# ---- 7. landings ---------------------------------------------------------------------------------------------------------------

def test_landings(big):
    import torch
    ref_truth = bt.translate_locations(bt.big(), lu.brute_force(bt.big().twin()))
    sites, occ = np.unique(ref_truth["site"], return_counts=True)
    guides = bt.landing_guides()
    truth = big.truth()
    gff = bt.annotation()
    names = [(n, b"") for n in bt.NAMES]
    with ca.IsslIndex.build_from_sites(sites, occ.astype(np.uint32)).upload(0) as ix, ca.Annotation.open(gff) as ann:
        offs, recs = ix.offtargets(guides, max_dist=LANDING_DIST)
        for annotation, hits in ((None, None), (ann, ldu.location_hits(names, truth, tu.Model(gff)))):
            want_off, want, cnt = ldu.join(len(guides), offs, recs, truth, hits)
            want_prof = ldu.profile(len(guides), recs, cnt, want)
            offsets, rows = ix.landings(guides, big.g, annotation, max_dist=LANDING_DIST)
            assert offsets.tobytes() == want_off.tobytes()
            same(rows, want, "landings")
            classes(big, rows)
            prof = ix.landing_profile(guides, big.g, annotation, max_dist=LANDING_DIST)
            assert prof.tobytes() == want_prof.tobytes()
            if annotation is not None:
                cut = rows[rows["hits"]["hit"] > 0]
                tp = big.layout.text_pos(cut["record"], cut["pos"])
                assert (tp < T32).any() and ((tp >= T32) & (cut["pos"] < T32)).any() and (cut["pos"] >= T32).any() and (cut["record"] == 2).any()
                assert (rows["hits"]["hit"] == 0).any() and int(prof["in_exon"].sum()) == len(cut)
            d_guides = torch.from_numpy(guides.view(np.int64)).cuda()
            d_offs = torch.zeros(len(guides) + 1, dtype=torch.int64, device="cuda")
            d_rows = torch.full((64 * len(want),), 0xAB, dtype=torch.uint8, device="cuda")
            assert ix.landings_device(d_guides, big.g, d_offs, d_rows, annotation, max_dist=LANDING_DIST) == len(want)
            torch.cuda.synchronize()
            assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
            same(d_rows.cpu().numpy().view(ca.LANDING_DTYPE), want, "landings_device")
            d_prof = torch.full((144 * len(guides),), 0xAB, dtype=torch.uint8, device="cuda")
            ix.landing_profile_device(d_guides, big.g, d_prof, annotation, max_dist=LANDING_DIST)
            torch.cuda.synchronize()
            assert d_prof.cpu().numpy().tobytes() == want_prof.tobytes()


# ---- 8. extraction -------------------------------------------------------------------------------------------------------------

def test_guide_extraction(big):
    want = bt.guide_rows(bt.big())  # the extraction reads the FASTA, not the handle's text
    with ca.GuideSet.extract(big.blobs) as gs:
        assert gs.records == list(zip(bt.NAMES, bt.LENGTHS))
        got = gs.guides
        assert gs.strings() == [g.decode() for g in want["guide23"]]
        for f in ("record", "start", "strand", "seen"):
            assert np.array_equal(got[f], want[f]), f
        assert gs.n_matches == int(want["seen"].sum()) and gs.n_unique == int((want["seen"] == 1).sum())
        classes(big, got, pos="start")
        twice = got[got["seen"] > 1]
        assert len(twice) >= 3 and (big.layout.text_pos(twice["record"], twice["start"]) < T32).any()


def test_site_extraction(big):
    got = ca.extract_offtargets(big.blobs)
    want = oracle_extract([gt.fasta(bt.big().twin())])
    assert got == want and len(want) // 21 == len(lu.brute_force(bt.big().twin()))
