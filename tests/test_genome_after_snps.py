"""Every reader of a genome handle after issl_genome_apply_snps / issl_genome_apply_vcf: locate, the occurrence calls (plain,
paged and with page boundaries), the plain search, the bulge search, the variant search and the landings, each against its
model on the text WITH the codes (tests/genome_text_util.py) -- on the reference, on the reference after apply_snps, and on a
handle opened from the coded FASTA, whose bytes must be those of the second.  The tests that need a device carry the gpu
mark; the others assert on the models alone that the SNPs take away what the tests think they take away."""
import functools

import numpy as np
import pytest

import crackling_amd as ca
import bowtie_util as bwu
import genome_text_util as gt
import locate_util as lu
import search_util as su
import variant_util as vu
from test_variants_gpu import same_text, variant_case

gpu = pytest.mark.gpu
NGG = gt.NGG
TILE = 4096
READERS = ("locate", "occurrences", "search", "bulges", "variants", "landings")


class Asked:
    """What the readers are asked on the texts of one case: the same for every handle."""

    def __init__(self, ref_records, records, queries, seed=3, n_guides=48):
        self.sites = gt.sites_of(ref_records, records, extra=40, seed=seed)  # of the coded text, and some only the reference has
        self.queries = list(queries)
        ref_sites, occ = np.unique(gt.Truth.of(ref_records).locate["site"], return_counts=True)
        # guides: the first sites that occur more than once, and sites spread over the whole list
        self.guides = np.unique(np.concatenate([ref_sites[occ > 1][:24], ref_sites[np.linspace(0, len(ref_sites) - 1, n_guides).astype(np.int64)]]))

    def check(self, reader, records, g, ix=None):
        """One reader on handle g against the model of `records`.  -> its bytes"""
        if reader == "locate":
            return gt.check_locate(records, g, self.sites)
        if reader == "occurrences":
            return gt.check_occurrences(records, g, self.sites)
        if reader == "search":
            return gt.check_search(records, g, self.queries)
        if reader == "bulges":
            return gt.check_bulges(records, g, self.queries)
        if reader == "variants":
            return gt.check_variants(records, g, self.queries)
        return gt.check_landings(records, g, ix, self.guides)

    def check_all(self, records, g, ix):
        return {r: self.check(r, records, g, ix) for r in READERS}


# ---- the main case -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def main_case():
    """variant_case(7, 12000, 30, 70) of tests/test_variants_gpu.py: 12 000 bases in two records, 387 SNPs.  The queries: ten
    of its own (spelled with ALT alleles), eight read off the reference (two of them through a bulge), one named twice and the
    all-N query."""
    blob, ref_records, snps, records, queries = variant_case(7, 12000, 30, 70)
    mine = queries[:10] + gt.queries_of(ref_records, np.random.default_rng(70))
    mine += [mine[11], "N" * 23]
    return ref_records, snps, records, Asked(ref_records, records, mine)


@functools.lru_cache(maxsize=None)
def repeat_case():
    """genome_text_util.repeat_case: sites that occur several times in the reference and less often once the SNPs are in."""
    ref_records, snps, records = gt.repeat_case()
    queries = gt.queries_of(ref_records, np.random.default_rng(71)) + ["N" * 23]
    return ref_records, snps, records, Asked(ref_records, records, queries, seed=4)


def lost_landings(case, max_dist=2):
    """From the models: the landings of the case's guides on the reference and on the coded text.
    -> (off-target records, landings per record before, after)"""
    ref_records, _, records, asked = case
    offs, recs = gt.model_offtargets(ref_records, asked.guides, max_dist)
    before = gt.landing_model(ref_records, asked.guides, offs, recs)[3]
    after = gt.landing_model(records, asked.guides, offs, recs)[3]
    return recs, before, after


def test_the_main_case_is_not_vacuous():
    ref_records, snps, records, asked = main_case()
    ref, coded = gt.Truth.of(ref_records), gt.Truth.of(records)
    assert len(snps) == 387 and sum(len(s) for _, s in records) == 12000
    # locate: the truth shrinks by at least a third and keeps at least a third
    assert (len(ref.locate), len(coded.locate)) == (2181, 996)
    assert 3 * len(coded.locate) <= 2 * len(ref.locate) and 3 * len(coded.locate) >= len(ref.locate)
    assert len(np.setdiff1d(asked.sites, coded.locate["site"])) > 1000  # asked, and only the reference has them
    # the occurrence reads
    assert (len(ref.bowtie.occ), len(coded.bowtie.occ)) == (2966, 1374)
    assert 3 * len(coded.bowtie.occ) <= 2 * len(ref.bowtie.occ) and 3 * len(coded.bowtie.occ) >= len(ref.bowtie.occ)
    before, after = ref.bowtie.rows(asked.sites), coded.bowtie.rows(asked.sites)
    assert 2 * int((before["aligned"] != 0).sum()) > 3 * int((after["aligned"] != 0).sum()) > 0
    # the searches: rows of every bulge before and after, fewer after; the variant search has rows the plain one lost
    for t in (ref, coded):
        _, rows, _ = t.bulges(NGG, asked.queries, gt.SPAN, 2, 1, 1)
        assert set(rows["bulge"].tolist()) == {-1, 0, 1}
        named = rows[rows["query"] < len(asked.queries) - 1]  # all but the all-N query
        assert set(named["bulge"].tolist()) == {-1, 0, 1} or t is coded
    plain_ref, plain = ref.search(NGG, asked.queries, 2)[1], coded.search(NGG, asked.queries, 2)[1]
    assert 3 * len(plain) <= 2 * len(plain_ref) and len(plain) > 100
    assert len(coded.variants(NGG, asked.queries, 2, 2)[1]) > len(plain) + 100
    # the landings: at least ten are lost
    recs, cnt_ref, cnt = lost_landings(main_case())
    assert np.array_equal(cnt_ref, recs["occ"]) and int(cnt_ref.sum() - cnt.sum()) >= 10 and int(cnt.sum()) >= 10
    assert int((cnt == 0).sum()) >= 10  # sites that lost every place: `absent`


def test_the_repeat_case_loses_some_places_of_a_site_and_keeps_others():
    """No 20-mer of the main case's random text occurs twice, so a site there is lost whole or not at all; here a site of the
    element occurs four times (the forward copies) or twice (the reversed ones) and loses some of its places."""
    ref_records, snps, records, asked = repeat_case()
    recs, cnt_ref, cnt = lost_landings(repeat_case())
    assert np.array_equal(cnt_ref, recs["occ"])
    partly = (cnt > 0) & (cnt < recs["occ"])
    assert int(partly.sum()) >= 1 and sorted(set(recs["occ"][partly].tolist())) == [2, 4]
    assert ((cnt == 0) & (recs["occ"] > 0)).any() and (cnt == recs["occ"]).any()
    ref, coded = gt.Truth.of(ref_records), gt.Truth.of(records)
    repeated = lambda t: sum(1 for where in t.bowtie.occ.values() if len(where) > 1)  # noqa: E731
    assert repeated(ref) > repeated(coded) > 0


def three_handles(case):
    ref_records, snps, records, asked = case
    ref_blob = gt.fasta(ref_records)
    with ca.IsslIndex.build_from_fasta([ref_blob]) as ix, ca.Genome.open([ref_blob]) as plain, ca.Genome.open([ref_blob]) as applied, \
            ca.Genome.open([gt.fasta(records)]) as opened:
        assert applied.apply_snps(snps) == len(snps)
        yield ix, plain, applied, opened


@gpu
@pytest.mark.parametrize("case", [main_case, repeat_case], ids=["main", "repeat"])
def test_every_reader_on_three_handles(case):
    ref_records, snps, records, asked = case()
    for ix, plain, applied, opened in three_handles(case()):
        on_ref = asked.check_all(ref_records, plain, ix)
        after = asked.check_all(records, applied, ix)
        from_fasta = asked.check_all(records, opened, ix)
        for reader in READERS:
            assert after[reader] == from_fasta[reader], reader  # however the codes got there
            assert after[reader] != on_ref[reader], reader


# ---- a code at every offset of one site ----------------------------------------------------------------------------------

RG = "N" * 21 + "RG"


@functools.lru_cache(maxsize=None)
def offset_text():
    """4 300 random bases with one 20-mer planted twice: + AGG inside the first tile, + AAG from text position 4096 - 11 on."""
    rng = np.random.default_rng(23)
    text = list("".join("ACGT"[c] for c in rng.integers(0, 4, size=4300)))
    guide = "G" + "".join("ACGT"[c] for c in rng.integers(0, 4, size=19))
    starts = (1000, TILE - 11)
    for start, pam in zip(starts, ("AGG", "AAG")):
        text[start:start + 23] = guide + pam
    return [(b"one record", "".join(text).encode())], guide, starts


@functools.lru_cache(maxsize=None)
def offset_case(o):
    """-> (ref_records, the two SNPs at offset o of the two plants, records, guide, starts)"""
    ref_records, guide, starts = offset_text()
    snps = np.zeros(2, dtype=ca.SNP_DTYPE)
    for k, start in enumerate(starts):
        r = "ACGT".index(chr(ref_records[0][1][start + o]))
        snps[k] = (start + o, 0, 1 << r, 1 << ((r + 1 + (o + k) % 3) % 4), (0, 0))
    records, changed = vu.apply_snps(ref_records, snps)
    assert changed == 2
    return ref_records, snps, records, guide, starts


def site_rows(rows, starts, over=0):
    """The rows of query 0 at the two plants, strand 0, whose window covers offset `over` (a bulged window has 23 + bulge bases:
    with a code in the PAM's last two bases the shorter windows at the plant do not hold it)."""
    width = lambda r: 23 + (int(r["bulge"]) if "bulge" in rows.dtype.names else 0)  # noqa: E731
    return [r for r in rows if int(r["query"]) == 0 and int(r["strand"]) == 0 and int(r["pos"]) in starts and width(r) > over]


@pytest.mark.parametrize("o", range(23))
def test_the_models_lose_the_site_at_every_offset(o):
    ref_records, snps, records, guide, starts = offset_case(o)
    ref, coded = gt.Truth.of(ref_records), gt.Truth.of(records)
    sig = bwu.sig(guide)
    place = lambda t: [(int(x["pos"]), int(x["strand"])) for x in t.locate[t.locate["site"] == np.uint64(sig)]]  # noqa: E731
    assert place(ref) == [(starts[0], 0), (starts[1], 0)] and place(coded) == []
    row = lambda t: t.bowtie.rows(np.array([sig], dtype=np.uint64))[0]  # noqa: E731
    assert int(row(ref)["aligned"]) == 0b10001 and int(row(ref)["record"]) == 0 and int(row(ref)["pos"]) == starts[0]
    assert int(row(coded)["aligned"]) == 0 and int(row(coded)["record"]) == bwu.NONE
    queries = [guide + "NNN"]
    assert len(site_rows(ref.search(RG, queries, 1)[1], starts)) == 2 and not site_rows(coded.search(RG, queries, 1)[1], starts)
    assert len(site_rows(ref.bulges(RG, queries, gt.SPAN, 1, 1, 1)[1], starts)) >= 2
    assert not site_rows(coded.bulges(RG, queries, gt.SPAN, 1, 1, 1)[1], starts, over=o)
    kept = site_rows(coded.variants(RG, queries, 1, 1)[1], starts)
    assert len(kept) == 2 and all(int(r["n_var"]) == 1 and int(r["dist"]) == 0 for r in kept)
    assert not site_rows(coded.variants(RG, queries, 1, 0)[1], starts)


@pytest.fixture(scope="module")
def offset_index():
    ref_records, _, _ = offset_text()
    with ca.IsslIndex.build_from_fasta([gt.fasta(ref_records)]) as ix:
        yield ix


@gpu
@pytest.mark.parametrize("o", range(23))
def test_a_code_at_every_offset_of_a_site(o, offset_index):
    ref_records, snps, records, guide, starts = offset_case(o)
    sites = np.array([bwu.sig(guide), bwu.sig(su.revcomp(guide)), bwu.sig(guide[1:] + "A")], dtype=np.uint64)
    queries = [guide + "NNN", "N" * 23]
    with ca.Genome.open([gt.fasta(ref_records)]) as g:
        if o == 0:  # the reference, once
            assert np.diff(g.locate(sites[:1])[0].astype(np.int64)).tolist() == [2]
            gt.check_locate(ref_records, g, sites)
            gt.check_occurrences(ref_records, g, sites)
            gt.check_landings(ref_records, g, offset_index, sites[:1], 0)
        assert g.apply_snps(snps) == 2
        assert g.locate(sites[:1])[0].tolist() == [0, 0]
        gt.check_locate(records, g, sites)
        assert int(g.occurrences(sites[:1])["aligned"][0]) == 0
        gt.check_occurrences(records, g, sites)
        gt.check_search(records, g, queries, 1, RG)
        gt.check_bulges(records, g, queries, 1, RG)
        gt.check_variants(records, g, queries, 1, 1, RG)
        gt.check_variants(records, g, queries, 1, 0, RG)
        gt.check_landings(records, g, offset_index, sites[:1], 0)
        prof = offset_index.landing_profile(sites[:1], g, None, max_dist=0)
        assert int(prof["absent"][0, 0]) == 1 and not prof["located"].any()


# ---- sequences on one handle ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sequence_case():
    """6 000 bases in two records and four lists of SNPs: A and B share no place, C names a third of A's places again with
    another allele and places of its own, and a VCF of further places; one list that is refused at input index 1."""
    blob, ref_records, snps, records, queries = variant_case(19, 6000, 25, 12)
    rng = np.random.default_rng(190)
    rest, vcf_snps = snps[:-12], snps[-12:]
    a, b = rest[0::3].copy(), rest[1::3].copy()
    c = np.concatenate([rest[2::3], a[::3]])
    for k in range(len(rest[2::3]), len(c)):  # a third allele at a place of A
        ref, alt = int(c["ref"][k]), int(c["alt"][k])
        c["alt"][k] = [m for m in (1, 2, 4, 8) if m not in (ref, alt)][int(rng.integers(0, 2))]
    rng.shuffle(c)
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for s in vcf_snps:
        lines.append(b"rec%d\t%d\t.\t%s\t%s,<DEL>" % (s["record"], s["pos"] + 1, b"ACGT"[int(s["ref"]).bit_length() - 1:][:1],
                                                   b"ACGT"[int(s["alt"]).bit_length() - 1:][:1]))
    vcf = b"\n".join(lines) + b"\n"
    refused = b[:3].copy()  # a base the text does not hold there, before B is applied or after
    refused["ref"][1] = [m for m in (1, 2, 4, 8) if m not in (int(b["ref"][1]), int(b["alt"][1]))][0]
    every = [ref_records]
    for step in (a, b, c, vu.vcf_snps(vcf, ref_records)[0]):
        every.append(vu.apply_snps(every[-1], step)[0])
    queries = queries[:6] + gt.queries_of(ref_records, rng, 4) + ["N" * 23]
    return ref_records, {"A": a, "B": b, "C": c, "vcf": vcf, "refused": refused}, Asked(ref_records, every[-1], queries, seed=5, n_guides=24), every[-1]


SEQUENCES = [
    ["locate", "A", "occurrences", "search_device", "B", "bulges", "refused", "variants", "C", "landings", "vcf", "locate_device",
     "occurrences_device", "landings_device"],
    ["B", "landings", "refused", "locate_device", "A", "search", "vcf", "occurrences_device", "bulges", "C", "variants", "search_device",
     "locate", "occurrences"],
    ["search", "vcf", "C", "occurrences", "landings_device", "B", "locate", "variants", "A", "refused", "bulges", "search_device",
     "occurrences_device", "landings"],
]


def test_the_sequences_mix_every_reader_with_every_list():
    ref_records, lists, asked, final = sequence_case()
    places = lambda s: set(zip(s["record"].tolist(), s["pos"].tolist()))  # noqa: E731
    assert not places(lists["A"]) & places(lists["B"]) and len(places(lists["C"]) & places(lists["A"])) >= 5 and places(lists["C"]) - places(lists["A"])
    with pytest.raises(vu.Refused) as m:
        vu.apply_snps(ref_records, lists["refused"])
    assert m.value.index == 1
    for seq in SEQUENCES:
        assert {"A", "B", "C", "vcf", "refused"} <= set(seq) and all(r in seq or r + "_device" in seq for r in READERS) and 12 <= len(seq) <= 14
        assert len({"locate_device", "occurrences_device", "landings_device"} & set(seq)) >= 2 and "search_device" in seq  # (on a stream)
        records = ref_records
        for step in seq:  # whatever the order, the lists apply and the text ends the same
            if step in ("A", "B", "C"):
                records, changed = vu.apply_snps(records, lists[step])
                assert changed >= 5
            elif step == "vcf":
                records, changed = vu.apply_snps(records, vu.vcf_snps(lists["vcf"], records)[0])
                assert changed == 12
        assert records == final
    assert SEQUENCES[0].index("A") < SEQUENCES[0].index("B") and SEQUENCES[1].index("B") < SEQUENCES[1].index("A")
    assert SEQUENCES[2].index("C") < SEQUENCES[2].index("A")  # the list that overlaps A ahead of A


def device_reader(step, records, g, ix, asked):
    """The _device form of a reader against the model of `records`; the search runs on a torch stream of its own."""
    import torch
    t = gt.Truth.of(records)
    if step == "locate_device":
        sites = asked.sites
        d_sites = torch.from_numpy(sites.view(np.int64)).cuda()
        d_offs = torch.zeros(len(sites) + 1, dtype=torch.int64, device="cuda")
        total = g.locate_device(d_sites, d_offs, None)
        d_locs = torch.full((16 * max(total, 1),), 0xAB, dtype=torch.uint8, device="cuda")
        assert g.locate_device(d_sites, d_offs, d_locs) == total
        torch.cuda.synchronize()
        locs = d_locs.cpu().numpy()[:16 * total].view(ca.LOCATION_DTYPE)
        lu.check_locate(g.records, d_offs.cpu().numpy().view(np.uint64), locs, sites, t.locate)
    elif step == "occurrences_device":
        d_sigs = torch.from_numpy(asked.sites.view(np.int64)).cuda()
        d_rows = torch.full((len(asked.sites), 32), 0xAB, dtype=torch.uint8, device="cuda")
        g.occurrences_device(d_sigs, d_rows, 7)
        bwu.same_rows(d_rows.cpu().numpy().view(bwu.DTYPE).reshape(-1), t.bowtie.rows(asked.sites, 7))
        starts = gt.ragged_starts(len(asked.sites))
        g.occurrences_device(d_sigs, d_rows, page_starts=torch.from_numpy(starts.view(np.int64)).cuda())
        import batches_util as bt
        bwu.same_rows(d_rows.cpu().numpy().view(bwu.DTYPE).reshape(-1), bt.paged_rows(t.bowtie, asked.sites, starts))
    elif step == "search_device":
        want_off, want_rows, want_prof = t.search(NGG, asked.queries, 2)
        pat, q = ca.search_prepare(NGG, asked.queries)
        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((len(q) + 1,), -1, dtype=torch.int64, device="cuda")
        d_hits = torch.full((len(want_rows) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_device(pat, d_q, d_off, d_hits, 2, stream=stream.cuda_stream) == len(want_rows)
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes() and d_hits.cpu().numpy().tobytes() == want_rows.tobytes()
    else:
        assert step == "landings_device"
        guides = asked.guides
        offs, recs = ix.offtargets(guides, max_dist=2)
        want_off, want, want_prof, _ = gt.landing_model(records, guides, offs, recs)
        d_guides = torch.from_numpy(guides.view(np.int64)).cuda()
        d_offs = torch.zeros(len(guides) + 1, dtype=torch.int64, device="cuda")
        d_rows = torch.full((64 * (len(want) + 1),), 0xAB, dtype=torch.uint8, device="cuda")
        assert ix.landings_device(d_guides, g, d_offs, d_rows, None, max_dist=2) == len(want)
        torch.cuda.synchronize()
        assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        assert d_rows.cpu().numpy()[:64 * len(want)].tobytes() == want.tobytes()
        d_prof = torch.full((144 * len(guides),), 0xAB, dtype=torch.uint8, device="cuda")
        ix.landing_profile_device(d_guides, g, d_prof, None, max_dist=2)
        torch.cuda.synchronize()
        assert d_prof.cpu().numpy().tobytes() == want_prof.tobytes()


@pytest.fixture(scope="module")
def sequence_index():
    ref_records = sequence_case()[0]
    with ca.IsslIndex.build_from_fasta([gt.fasta(ref_records)]) as ix:
        yield ix


@gpu
@pytest.mark.parametrize("which", range(len(SEQUENCES)))
def test_sequences_on_one_handle(which, sequence_index):
    ref_records, lists, asked, final = sequence_case()
    records = ref_records
    with ca.Genome.open([gt.fasta(ref_records)]) as g:
        for step in SEQUENCES[which]:
            if step in ("A", "B", "C"):
                records, changed = vu.apply_snps(records, lists[step])
                assert g.apply_snps(lists[step]) == changed
                same_text(g, records)
            elif step == "vcf":
                records, changed = vu.apply_snps(records, vu.vcf_snps(lists["vcf"], records)[0])
                assert g.apply_vcf(lists["vcf"])["changed"] == changed
                same_text(g, records)
            elif step == "refused":
                with pytest.raises(vu.Refused):
                    vu.apply_snps(records, lists["refused"])
                before = asked.check_all(records, g, sequence_index)
                with pytest.raises(ca.IsslError) as e:
                    g.apply_snps(lists["refused"])
                assert e.value.code == -1 and "snp 1:" in e.value.message, e.value.message
                assert asked.check_all(records, g, sequence_index) == before  # no reader's bytes change
            elif step.endswith("_device"):
                device_reader(step, records, g, sequence_index, asked)
            else:
                asked.check(step, records, g, sequence_index)
        assert records == final
        asked.check_all(final, g, sequence_index)


@gpu
def test_the_order_of_two_lists_does_not_show(sequence_index):
    ref_records, lists, asked, _ = sequence_case()
    blob = gt.fasta(ref_records)
    both = vu.apply_snps(vu.apply_snps(ref_records, lists["A"])[0], lists["B"])[0]
    with ca.Genome.open([blob]) as ab, ca.Genome.open([blob]) as ba:
        ab.apply_snps(lists["A"]), ab.apply_snps(lists["B"])
        ba.apply_snps(lists["B"]), ba.apply_snps(lists["A"])
        assert asked.check_all(both, ab, sequence_index) == asked.check_all(both, ba, sequence_index)


# ---- two handles ---------------------------------------------------------------------------------------------------------

@gpu
def test_snps_on_one_handle_never_show_in_another(sequence_index):
    ref_records, lists, asked, _ = sequence_case()
    blob = gt.fasta(ref_records)
    coded = vu.apply_snps(ref_records, lists["A"])[0]
    with ca.Genome.open([blob]) as one, ca.Genome.open([blob]) as other:
        before = asked.check_all(ref_records, other, sequence_index)
        assert one.apply_snps(lists["A"]) == len(lists["A"])
        changed = asked.check_all(coded, one, sequence_index)
        assert asked.check_all(ref_records, other, sequence_index) == before
        same_text(other, ref_records)
        assert all(changed[r] != before[r] for r in READERS)
        assert other.apply_snps(lists["B"]) == len(lists["B"])  # and the other way round
        assert asked.check_all(coded, one, sequence_index) == changed
