"""GPU: issl_genome_search_bulges_variants* and bin/isslSearchGenome --guide-variants / --guide-vcf against the brute force of
tests/bulge_variant_util.py (the loop of the bulge search's brute force around the variant search's, pinned on the CPU by
test_bulge_variants_model.py): rows, offsets and profile byte for byte."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import bulge_util as bu
import bulge_variant_util as bvu
import locate_util as lu
import search_util as su

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslSearchGenome")
NGG = "N" * 21 + "GG"
TILE = 4096  # kPosPerBlock: text positions per workgroup; its planes are words of 32 positions
GROUP = 4    # kQueryGroup: queries whose bounds share one branch; what is left behind the last whole group goes one by one
AMBIGUOUS = "RYSWKMBDHV"
ROW = 48
COMP = str.maketrans("ACGTRYSWKMBDHV", "TGCAYRSWMKVHDB")


def random_text(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def revcomp(s):
    """Of a text with codes: R <-> Y, K <-> M, B <-> V, D <-> H."""
    return s[::-1].translate(COMP)


def fasta_of(seqs):
    return b"".join(b">rec%d some text\n%s\n" % (k, s.encode()) for k, s in enumerate(seqs))


def mutate(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), size=k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def bulged(guide, b, i, rng):
    """The guide's site under alignment (b, i): b > 0 bases put in at i, or -b bases of the guide left out."""
    return guide[:i] + random_text(rng, max(b, 0)) + guide[i + max(-b, 0):]


def code_over(rng, base, other=None):
    """An ambiguity code whose set holds `base` (and `other`)."""
    fits = [c for c in AMBIGUOUS if base in su.IUPAC[c] and (other is None or other in su.IUPAC[c])]
    return fits[int(rng.integers(0, len(fits)))]


def other_base(rng, base):
    return "ACGT"[("ACGT".index(base) + 1 + int(rng.integers(0, 3))) % 4]


def coded_at(rng, site, p):
    """(the site with a code at p whose set holds the site's base, the reference text under it: another base of the set)"""
    ref = other_base(rng, site[p])
    return site[:p] + code_over(rng, site[p], ref) + site[p + 1:], site[:p] + ref + site[p + 1:]


def sprinkle(rng, text, every):
    """`text` (a list, the reference) -> a copy with an ambiguity code over about one base in `every`."""
    coded = list(text)
    for i in np.flatnonzero(rng.random(len(text)) < 1.0 / every):
        coded[i] = code_over(rng, text[i])
    return coded


def snps_between(ref_seqs, coded_seqs):
    """-> (SNP_DTYPE array, VCF text) that turn the reference records into the coded ones."""
    snps, lines = [], [b"##fileformat=VCFv4.2"]
    for r, (ref, coded) in enumerate(zip(ref_seqs, coded_seqs)):
        for p in np.flatnonzero(np.frombuffer(ref.encode(), np.uint8) != np.frombuffer(coded.encode(), np.uint8)):
            alts = [x for x in su.IUPAC[coded[p]] if x != ref[p]]
            assert ref[p] in su.IUPAC[coded[p]] and alts
            snps.append((int(p), r, 1 << "ACGT".index(ref[p]), sum(1 << "ACGT".index(x) for x in alts), (0, 0)))
            lines.append(b"rec%d\t%d\t.\t%s\t%s\t50\tPASS" % (r, p + 1, ref[p].encode(), ",".join(alts).encode()))
    return np.array(snps, dtype=ca.SNP_DTYPE), b"\n".join(lines) + b"\n"


def check(blobs, pattern, queries, span, max_dist, D, R, mv, genome=None, want=None):
    """One search and one profile on the device equal the brute force, byte for byte.  -> (offsets, rows)"""
    want_off, want_rows, want_prof = want or bvu.brute_force_fasta(blobs, pattern, queries, span, max_dist, D, R, mv)
    g = genome or ca.Genome.open(blobs)
    try:
        off, rows = g.search_bulges_variants(pattern, queries, span, max_dist, D, R, mv)
        prof = g.search_bulges_variants_profile(pattern, queries, span, max_dist, D, R, mv)
    finally:
        if genome is None:
            g.close()
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == ca.BULGE_VARIANT_HIT_DTYPE and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    counted = np.zeros_like(prof)  # the profile is the rows counted by (bulge, dist)
    np.add.at(counted, (rows["query"], rows["bulge"].astype(np.int64) + R, rows["dist"]), 1)
    assert np.array_equal(counted, prof) and not rows["reserved"].any()
    return off, rows


def keys_of(rows):
    return {(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["bulge"])) for r in rows}


# ---- NGG: every class of row on both strands ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ngg_case():
    """L = 23, span (0, 20), D = R = 2, max_dist 3, max_variants 2 on 2 x TILE + 100 bases in three records, a code over about
    one base in 90.  Planted for every b in -2..2 on both strands: a site with a code over one of its bases, and a site with
    one mismatch whose PAM is TRG where the reference has TAG.  Beside them a homopolymer tie, and a site with three codes
    (on either strand), which max_variants drops.  10 queries, one of them all N and one named twice."""
    rng = np.random.default_rng(2025)
    G, n = 20, 2 * TILE + 100
    ref = list(random_text(rng, n))
    text = sprinkle(rng, ref, 90)
    guides = [random_text(rng, G) for _ in range(3)]
    run = random_text(rng, 8) + "AAAA" + random_text(rng, 8)  # a DNA bulge of A inside the run ties between break points
    plants = []  # (strand, the site with its codes, the reference under it)
    for b in (-2, -1, 0, 1, 2):
        for strand in (0, 1):
            guide = guides[(b + strand) % 3]
            i = 1 + (7 * strand + 3 * b) % (G - 1 - max(-b, 0)) if b else 0
            site = bulged(guide, b, i, rng)
            plants.append((strand,) + tuple(x + "TGG" for x in coded_at(rng, site, int(rng.integers(0, len(site))))))
            site = mutate(rng, bulged(guide, b, i, rng), 1)
            plants.append((strand, site + "TRG", site + "TAG"))
    plants.append((0, run[:10] + "A" + run[10:] + "CGG", run[:10] + "A" + run[10:] + "CGG"))
    plants.append((1, run[:9] + run[10:] + "CGG", run[:9] + run[10:] + "CGG"))
    triple = guides[0]
    for p in (8, 10, 12):
        triple = triple[:p] + code_over(rng, triple[p]) + triple[p + 1:]
    at, dropped_at = 60, []
    for strand, coded, plain in plants + [(0, triple + "TGG", guides[0] + "TGG"), (1, triple + "TGG", guides[0] + "TGG")]:
        if coded.startswith(triple):
            dropped_at.append(at)
        text[at - 10:at + 36] = ref[at - 10:at + 36]  # no other code nearby
        text[at:at + len(coded)] = coded if strand == 0 else revcomp(coded)
        ref[at:at + len(plain)] = plain if strand == 0 else su.revcomp(plain)
        at += 340
    assert at < 8250 and len(dropped_at) == 2
    text, ref = "".join(text), "".join(ref)
    cut = lambda s: [s[:3000], s[3000:8250], s[8250:]]
    blob, ref_blob = fasta_of(cut(text)), fasta_of(cut(ref))
    records = lu.parse([blob])
    queries = [g + "NNN" for g in guides] + [run + "NNN"] + [random_text(rng, G) + "NNN" for _ in range(4)] + ["N" * 23, guides[1] + "NNN"]
    ties = []
    want = bvu.brute_force(records, NGG, queries, (0, G), 3, 2, 2, 2, ties=ties)
    return dict(blob=blob, ref_blob=ref_blob, records=records, queries=queries, want=want, ties=ties, dropped_at=dropped_at,
                text=text, ref=ref, cut=cut)


def test_the_brute_force_covers_every_class(ngg_case):
    """Asserted on the brute force alone, so that a failure cannot hide behind an agreement of two empty lists."""
    queries, (offsets, rows, profile), ties = ngg_case["queries"], ngg_case["want"], ngg_case["ties"]
    planted = rows[rows["query"] < 4]
    on_reference = keys_of(bu.brute_force(lu.parse([ngg_case["ref_blob"]]), NGG, queries[:4], (0, 20), 3, 2, 2)[1])
    assert on_reference  # (the reference has rows of its own: what is absent below is absent because of an allele)
    for b in (-2, -1, 0, 1, 2):
        for strand in (0, 1):
            mine = planted[(planted["bulge"] == b) & (planted["strand"] == strand)]
            assert (mine["n_var"] >= 1).any(), (b, strand)                # a row over a code
            assert keys_of(mine) - on_reference, (b, strand)              # a row whose minimum needs an alt allele
            if b:
                assert [k for k in ties if k[3] == strand and k[4] == b], (b, strand)  # a tie of break points
    assert any(k[0] == 3 for k in ties)
    # the site with three codes: with max_variants 3 it has rows of every b on either strand, with 2 it has none of them
    for strand, at in enumerate(ngg_case["dropped_at"]):
        near = [(b"rec0", ngg_case["text"][at - 10:at + 36].encode())]
        kept = keys_of(bvu.brute_force(near, NGG, queries[:1], (0, 20), 3, 2, 2, 2)[1])
        lost = keys_of(bvu.brute_force(near, NGG, queries[:1], (0, 20), 3, 2, 2, 3)[1]) - kept
        assert {k[4] for k in lost if k[3] == strand} == {-2, -1, 0, 1, 2}
        assert not {(q, r, pos + at - 10, s, b) for q, r, pos, s, b in lost} & keys_of(rows)
    assert (np.diff(offsets.astype(np.int64))[:4] > 0).all() and int(offsets[-2] - offsets[-3]) > 1000  # the all-N query
    a, b = rows[int(offsets[1]):int(offsets[2])].copy(), rows[int(offsets[-2]):].copy()  # the query named twice
    a["query"] = b["query"] = 0
    assert len(a) and a.tobytes() == b.tobytes()


def test_ngg_rows_offsets_and_profile(ngg_case):
    with ca.Genome.open([ngg_case["blob"]]) as g:
        off, rows = check(None, NGG, ngg_case["queries"], (0, 20), 3, 2, 2, 2, genome=g, want=ngg_case["want"])
        off2, rows2 = g.search_bulges_variants(NGG, ngg_case["queries"], (0, 20), 3, 2, 2, 2)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs


def test_device_entry_points_on_a_stream(ngg_case):
    import torch
    queries, (want_off, want_rows, want_prof) = ngg_case["queries"], ngg_case["want"]
    pat, q = ca.search_prepare(NGG, queries)
    d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_off = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda")
    with ca.Genome.open([ngg_case["blob"]]) as g:
        total = g.search_bulges_variants_device(pat, d_q, d_off, None, (0, 20), 3, 2, 2, 2)  # the counting call
        assert total == len(want_rows) and d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        assert g.search_bulges_variants_device(pat, d_q, d_off, d_hits[:(total - 1) * ROW], (0, 20), 3, 2, 2, 2) == total
        assert bool((d_hits == 0xA5).all())  # they do not fit: nothing is written
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_bulges_variants_device(NGG, d_q, d_off, d_hits, (0, 20), 3, 2, 2, 2, stream=stream.cuda_stream) == total
        assert d_hits.cpu().numpy().view(ca.BULGE_VARIANT_HIT_DTYPE).tobytes() == want_rows.tobytes()
        d_counts = torch.full((want_prof.size,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        g.search_bulges_variants_profile_device(pat, d_q, d_counts, (0, 20), 3, 2, 2, 2, stream=stream.cuda_stream)
        assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes()
        with pytest.raises(ValueError):
            g.search_bulges_variants_profile_device(pat, d_q, d_counts[:-1], (0, 20), 3, 2, 2, 2)
        assert g.search_bulges_variants_device(pat, d_q[:0], d_off[:1], None, (0, 20), 3, 2, 2, 2) == 0 and int(d_off[0]) == 0  # n == 0


def test_capacity_rule(ngg_case):
    queries, (want_off, want_rows, _) = ngg_case["queries"], ngg_case["want"]
    pat, q = ca.search_prepare(NGG, queries)
    bg = _lib.SearchBulges(0, 20, 2, 2)
    total = len(want_rows)
    with ca.Genome.open([ngg_case["blob"]]) as g:
        poison = np.full(total * ROW, 0xA5, dtype=np.uint8)
        off = np.full(len(queries) + 1, 0xFFFFFFFF, dtype=np.uint64)
        n = C.c_size_t()
        args = (g._h, C.byref(pat), C.byref(bg), q.ctypes.data, len(queries), 3, 2, off.ctypes.data)
        assert _lib.lib.issl_genome_search_bulges_variants(*args, None, 0, C.byref(n)) == 0  # the counting call
        assert n.value == total and off.tobytes() == want_off.tobytes()
        off[:] = 0xFFFFFFFF
        assert _lib.lib.issl_genome_search_bulges_variants(*args, poison.ctypes.data, total - 1, C.byref(n)) == 0
        assert n.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
        assert _lib.lib.issl_genome_search_bulges_variants(*args, poison.ctypes.data, total, C.byref(n)) == 0
        assert poison.tobytes() == want_rows.tobytes()
        off, rows = g.search_bulges_variants(NGG, [], (0, 20), 3, 2, 2, 2)  # n == 0
        assert off.tolist() == [0] and len(rows) == 0 and g.search_bulges_variants_profile(NGG, [], (0, 20), 3, 2, 2, 2).shape == (0, 5, 4)


# ---- the identities, on the device -------------------------------------------------------------------------------------

def test_without_bulges_the_rows_of_the_variant_search(ngg_case):
    queries = ngg_case["queries"]
    with ca.Genome.open([ngg_case["blob"]]) as g:
        for pattern, span, mv in ((NGG, (0, 20), 2), ("NNRNNNNNNNNNNNNNNNNNNGG", (0, 23), 3)):  # any code inside the span
            off, rows = g.search_bulges_variants(pattern, queries, span, 3, 0, 0, mv)
            want_off, want_rows = g.search_variants(pattern, queries, 3, mv)
            assert off.tobytes() == want_off.tobytes() and len(rows) == len(want_rows) > 400
            assert rows.tobytes() == bvu.from_variants(want_rows).tobytes() and (rows["n_var"] > 0).any()
            prof = g.search_bulges_variants_profile(pattern, queries, span, 3, 0, 0, mv)
            assert prof.shape == (len(queries), 1, 4) and np.array_equal(prof[:, 0], g.search_variants_profile(pattern, queries, 3, mv))


def test_max_variants_0_and_a_clean_text_give_the_rows_of_the_bulge_search(ngg_case):
    queries = ngg_case["queries"]
    for blob, mv in ((ngg_case["blob"], 0), (ngg_case["ref_blob"], 2), (ngg_case["ref_blob"], 23)):
        with ca.Genome.open([blob]) as g:
            off, rows = g.search_bulges_variants(NGG, queries, (0, 20), 3, 2, 2, mv)
            want_off, want_rows = g.search_bulges(NGG, queries, (0, 20), 3, 2, 2)
            assert off.tobytes() == want_off.tobytes() and len(rows) == len(want_rows) > 400
            assert rows.tobytes() == bvu.from_bulges(want_rows, 23).tobytes() and set(rows["bulge"].tolist()) == {-2, -1, 0, 1, 2}
            prof = g.search_bulges_variants_profile(NGG, queries, (0, 20), 3, 2, 2, mv)
            assert prof.tobytes() == g.search_bulges_profile(NGG, queries, (0, 20), 3, 2, 2).tobytes()


# ---- after SNPs ---------------------------------------------------------------------------------------------------------

def test_a_handle_with_snps_applied_equals_one_opened_from_the_coded_fasta(ngg_case):
    queries, want, cut = ngg_case["queries"], ngg_case["want"], ngg_case["cut"]
    snps, vcf = snps_between(cut(ngg_case["ref"]), cut(ngg_case["text"]))
    assert len(snps) > 80
    with ca.Genome.open([ngg_case["ref_blob"]]) as g:
        before = g.search_bulges(NGG, queries, (0, 20), 3, 2, 2)
        assert g.apply_snps(snps) == len(snps)
        check(None, NGG, queries, (0, 20), 3, 2, 2, 2, genome=g, want=want)
        # the plain bulge search on the same handle skips the coded windows: fewer rows than before, those of its model
        off, rows = g.search_bulges(NGG, queries, (0, 20), 3, 2, 2)
        m_off, m_rows, _ = bu.brute_force(ngg_case["records"], NGG, queries, (0, 20), 3, 2, 2)
        assert off.tobytes() == m_off.tobytes() and rows.tobytes() == m_rows.tobytes() and len(rows) < len(before[1])
    with ca.Genome.open([ngg_case["ref_blob"]]) as g:
        assert g.apply_vcf(vcf)["changed"] == len(snps)
        check(None, NGG, queries, (0, 20), 3, 2, 2, 2, genome=g, want=want)


# ---- the executable -----------------------------------------------------------------------------------------------------

def test_cli_prints_the_brute_force(tmp_path, ngg_case):
    records, cut = ngg_case["records"], ngg_case["cut"]
    queries = [q.lower() if k == 2 else q for k, q in enumerate(ngg_case["queries"])]
    fasta, ref_fasta, vcf_file, qfile = (tmp_path / n for n in ("genome.fa", "reference.fa", "snps.vcf", "queries.txt"))
    fasta.write_bytes(ngg_case["blob"])
    ref_fasta.write_bytes(ngg_case["ref_blob"])
    vcf_file.write_bytes(snps_between(cut(ngg_case["ref"]), cut(ngg_case["text"]))[1])
    qfile.write_text("\r\n".join(queries[:5]) + "\r\n" + "\n".join(queries[5:]) + "\n\n")
    _, want_rows, want_prof = bvu.brute_force(records, NGG, queries, (0, 20), 3, 1, 1, 2)
    assert (want_rows["n_var"] > 0).any() and set(want_rows["bulge"].tolist()) == {-1, 0, 1}
    options = ["--guide", "0:20", "--dna-bulge", "1", "--rna-bulge", "1", "--guide-variants", "2"]
    for more, genome in (([], fasta), (["--guide-vcf", str(vcf_file)], ref_fasta)):
        r = subprocess.run([EXE] + options + more + [NGG, str(qfile), "3", str(genome)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == bvu.format_rows(records, queries, want_rows, (0, 20))
        assert (b"vcf: lines" in r.stderr) == bool(more)
        r = subprocess.run([EXE, "--profile", NGG.lower(), str(qfile), "3"] + options + more + [str(genome)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == bvu.format_profile(queries, want_prof)
    # --guide-vcf alone: max_variants is the pattern's length
    _, all_rows, _ = bvu.brute_force(records, NGG, queries[:4], (0, 20), 1, 1, 1, 23)
    (tmp_path / "four.txt").write_text("\n".join(queries[:4]) + "\n")
    r = subprocess.run([EXE, "--guide", "0:20", "--guide-vcf", str(vcf_file), NGG, str(tmp_path / "four.txt"), "1", str(ref_fasta)],
                       capture_output=True)
    assert r.returncode == 0 and r.stdout == bvu.format_rows(records, queries[:4], all_rows, (0, 20)) and len(all_rows) > 10


# ---- tile edges ----------------------------------------------------------------------------------------------------------

EDGE_PATTERN, EDGE_SPAN = "N" * 10 + "GG", (0, 9)  # L = 12: windows of 9 to 15 codes


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("b", [-3, -2, -1, 0, 1, 2, 3])
def test_tile_edges(b, strand):
    """A site whose window of W = L + b codes starts at TILE - W + 1 (its last code is the halo's first), at TILE - 1, at TILE,
    and one that ends at the text's last base, with a code in the part beyond the tile's edge; texts of 4095, 4096, 4097 and
    2 x TILE + 1 bases, where the window that ends the text starts at 2 x TILE - W + 1."""
    rng = np.random.default_rng(100 + 10 * b + strand)
    L, W = 12, 12 + b
    D, R = max(b, 0), max(-b, 0)
    guide = random_text(rng, 9)
    i = 1 + int(rng.integers(0, 8 - R)) if b else 0
    site = bulged(guide, b, i, rng) + "TGG"
    assert len(site) == W
    cases = [(4095, None), (4096, None), (4097, None), (2 * TILE + 1, TILE - W + 1), (2 * TILE + 1, TILE - 1), (2 * TILE + 1, TILE)]
    for n, start in cases:
        text = list(random_text(rng, n))
        placed = [n - W] + ([start] if start is not None else [])
        for s in placed:
            # the code: at or behind the tile's edge where the window crosses one, else anywhere in it
            edge = (s // TILE + 1) * TILE
            lo = edge - s if s < edge < s + W and edge < n else 0
            p = lo + int(rng.integers(0, W - lo))
            plain = su.revcomp(site) if strand else site  # as the text holds it
            text[s:s + W] = plain[:p] + code_over(rng, plain[p]) + plain[p + 1:]
            assert not lo or s + p >= edge
        blob = fasta_of(["".join(text)])
        off, rows = check([blob], EDGE_PATTERN, [guide + "NNN", "N" * L], EDGE_SPAN, 1, D, R, 2)
        mine = bvu.as_tuples(rows[:int(off[1])], L)
        for s in placed:
            assert [r for r in mine if r[2] == s and r[3] == strand and r[5] == b and r[4] == 0 and r[7] == 1], (n, s, mine)


# ---- bad bytes, record ends, short genomes ---------------------------------------------------------------------------------

def test_bad_bytes_at_every_offset_record_ends_and_short_genomes():
    rng = np.random.default_rng(31)
    L = 12
    guide = random_text(rng, 9)
    sites = {3: bulged(guide, 3, 4, rng) + "CGG", -3: bulged(guide, -3, 2, rng) + "AGG"}
    assert len(sites[3]) == 15 and len(sites[-3]) == 9
    head, tail = "TTTTCTTTT", "TTTCTTTT"  # no PAM of either strand around the site
    seqs, clean, spoiled = [], {}, []
    for b, site in sites.items():
        coded = site[:1] + code_over(rng, site[1]) + site[2:]
        clean[b] = len(seqs)
        seqs.append(head + coded + tail)
        for p in range(len(site)):
            for bad in "N-":
                spoiled.append((len(seqs), b))
                seqs.append(head + coded[:p] + bad + coded[p + 1:] + tail)
        for keep in (len(site) - 1, len(site) // 2, 1):  # the record ends inside the window; the next one holds the rest
            spoiled.append((len(seqs), b))
            seqs.append(head + coded[:keep])
            spoiled.append((len(seqs), b))
            seqs.append(coded[keep:] + tail)
    off, rows = check([fasta_of(seqs)], EDGE_PATTERN, [guide + "NNN", "N" * L], EDGE_SPAN, 0, 3, 3, 2)
    mine = {(int(r["record"]), int(r["bulge"])) for r in rows[:int(off[1])] if r["pos"] == len(head) or r["record"] not in clean.values()}
    for b in sites:
        assert (clean[b], b) in mine
    assert not mine & set(spoiled)
    # genomes shorter than some or all of the seven window lengths (9 to 15 codes)
    whole = sites[3]
    for n in (0, 1, 8, 9, 10, 12, 14, 15):
        text = whole[15 - n:] if n else ""
        text = text[:-1] + code_over(rng, text[-1]) if n else text
        off, rows = check([fasta_of([text])], EDGE_PATTERN, [guide + "NNN", "N" * L], EDGE_SPAN, L, 3, 3, 2)
        assert set(rows["bulge"].tolist()) <= set(range(-3, n - L + 1)) and (len(rows) > 0) == (n >= 9)


# ---- strand 1 -----------------------------------------------------------------------------------------------------------

def test_strand_1_with_every_ambiguity_code():
    """Cas12a, TTTV ahead of the protospacer, sites planted on strand 1: every one of the ten codes once under a compared
    position and once under the pattern's V, with and without a bulge."""
    rng = np.random.default_rng(12)
    pattern, span = "TTTV" + "N" * 20, (4, 20)
    guide = random_text(rng, 20)
    text, expected = list("T" * 40), []
    for k, code in enumerate(AMBIGUOUS):
        for under_v in (False, True):
            b = (-1, 0, 1)[(k + under_v) % 3]
            i = 1 + (3 * k) % 17 if b else 0
            v = next(x for x in "ACG" if x in su.IUPAC[code]) if under_v else "ACG"[k % 3]
            site = "TTT" + v + bulged(guide, b, i, rng)
            base = su.IUPAC[code][k % len(su.IUPAC[code])]  # the base of the set the site takes
            p = 3 if under_v else 4 + (5 * k) % 10 + (12 if k % 2 else 0)
            if not under_v:
                site = site[:p] + base + site[p + 1:]
            query_site = site
            site = site[:p] + code + site[p + 1:]
            expected.append((len(text), b, query_site))
            text += list(revcomp(site)) + list("T" * 30)
    blob = fasta_of(["".join(text)])
    queries = ["NNNN" + guide, "N" * 24]
    off, rows = check([blob], pattern, queries, span, 2, 1, 1, 1)
    mine = bvu.as_tuples(rows[:int(off[1])], 24)
    for pos, b, _ in expected:
        assert [r for r in mine if r[2] == pos and r[3] == 1 and r[5] == b and r[4] <= 1 and r[7] == 1], (pos, b)
    assert {r[8][3] for r in mine if r[3] == 1} >= set(AMBIGUOUS) and len({c for r in mine if r[3] == 1 for c in r[8][4:]} & set(AMBIGUOUS)) == 10


# ---- limits --------------------------------------------------------------------------------------------------------------

def test_windows_of_32_codes():
    """L = 29 with D = 3: every bit of a plane in use, on random text with codes and on poly-A and poly-T stretches."""
    rng = np.random.default_rng(29)
    ref = list(random_text(rng, 2 * TILE // 3))
    ref[1000:1100] = "A" * 100
    ref[2000:2100] = "T" * 100
    text = sprinkle(rng, ref, 25)
    text[1050], text[2050] = "R", "Y"
    text = "".join(text)
    queries = ["T" * 29, "A" * 29, "T" * 28 + "C", "".join(ref[300:329]), su.revcomp("".join(ref[500:510] + ref[512:531]))]
    off, rows = check([fasta_of([text])], "N" * 29, queries, (0, 29), 2, 3, 0, 2)
    assert set(rows["bulge"].tolist()) == {0, 1, 2, 3} and int(rows["site"][rows["bulge"] == 3].max()) >= 1 << 31
    assert (rows["n_var"] == 2).any() and (rows["query"] == 3).any() and ((rows["query"] == 4) & (rows["bulge"] == 2)).any()


def test_a_span_inside_the_pattern_with_three_rna_bases():
    rng = np.random.default_rng(7)
    pattern, span = "NRN" + "N" * 12 + "NGGN", (3, 12)
    guide = random_text(rng, 12)
    ref = list(random_text(rng, 3000))
    for k, r in enumerate((0, 1, 2, 3, 3, 3)):
        site = "CAT" + bulged(guide, -r, 1 + 2 * k if r else 0, rng) + "TGGA"
        ref[200 + 400 * k:200 + 400 * k + len(site)] = site if k % 2 else su.revcomp(site)
    text = "".join(sprinkle(rng, ref, 20))
    queries = ["NNN" + guide + "NNNN", "N" * 19, "CNN" + mutate(rng, guide, 1) + "NNNA"]
    off, rows = check([fasta_of([text])], pattern, queries, span, 2, 0, 3, 2)
    assert set(rows["bulge"][:int(off[1])].tolist()) == {-3, -2, -1, 0} and (rows["n_var"][:int(off[1])] > 0).any()


@pytest.mark.parametrize("max_dist", [0, 12])
def test_max_dist_0_and_the_patterns_length(max_dist):
    rng = np.random.default_rng(max_dist)
    ref = list(random_text(rng, 400))
    guide = random_text(rng, 9)
    for k, b in enumerate((-2, -1, 0, 1, 2)):
        site = bulged(guide, b, 3 if b else 0, rng) + "AGG"
        ref[30 + 70 * k:30 + 70 * k + len(site)] = site if k % 2 else su.revcomp(site)
    text = sprinkle(rng, ref, 15)
    off, rows = check([fasta_of(["".join(text)])], EDGE_PATTERN, [guide + "NNN", "N" * 12, random_text(rng, 12)], EDGE_SPAN, max_dist, 2, 2, 2)
    assert set(rows["bulge"].tolist()) == {-2, -1, 0, 1, 2} and (rows["n_var"] > 0).any() and (int(rows["dist"].max()) > 6) == (max_dist > 0)


# ---- query counts and cutting ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def query_case():
    rng = np.random.default_rng(77)
    ref = list(random_text(rng, 3000))
    drawn = []
    for k in range(40):  # 40 guides, each with one bulged site in the text
        guide = random_text(rng, 20)
        b, i = [(1, 1 + k % 19), (-1, 1 + k % 18), (0, 0)][k % 3]
        site = bulged(guide, b, i, rng) + "NGG".replace("N", "ACGT"[k % 4])
        ref[60 + 72 * k:60 + 72 * k + len(site)] = site if k % 2 else su.revcomp(site)
        drawn.append(guide + "NNN")
    blob = fasta_of(["".join(sprinkle(rng, ref, 30))])
    records = lu.parse([blob])
    pool = [random_text(rng, 20) + "NNN" for _ in range(257 - 40 - 60 - 10)] + [mutate(rng, q[:20], 1) + "NNN" for q in drawn] + \
           [mutate(rng, q[:20], 2) + "NNN" for q in drawn[:20]] + drawn + drawn[:10]  # duplicated queries at the end
    assert len(pool) == 257
    want = bvu.brute_force(records, NGG, pool, (0, 20), 2, 1, 1, 2)
    return blob, pool, want


@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 65, 257])
def test_query_counts(query_case, n):
    blob, pool, want = query_case
    queries = pool[-n:]
    part = bvu.of_queries(want, len(pool) - n, n)
    with ca.Genome.open([blob]) as g:
        off, rows = check(None, NGG, queries, (0, 20), 2, 1, 1, 2, genome=g, want=part)
        assert len(rows) > 0 and (rows["n_var"] > 0).any()
        if n == 65:  # one call = the concatenation of n single-query calls
            parts = [g.search_bulges_variants(NGG, [q], (0, 20), 2, 1, 1, 2)[1] for q in queries]
            for k, p in enumerate(parts):
                p["query"] = k
            assert np.concatenate(parts).tobytes() == rows.tobytes() and {-1, 0, 1} == set(rows["bulge"].tolist())
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()


PIECE = 1 << 19  # BulgeVariantSearch::kPieceQueries: 19 bits of query in a hit word


def two_piece_case():
    """2^19 + 3 queries over a pool of 65 (query k is pool[k % 65]) against one record of 400 bases with codes, NGG, span
    (0, 20), max_dist 1, D = R = 1, max_variants 2.  The three queries of the second piece are pool[63], pool[64] and pool[0]
    (2^19 mod 65 = 63), read off forward sites of the record: a copy, a site of 21 bases less one base (a DNA bulge), and a
    site of 19 bases with one base put in (an RNA bulge).  -> (blob, pool, which, offsets, rows), the expected bytes being the
    pool's brute force, tiled.  No device needed."""
    rng = np.random.default_rng(5)
    ref = random_text(rng, 400)
    sites = [p for p in range(1, 400 - 23) if ref[p + 21:p + 23] == "GG"]
    a, b, c = (int(p) for p in rng.choice(sites, size=3, replace=False))
    text = list(ref)
    for p in (a + 5, b + 3, c + 12):
        text[p] = code_over(rng, ref[p])
    records = [(b"rec0 some text", "".join(text).encode())]
    pool = [random_text(rng, 20) + "NNN" for _ in range(65)]
    pool[63] = ref[a:a + 20] + "NNN"
    pool[64] = ref[b - 1:b + 8] + ref[b + 9:b + 20] + "NNN"
    pool[0] = ref[c + 1:c + 10] + "ACGT"[int(rng.integers(0, 4))] + ref[c + 10:c + 20] + "NNN"
    p_off, p_rows, _ = bvu.brute_force(records, NGG, pool, (0, 20), 1, 1, 1, 2)
    n = PIECE + 3
    which = np.arange(n) % 65
    counts = np.diff(p_off.astype(np.int64))[which]
    want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    has = np.flatnonzero(counts)
    want_rows = np.concatenate([p_rows[int(p_off[which[k]]):int(p_off[which[k] + 1])] for k in has])
    want_rows["query"] = np.repeat(has, counts[has])
    return fasta_of(["".join(text)]), pool, which, want_off, want_rows


def test_more_queries_than_a_piece_holds():
    """The two-piece path: the rows of the second piece are written behind the first piece's, to host memory and to device
    memory, and not at all when they do not fit."""
    import torch
    blob, pool, which, want_off, want_rows = two_piece_case()
    n, total = len(which), len(want_rows)
    second = want_rows[int(want_off[PIECE]):]
    assert which[PIECE] == 63 and set(second["bulge"].tolist()) >= {-1, 0, 1} and (second["n_var"] > 0).any()
    pat, pq = ca.search_prepare(NGG, pool)
    q = np.ascontiguousarray(pq[which])
    bg = _lib.SearchBulges(0, 20, 1, 1)
    with ca.Genome.open([blob]) as g:
        off, rows = g.search_bulges_variants(pat, q, (0, 20), 1, 1, 1, 2)
        assert off.tobytes() == want_off.tobytes() and rows.tobytes() == want_rows.tobytes()
        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        d_hits = torch.full((total * ROW,), 0xA5, dtype=torch.uint8, device="cuda")  # exactly n_total rows
        assert g.search_bulges_variants_device(pat, d_q, d_off, d_hits, (0, 20), 1, 1, 1, 2) == total
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        assert d_hits.cpu().numpy().tobytes() == want_rows.tobytes()
        poison = np.full(total * ROW, 0xA5, dtype=np.uint8)
        off = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint64)
        n_total = C.c_size_t()
        assert _lib.lib.issl_genome_search_bulges_variants(g._h, C.byref(pat), C.byref(bg), q.ctypes.data, n, 1, 2, off.ctypes.data,
                                                           poison.ctypes.data, total - 1, C.byref(n_total)) == 0
        assert n_total.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
