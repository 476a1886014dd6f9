"""GPU: issl_genome_search_variants*, issl_genome_apply_snps / _vcf and bin/isslSearchGenome --variants / --vcf against the
model of tests/variant_util.py, byte for byte: rows, offsets, profile."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import locate_util as lu
import search_util as su
import variant_util as vu

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslSearchGenome")
NGG = "N" * 21 + "GG"
TILE = 4096  # kPosPerBlock: text positions per workgroup; its planes are words of 32 positions
AMBIGUOUS = "RYSWKMBDHV"


def random_text(rng, n, codes="ACGT"):
    return "".join(codes[i] for i in rng.integers(0, len(codes), size=n))


def fasta_of(seqs):
    return b"".join(b">rec%d some text\n%s\n" % (k, s.encode()) for k, s in enumerate(seqs))


def check_search(blobs, pattern, queries, max_dist, max_variants, genome=None, records=None):
    """One search and one profile on the device equal the model, byte for byte.  -> (offsets, rows)"""
    want_off, want_rows, want_prof = vu.brute_force(records or lu.parse(blobs), pattern, queries, max_dist, max_variants)
    g = genome or ca.Genome.open(blobs)
    try:
        off, rows = g.search_variants(pattern, queries, max_dist, max_variants)
        prof = g.search_variants_profile(pattern, queries, max_dist, max_variants)
    finally:
        if genome is None:
            g.close()
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == ca.VARIANT_HIT_DTYPE and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    return off, rows


# ---- tile edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 23, 32])
@pytest.mark.parametrize("extra", ["4095", "4096", "4097", "4096+L-1", "8193"])
def test_tile_edges(L, extra):
    """Codes in the last L bases before and the first L after position 4096 -- the halo word and every cut of a window across
    two plane words -- and one as the very last base of the text."""
    n = {"4095": 4095, "4096": 4096, "4097": 4097, "4096+L-1": TILE + L - 1, "8193": 8193}[extra]
    rng = np.random.default_rng(n * 100 + L)
    text = list(random_text(rng, n))
    for i in range(TILE - L, min(n, TILE + L)):
        if rng.random() < (1.0 if L == 1 else 3.0 / L):
            text[i] = AMBIGUOUS[int(rng.integers(0, 10))]
    for i in (31, 32, 63, 64, TILE - 1, TILE):  # the borders of plane words
        if i < n:
            text[i] = AMBIGUOUS[int(rng.integers(0, 10))]
    text[n - 1] = "R"
    text = "".join(text)
    queries = ["N" * L, "A" * L, text[TILE - L:TILE].translate(str.maketrans(AMBIGUOUS, "ACCAGAGAAA")) if n >= TILE else "C" * L,
               random_text(rng, L)]
    off, rows = check_search([fasta_of([text])], "N" * L, queries, min(L, 2), L)
    every = rows[:int(off[1])]
    assert len(every) == 2 * (n - L + 1) and int(every["pos"].max()) == n - L and int(every["n_var"].max()) >= 1
    assert (every["n_var"][every["pos"] == n - L] >= 1).all()
    if L > 1:
        check_search([fasta_of([text])], ("N" * L + "RG")[-L:], queries, 2, 2)


# ---- records ------------------------------------------------------------------------------------------------------------

def test_records_short_empty_n_runs_and_lower_case():
    rng = np.random.default_rng(8)
    a, b = random_text(rng, 40), random_text(rng, 30)
    seqs = ["ACRT", "", a[:20] + "R" + a[21:], "ACGTRYS", b[:10] + "NNNNNNNN" + b[18:], "acgtryswkmbdhvacgt", "AC-GU.RY*"]
    blob = fasta_of(seqs)
    across = a[33:40] + "ACG"   # would lie across records 2 | 3
    queries = ["N" * 10, across, a[15:25], su.revcomp(a[15:25]), b[5:15], "ACGTACGTAC"]
    off, rows = check_search([blob], "N" * 10, queries, 1, 10)
    every = rows[:int(off[1])]
    assert set(every["record"].tolist()) == {2, 4, 5} and int(off[2]) == int(off[1])
    assert len(every) == 2 * (31 + 1 + 3 + 9)  # record 4: one window ahead of the N run, 3 behind it
    assert int(off[3]) - int(off[2]) >= 1 and int(off[4]) - int(off[3]) >= 1
    for blob in (b"", b">only\n", b">a\nACGTRYS\n"):
        check_search([blob], "N" * 8, ["N" * 8], 0, 8)
    with ca.Genome.open([b">a\nACGTRYSW\n"]) as g:
        off, rows = g.search_variants("NNNNNNNN", [], 2, 2)  # n == 0
        assert off.tolist() == [0] and len(rows) == 0 and g.search_variants_profile("NNNNNNNN", [], 2, 2).shape == (0, 3)


# ---- strand 1 -----------------------------------------------------------------------------------------------------------

def test_strand_1_every_code_and_a_pam_only_an_alt_allele_gives():
    codes = vu.TEXT_CODES
    text = "".join(c + "ACGT"[k % 4] for k, c in enumerate(codes))  # every code, a base between two
    off, rows = check_search([fasta_of([text])], "N", ["N", "A", "C", "G", "T"], 0, 1)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
            "D": "H", "H": "D"}
    every = vu.as_tuples(rows[:int(off[1])], 1)
    for k, c in enumerate(codes):
        assert (0, 0, 2 * k, 0, 0, int(c in AMBIGUOUS), c) in every and (0, 0, 2 * k, 1, 0, int(c in AMBIGUOUS), comp[c]) in every
    check_search([fasta_of([text])], "NNN", ["NNN", "ACG", "TNA"], 1, 2)
    check_search([fasta_of([text])], "SWN", ["NNN", "CAG"], 1, 3)
    # CCN ahead of a protospacer is NGG on strand 1.  The reference reads CTA: no PAM.  With the SNP T>C the text is CYA,
    # strand 1 reads T R G ... and NGG is reachable only through the ALT allele
    rng = np.random.default_rng(12)
    guide = random_text(rng, 20)
    pam_text = "TTTT" + "CYA" + su.revcomp(guide) + "TTTT"
    ref_text = "TTTT" + "CTA" + su.revcomp(guide) + "TTTT"
    query = guide + "NNN"
    assert len(vu.brute_force([(b"r", ref_text.encode())], NGG, [query], 0, 23)[1]) == 0
    off, rows = check_search([fasta_of([pam_text])], NGG, [query, "N" * 23], 0, 1)
    assert vu.as_tuples(rows[:int(off[1])], 23) == [(0, 0, 4, 1, 0, 1, guide + "TRG")]
    assert len(check_search([fasta_of([pam_text])], NGG, [query], 0, 0)[1]) == 0


# ---- pattern and query on the same position ---------------------------------------------------------------------------

def test_a_restricted_position_that_is_also_compared():
    rng = np.random.default_rng(3)
    text = list(random_text(rng, 3000))
    for i in range(10, 3000, 9):
        text[i] = AMBIGUOUS[int(rng.integers(0, 10))]
    text = "".join(text)
    # the text's R holds the query's A, the pattern's G forbids it: a mismatch, not a match
    off, rows = check_search([b">r\nCRT\n"], "NGN", ["NAN", "NGN"], 1, 1)
    assert vu.as_tuples(rows, 3)[0] == (0, 0, 0, 0, 1, 1, "CrT") and (1, 0, 0, 0, 0, 1, "CRT") in vu.as_tuples(rows, 3)
    pattern = "NNRNNNNSNNNNGG"
    records = lu.parse([fasta_of([text])])
    _, pos, strand, _, t, _ = vu.candidates(records, pattern, 3)
    assert len(t) > 60
    drawn = []
    for i in rng.choice(len(t), size=20, replace=False):  # a base of every set, the pattern's restriction ignored
        drawn.append("".join("ACGT"[[b for b in range(4) if int(s) >> b & 1][int(rng.integers(0, bin(int(s)).count("1")))]] for s in t[i]))
    off, rows = check_search([fasta_of([text])], pattern, drawn + ["N" * 14], 2, 3)
    assert (rows["dist"] > 0).any() and (rows["n_var"] > 1).any()


# ---- max_variants --------------------------------------------------------------------------------------------------------

def test_max_variants_0_1_2_and_length():
    rng = np.random.default_rng(21)
    L = 12
    text = list(random_text(rng, 5000))
    for at, k in ((100, 1), (300, 2), (500, 3), (700, 4), (4090, 2), (4100, 3)):  # k codes next to each other
        text[at:at + k] = [AMBIGUOUS[int(rng.integers(0, 10))] for _ in range(k)]
    for i in rng.choice(5000, size=120, replace=False):
        text[i] = AMBIGUOUS[int(rng.integers(0, 10))]
    text = "".join(text)
    blob = fasta_of([text])
    queries = ["N" * L, random_text(rng, L), text[295:307].translate(str.maketrans(AMBIGUOUS, "ACCAGAGAAA"))]
    with ca.Genome.open([blob]) as g:
        seen = {}
        for mv in (0, 1, 2, L):
            off, rows = check_search([blob], "N" * L, queries, 3, mv, genome=g)
            every = rows[:int(off[1])]
            assert (every["n_var"] <= mv).all() and (mv in (0, L) or (every["n_var"] == mv).any())  # exactly mv is in, mv + 1 is out
            seen[mv] = len(every)
        assert int(every["n_var"].max()) >= 4
        assert seen[0] < seen[1] < seen[2] < seen[L] == 2 * (5000 - L + 1)


# ---- query counts --------------------------------------------------------------------------------------------------------

def variant_case(seed, n_bases, every, n_queries):
    """A REF text, SNPs at about one base in `every`, the text with them applied, and queries drawn from the windows NGG
    admits there, spelled with the ALT alleles, some mutated; one named twice and one all-N."""
    rng = np.random.default_rng(seed)
    ref = random_text(rng, n_bases)
    places = np.flatnonzero(rng.random(n_bases) < 1.0 / every)
    snps = np.zeros(len(places), dtype=ca.SNP_DTYPE)
    snps["pos"], snps["record"] = places % (n_bases // 2), places // (n_bases // 2)
    for k, p in enumerate(places):
        r = "ACGT".index(ref[p])
        snps["ref"][k] = 1 << r
        snps["alt"][k] = 1 << ((r + 1 + int(rng.integers(0, 3))) % 4)
    ref_records = [(b"rec0 some text", ref[:n_bases // 2].encode()), (b"rec1 some text", ref[n_bases // 2:].encode())]
    records, _ = vu.apply_snps(ref_records, snps)
    _, _, _, n_var, t, _ = vu.candidates(records, NGG, 2)
    with_alt = np.flatnonzero(n_var > 0)
    queries = []
    for i in rng.choice(with_alt, size=n_queries - 2, replace=False):
        q = ""
        for s in t[i][:20]:
            bases = [b for b in range(4) if int(s) >> b & 1]
            q += "ACGT"[bases[int(rng.integers(0, len(bases)))]]
        if len(queries) % 3 == 2:
            at = int(rng.integers(0, 20))
            q = q[:at] + "ACGT"[("ACGT".index(q[at]) + 1) % 4] + q[at + 1:]
        queries.append(q + "NNN")
    queries += [queries[0], "N" * 23]
    blob = b"".join(b">%s\n%s\n" % (name, seq) for name, seq in ref_records)
    return blob, ref_records, snps, records, queries


@pytest.fixture(scope="module")
def main_case():
    blob, ref_records, snps, records, queries = variant_case(7, 12000, 30, 70)
    want = vu.brute_force(records, NGG, queries, 2, 2)
    return blob, ref_records, snps, records, queries, want


def test_the_main_case_is_not_vacuous(main_case):
    blob, ref_records, snps, records, queries, (off, rows, prof) = main_case
    assert (rows["n_var"] > 0).sum() >= 50
    _, ref_rows, _ = vu.brute_force(ref_records, NGG, queries, 2, 2)
    key = lambda r: {(int(x["query"]), int(x["record"]), int(x["pos"]), int(x["strand"])) for x in r}
    assert len(key(rows) - key(ref_rows)) >= 10  # rows that exist only because of an ALT allele


@pytest.mark.parametrize("n", [1, 3, 4, 9, 70])
@pytest.mark.parametrize("max_dist", [0, 2, 23])
def test_query_counts(main_case, n, max_dist):
    blob, ref_records, snps, records, queries, _ = main_case
    mine = queries[-n:]  # the all-N query, the one named twice, ...
    if max_dist == 23:
        records = [(name, seq[:300]) for name, seq in records]  # every window-strand hits every query
        ref_records = [(name, seq[:300]) for name, seq in ref_records]
        snps = snps[snps["pos"] < 300]
        blob = b"".join(b">%s\n%s\n" % (name, seq) for name, seq in ref_records)
    with ca.Genome.open([blob]) as g:
        assert g.apply_snps(snps) == len(snps)
        off, rows = check_search(None, NGG, mine, max_dist, 2, genome=g, records=records)
        off2, rows2 = g.search_variants(NGG, mine, max_dist, 2)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs
        assert len(rows) > 0
        if n == 70 and max_dist == 2:
            first = rows[int(off[0]):int(off[1])].copy()   # the query named twice gets the same list twice
            again = rows[int(off[68]):int(off[69])].copy()
            first["query"] = again["query"] = 0
            assert first.tobytes() == again.tobytes() and len(first) > 0


# ---- the two identities -------------------------------------------------------------------------------------------------

def test_the_identities_with_the_plain_search(main_case):
    blob, ref_records, snps, records, queries, _ = main_case
    with ca.Genome.open([blob]) as g:
        off, rows = g.search(NGG, queries, 3)
        prof = g.search_profile(NGG, queries, 3)
        assert len(rows) > 100
        for mv in (0, 1, 23):  # a text without codes: any max_variants
            v_off, v_rows = g.search_variants(NGG, queries, 3, mv)
            assert v_off.tobytes() == off.tobytes() and v_rows.tobytes() == vu.from_plain(rows, 23).tobytes()
            assert g.search_variants_profile(NGG, queries, 3, mv).tobytes() == prof.tobytes()
        g.apply_snps(snps)
        off, rows = g.search(NGG, queries, 3)  # a text with codes: the plain search skips their windows, as max_variants = 0 does
        v_off, v_rows = g.search_variants(NGG, queries, 3, 0)
        assert 100 < len(rows) and v_off.tobytes() == off.tobytes() and v_rows.tobytes() == vu.from_plain(rows, 23).tobytes()
        assert g.search_variants_profile(NGG, queries, 3, 0).tobytes() == g.search_profile(NGG, queries, 3).tobytes()
        assert len(g.search_variants(NGG, queries, 3, 2)[1]) > len(rows)


# ---- capacity, device entry points ------------------------------------------------------------------------------------

def test_capacity_and_device_entry_points(main_case):
    import torch
    blob, ref_records, snps, records, queries, (want_off, want_rows, want_prof) = main_case
    pat, q = ca.search_prepare(NGG, queries)
    total = len(want_rows)
    with ca.Genome.open([blob]) as g:
        g.apply_snps(snps)
        poison = np.full(total * 40, 0xA5, dtype=np.uint8)
        off = np.full(len(queries) + 1, 0xFFFFFFFF, dtype=np.uint64)
        n = C.c_size_t()
        args = (g._h, C.byref(pat), q.ctypes.data, len(q), 2, 2, off.ctypes.data, poison.ctypes.data)
        assert _lib.lib.issl_genome_search_variants(*args, total - 1, C.byref(n)) == 0
        assert n.value == total and off.tobytes() == want_off.tobytes() and (poison == 0xA5).all()  # one below: nothing is written
        assert _lib.lib.issl_genome_search_variants(*args, total, C.byref(n)) == 0 and poison.tobytes() == want_rows.tobytes()

        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda")
        assert g.search_variants_device(pat, d_q, d_off, None, 2, 2) == total  # the counting call
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * 40,), 0xA5, dtype=torch.uint8, device="cuda")
        assert g.search_variants_device(pat, d_q, d_off, d_hits[:(total - 1) * 40], 2, 2) == total
        assert bool((d_hits == 0xA5).all())
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_variants_device(NGG, d_q, d_off, d_hits, 2, 2, stream=stream.cuda_stream) == total
        assert d_hits.cpu().numpy().view(ca.VARIANT_HIT_DTYPE).tobytes() == want_rows.tobytes()
        d_counts = torch.full((len(queries) * 3,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        g.search_variants_profile_device(pat, d_q, d_counts, 2, 2, stream=stream.cuda_stream)
        assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes()
        assert g.search_variants_device(pat, d_q[:0], d_off[:1], None, 2, 2) == 0 and int(d_off[0]) == 0  # n == 0


# ---- SNPs onto the text ------------------------------------------------------------------------------------------------

def read_back(g, n_records):
    """The resident text as the search shows it: the strand-0 rows of the all-N one-base query with max_variants = L."""
    off, rows = g.search_variants("N", ["N"], 0, 1)
    rows = rows[rows["strand"] == 0]
    out = [dict() for _ in range(n_records)]
    for r in rows:
        out[int(r["record"])][int(r["pos"])] = vu.site_text(r["site"], 1)
    return out


def same_text(g, records):
    got = read_back(g, len(records))
    for r, (_, seq) in enumerate(records):
        assert got[r] == {i: chr(c) for i, c in enumerate(seq) if chr(c) in vu.TEXT_CODES}, r


def test_apply_snps_and_apply_vcf(main_case, tmp_path):
    blob, ref_records, snps, records, queries, _ = main_case
    with ca.Genome.open([blob]) as g:
        same_text(g, ref_records)
        assert g.apply_snps(snps) == len(snps)
        same_text(g, records)
        assert g.apply_snps(snps) == 0  # a second application changes nothing
        same_text(g, records)
    # two SNPs at one place merge; a code that is there already takes another allele
    small = [(b"a", b"ACGTNACGT"), (b"b x", b"ACRT")]
    blob = b">a\nACGTNACGT\n>b x\nacrt\n"
    snp = lambda pos, record, ref, alt: (pos, record, 1 << "ACGT".index(ref), sum(1 << "ACGT".index(b) for b in alt), (0, 0))
    with ca.Genome.open([blob]) as g:
        merged = np.array([snp(1, 0, "C", "T"), snp(8, 0, "T", "A"), snp(1, 0, "C", "G"), snp(2, 1, "G", "C")], dtype=ca.SNP_DTYPE)
        after, changed = vu.apply_snps(small, merged)
        assert after[0][1] == b"ABGTNACGW" and after[1][1] == b"ACVT" and changed == 3
        assert g.apply_snps(merged) == 3
        same_text(g, after)
        # refusals name the smallest failing input index and leave the text as it was
        for bad, index in (([snp(0, 0, "A", "C"), snp(2, 0, "T", "C"), snp(3, 0, "G", "C")], 1),   # REF disagrees with the text
                           ([snp(0, 0, "A", "C"), snp(4, 0, "A", "C")], 1),                         # the place is N
                           ([snp(0, 0, "A", "C"), snp(9, 0, "A", "C")], 1),                         # outside the record
                           ([snp(0, 0, "A", "C"), snp(0, 2, "A", "C")], 1),                         # no such record
                           ([snp(3, 0, "T", "C"), snp(0, 0, "A", "C"), snp(0, 0, "C", "G")], 2),    # two REFs at one place
                           ([snp(1, 0, "C", "A")], 0),                                              # B and A: all four bases
                           ([(0, 0, 3, 1, (0, 0))], 0), ([(0, 0, 1, 0, (0, 0))], 0), ([(0, 0, 1, 16, (0, 0))], 0)):
            with pytest.raises(vu.Refused) as m:
                vu.apply_snps(after, np.array(bad, dtype=ca.SNP_DTYPE))
            assert m.value.index == index
            with pytest.raises(ca.IsslError) as e:
                g.apply_snps(np.array(bad, dtype=ca.SNP_DTYPE))
            assert e.value.code == -1 and ("snp %d:" % index) in e.value.message, e.value.message
            same_text(g, after)
        assert g.apply_snps(np.zeros(0, dtype=ca.SNP_DTYPE)) == 0
    # a VCF: bytes and a path
    vcf = b"#CHROM\tPOS\tID\tREF\tALT\na\t2\t.\tC\tT,G\nb\t3\t.\tg\tc,<DEL>\nb\t9\t.\tA\tC\nc\t1\t.\tA\tC\na\t9\t.\tT\tA\r\na\t4\t.\tTN\tT\n"
    want_snps, want_counts = vu.vcf_snps(vcf, small)
    after, changed = vu.apply_snps(small, want_snps)
    assert changed == 3 and want_counts["alleles_skipped"] == 2
    path = tmp_path / "small.vcf"
    path.write_bytes(vcf)
    for source in (vcf, path):
        with ca.Genome.open([blob]) as g:
            assert g.apply_vcf(source) == dict(want_counts, changed=3)
            same_text(g, after)
            assert g.apply_vcf(source)["changed"] == 0
            with pytest.raises(ca.IsslError) as e:
                g.apply_vcf(b"a\t1\t.\tC\tT\n")  # REF is A
            assert "snp 0:" in e.value.message
            with pytest.raises(ca.IsslError) as e:
                g.apply_vcf(b"a\t1\t.\tA\tT\na\t1\n")
            assert "line 2:" in e.value.message
            same_text(g, after)


# ---- the executable ------------------------------------------------------------------------------------------------------

def test_cli_prints_the_model(tmp_path, main_case):
    blob, ref_records, snps, records, queries, _ = main_case
    queries = queries[:20] + ["n" * 23]
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(blob)
    coded = tmp_path / "coded.fa"
    coded.write_bytes(b"".join(b">%s\n%s\n" % (name, seq) for name, seq in records))
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\r\n".join(queries[:10]) + "\r\n" + "\n".join(queries[10:]) + "\n\n")
    vcf = tmp_path / "snps.vcf"
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT"]
    for s in snps:
        lines.append(b"rec%d\t%d\t.\t%s\t%s,<DEL>" % (s["record"], s["pos"] + 1, b"ACGT"[int(s["ref"]).bit_length() - 1:][:1],
                                                   b"ACGT"[int(s["alt"]).bit_length() - 1:][:1]))
    lines.append(b"chrUn\t5\t.\tA\tC")
    vcf.write_bytes(b"\n".join(lines) + b"\n")
    for mv in (2, 23):
        want_off, want_rows, want_prof = vu.brute_force(records, NGG, queries, 2, mv)
        assert len(want_rows) > 500
        options = ["--vcf", str(vcf)] + (["--variants", str(mv)] if mv != 23 else [])  # --vcf alone implies --variants L
        r = subprocess.run([EXE] + options + [NGG, str(qfile), "2", str(fasta)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == vu.format_rows(records, queries, want_rows)
        assert r.stderr.count(b"\n") == 1 and (b"vcf: lines %d snps %d alleles_skipped %d no_allele 0 unknown_chrom 1 beyond_record 0 changed %d\n"
                                               % (len(snps) + 1, len(snps), len(snps), len(snps))) == r.stderr
        r = subprocess.run([EXE, "--profile"] + options + [NGG.lower(), str(qfile), "2", str(fasta)], capture_output=True)
        assert r.returncode == 0 and r.stdout == vu.format_profile(queries, want_prof), r.stderr
        r = subprocess.run([EXE, "--variants", str(mv), NGG, str(qfile), "2", str(coded)], capture_output=True)  # an IUPAC FASTA
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == vu.format_rows(records, queries, want_rows)
    assert any(line.split("\t")[5] != line.split("\t")[5].upper() for line in vu.format_rows(records, queries, want_rows).decode().splitlines())
