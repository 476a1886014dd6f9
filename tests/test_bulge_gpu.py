"""GPU: issl_genome_search_bulges* against the brute force of tests/bulge_util.py (a loop around the mismatch search's
brute force, pinned on the CPU by test_bulge_model.py): rows, offsets and profile byte for byte."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import bulge_util as bu
import locate_util as lu
import search_util as su

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslSearchGenome")
NGG = "N" * 21 + "GG"
TILE = 4096  # kPosPerBlock: text positions per workgroup
GROUP = 4    # kQueryGroup: queries whose bounds share one branch; what is left behind the last whole group goes one by one


def random_text(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


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


def check_bulges(blobs, pattern, queries, span, max_dist, D, R, genome=None, want=None):
    """One search and one profile on the device equal the brute force, byte for byte.  -> (offsets, rows)"""
    want_off, want_rows, want_prof = want or bu.brute_force_fasta(blobs, pattern, queries, span, max_dist, D, R)
    g = genome or ca.Genome.open(blobs)
    try:
        off, rows = g.search_bulges(pattern, queries, span, max_dist, D, R)
        prof = g.search_bulges_profile(pattern, queries, span, max_dist, D, R)
    finally:
        if genome is None:
            g.close()
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == ca.BULGE_HIT_DTYPE and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    counted = np.zeros_like(prof)  # the profile is the rows counted by (bulge, dist)
    np.add.at(counted, (rows["query"], rows["bulge"].astype(np.int64) + R, rows["dist"]), 1)
    assert np.array_equal(counted, prof)
    return off, rows


# ---- NGG: every class of row on both strands ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ngg_case():
    """L = 23, span (0, 20), D = R = 2, max_dist 3 on 8 000 bases: planted sites of every b in -2..2 on both strands with break
    points 1, G - 1 and G - 1 - r, a homopolymer tie, 12 random queries, one all-N query and one query named twice."""
    rng = np.random.default_rng(2024)
    G = 20
    text = list(random_text(rng, 8000))
    guides = [random_text(rng, G) for _ in range(3)]
    run = random_text(rng, 8) + "AAAA" + random_text(rng, 8)  # a DNA bulge of A inside the run ties between break points
    at = 100
    plants = []
    for k, guide in enumerate(guides):
        plants.append(guide + "TGG")
        for b in (-2, -1, 1, 2):
            for i in (1, 7 + k, G - 1 - max(-b, 0)):
                site = bulged(guide, b, i, rng)
                plants.append((mutate(rng, site, 1) if (i + k) % 2 else site) + "AGG")
    plants.append(run[:10] + "A" + run[10:] + "CGG")
    plants.append(run[:9] + run[10:] + "CGG")
    for k, site in enumerate(plants):
        s = site if k % 2 == 0 else su.revcomp(site)
        text[at:at + len(s)] = s
        at += 180
    assert at < 7900
    text = "".join(text)
    blob = fasta_of([text[:5000], text[5000:]])
    records = lu.parse([blob])
    queries = [g + "NNN" for g in guides] + [run + "NNN"] + [random_text(rng, G) + "NNN" for _ in range(12)] + ["N" * 23, guides[1] + "NNN"]
    ties = []
    want = bu.brute_force(records, NGG, queries, (0, G), 3, 2, 2, ties=ties)
    return blob, records, queries, want, ties


def test_the_brute_force_covers_every_class(ngg_case):
    """Asserted on the brute force alone, so that a failure cannot hide behind an agreement of two empty lists."""
    _, _, queries, (offsets, rows, profile), ties = ngg_case
    planted = rows[rows["query"] < 4]
    for strand in (0, 1):
        assert set(planted["bulge"][planted["strand"] == strand].tolist()) == {-2, -1, 0, 1, 2}
    assert ((planted["bulge"] != 0) & (planted["dist"] > 0)).any()
    for b, last in ((1, 19), (2, 19), (-1, 18), (-2, 17)):
        seen = set(planted["at"][planted["bulge"] == b].tolist())
        assert 1 in seen and last in seen and seen - {1, last}, (b, seen)
    assert ties and any(k[0] == 3 for k in ties)
    assert (np.diff(offsets.astype(np.int64))[:4] > 0).all() and int(offsets[-2] - offsets[-3]) > 1000  # the all-N query
    a, b = rows[int(offsets[1]):int(offsets[2])].copy(), rows[int(offsets[-2]):].copy()  # the query named twice
    a["query"] = b["query"] = 0
    assert len(a) and a.tobytes() == b.tobytes()


def test_ngg_every_bulge_on_both_strands(ngg_case):
    blob, _, queries, want, _ = ngg_case
    with ca.Genome.open([blob]) as g:
        off, rows = check_bulges([blob], NGG, queries, (0, 20), 3, 2, 2, genome=g, want=want)
        off2, rows2 = g.search_bulges(NGG, queries, (0, 20), 3, 2, 2)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs


def test_without_bulges_the_rows_of_the_mismatch_search(ngg_case):
    blob, _, queries, _, _ = ngg_case
    with ca.Genome.open([blob]) as g:
        for pattern, span in ((NGG, (0, 20)), ("NNRNNNNNNNNNNNNNNNNNNGG", (0, 23))):  # any code inside the span
            off, rows = g.search_bulges(pattern, queries, span, 3, 0, 0)
            want_off, want_rows = g.search(pattern, queries, 3)
            assert off.tobytes() == want_off.tobytes() and len(rows) == len(want_rows) > 400
            for f in ("site", "pos", "record", "query", "mism", "strand", "dist"):
                assert np.array_equal(rows[f], want_rows[f]), f
            assert not rows["bulge"].any() and not rows["at"].any()
            assert rows.tobytes() == want_rows.tobytes()  # bulge and at lie where the reserved bytes do
            prof = g.search_bulges_profile(pattern, queries, span, 3, 0, 0)
            assert prof.shape == (len(queries), 1, 4) and np.array_equal(prof[:, 0], g.search_profile(pattern, queries, 3))


def test_capacity_rule(ngg_case):
    blob, _, queries, (want_off, want_rows, _), _ = ngg_case
    pat, q = ca.search_prepare(NGG, queries)
    bg = _lib.SearchBulges(0, 20, 2, 2)
    total = len(want_rows)
    with ca.Genome.open([blob]) as g:
        poison = np.full(total * 32, 0xA5, dtype=np.uint8)
        off = np.full(len(queries) + 1, 0xFFFFFFFF, dtype=np.uint64)
        n = C.c_size_t()
        args = (g._h, C.byref(pat), C.byref(bg), q.ctypes.data, len(queries), 3, off.ctypes.data, poison.ctypes.data)
        assert _lib.lib.issl_genome_search_bulges(*args, total - 1, C.byref(n)) == 0
        assert n.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
        assert _lib.lib.issl_genome_search_bulges(*args, total, C.byref(n)) == 0 and poison.tobytes() == want_rows.tobytes()
        off, rows = g.search_bulges(NGG, [], (0, 20), 3, 2, 2)  # n == 0
        assert off.tolist() == [0] and len(rows) == 0 and g.search_bulges_profile(NGG, [], (0, 20), 3, 2, 2).shape == (0, 5, 4)


def test_device_entry_points_on_a_stream(ngg_case):
    import torch
    blob, _, queries, (want_off, want_rows, want_prof), _ = ngg_case
    pat, q = ca.search_prepare(NGG, queries)
    d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_off = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda")
    with ca.Genome.open([blob]) as g:
        total = g.search_bulges_device(pat, d_q, d_off, None, (0, 20), 3, 2, 2)  # the counting call
        assert total == len(want_rows) and d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert g.search_bulges_device(pat, d_q, d_off, d_hits[:(total - 1) * 32], (0, 20), 3, 2, 2) == total
        assert bool((d_hits == 0xA5).all())  # they do not fit: nothing is written
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_bulges_device(NGG, d_q, d_off, d_hits, (0, 20), 3, 2, 2, stream=stream.cuda_stream) == total
        assert d_hits.cpu().numpy().view(ca.BULGE_HIT_DTYPE).tobytes() == want_rows.tobytes()
        d_counts = torch.full((want_prof.size,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        g.search_bulges_profile_device(pat, d_q, d_counts, (0, 20), 3, 2, 2, stream=stream.cuda_stream)
        assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes()
        with pytest.raises(ValueError):
            g.search_bulges_profile_device(pat, d_q, d_counts[:-1], (0, 20), 3, 2, 2)
        assert g.search_bulges_device(pat, d_q[:0], d_off[:1], None, (0, 20), 3, 2, 2) == 0 and int(d_off[0]) == 0  # n == 0


def test_cli_prints_the_brute_force(tmp_path, ngg_case):
    blob, records, queries, want, _ = ngg_case
    queries = [q.lower() if k == 2 else q for k, q in enumerate(queries)]
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(blob)
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\r\n".join(queries[:5]) + "\r\n" + "\n".join(queries[5:]) + "\n\n")
    _, want_rows, want_prof = want
    options = ["--guide", "0:20", "--dna-bulge", "2", "--rna-bulge", "2"]
    r = subprocess.run([EXE] + options + [NGG, str(qfile), "3", str(fasta)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == bu.format_rows(records, queries, want_rows, (0, 20))
    r = subprocess.run([EXE, "--profile", NGG.lower(), str(qfile), "3"] + options + [str(fasta)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == bu.format_profile(queries, want_prof)
    # --guide alone: one base of either kind
    one = bu.brute_force(records, NGG, queries[:4], (0, 20), 1, 1, 1)
    (tmp_path / "four.txt").write_text("\n".join(queries[:4]) + "\n")
    r = subprocess.run([EXE, "--guide", "0:20", NGG, str(tmp_path / "four.txt"), "1", str(fasta)], capture_output=True)
    assert r.returncode == 0 and r.stdout == bu.format_rows(records, queries[:4], one[1], (0, 20)) and len(one[1]) > 10


# ---- tile edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,start,at,strand", [(TILE + 1, TILE + 1 - 25, 10, 1), (TILE + 23 + 1, TILE - 10, 5, 0),
                                               (TILE + 23 + 1, TILE - 6, 10, 0), (TILE + 23 + 1, TILE - 1, 3, 1)])
def test_tile_edges(n, start, at, strand):
    """Windows of L + 2 bases whose break point lies on either side of text position 4096 (the second case: 4096 - 10 + 5, the
    third: 4096 - 6 + 10), and windows that end at the record's last base (the first and the last case, read on strand 1),
    on texts of 4097 and 4096 + L + 1 bases."""
    rng = np.random.default_rng(n + start)
    guide = random_text(rng, 20)
    site = bulged(guide, 2, at, rng) + "TGG"
    assert len(site) == 25 and start < TILE < start + 25 <= n
    text = list(random_text(rng, n))
    text[start:start + 25] = site if strand == 0 else su.revcomp(site)
    short = bulged(guide, -2, 9, rng) + "AGG"  # and an RNA-bulged site at the text's start
    text[0:21] = short
    blob = fasta_of(["".join(text)])
    off, rows = check_bulges([blob], NGG, [guide + "NNN", "N" * 23], (0, 20), 1, 2, 2)
    mine = bu.as_tuples(rows[:int(off[1])], 23)
    # in query coordinates on strand 1 too: the break point is counted from the site's own start
    assert [r for r in mine if r[2] == start and r[3] == strand and r[5] == 2 and r[4] == 0 and r[7] == site]
    assert [r for r in mine if r[2] == 0 and r[3] == 0 and r[5] == -2 and r[4] == 0 and r[7] == short]


# ---- every bit of a packed word ------------------------------------------------------------------------------------------

def test_every_bit_in_use():
    """L = 29 with D = 3: windows of 32 bases on poly-A and poly-T stretches."""
    rng = np.random.default_rng(29)
    text = list(random_text(rng, 6000))
    text[3000:3100] = "A" * 100
    text[4090:4190] = "T" * 100  # across the tile edge
    blob = fasta_of(["".join(text)])
    off, rows = check_bulges([blob], "N" * 29, ["T" * 29, "A" * 29, "T" * 28 + "C", "C" + "A" * 28], (0, 29), 1, 3, 0)
    assert set(rows["bulge"].tolist()) == {0, 1, 2, 3} and int(rows["site"].max()) == (1 << 64) - 1


# ---- other nucleases -------------------------------------------------------------------------------------------------------

def test_cas12a_five_prime_pam():
    rng = np.random.default_rng(12)
    text = list(random_text(rng, 6000))
    guide = random_text(rng, 20)
    for k, (b, i) in enumerate([(0, 0), (1, 1), (1, 19), (-1, 1), (-1, 18), (1, 9), (-1, 10)]):
        site = "TTT" + "ACG"[k % 3] + bulged(guide, b, i, rng)
        text[300 + 700 * k:300 + 700 * k + len(site)] = site if k % 2 == 0 else su.revcomp(site)
    blob = fasta_of(["".join(text)])
    queries = ["NNNN" + guide, "NNNN" + mutate(rng, guide, 2), "N" * 24, "NNNN" + random_text(rng, 20)]
    off, rows = check_bulges([blob], "TTTV" + "N" * 20, queries, (4, 20), 2, 1, 1)
    mine = rows[:int(off[1])]
    # (a planted break point whose neighbour gives the same distance is reported as the smaller of the two)
    assert set(mine["bulge"].tolist()) == {-1, 0, 1} and {0, 1, 10, 19} <= set(mine["at"].tolist())


def test_extraction_pattern_with_a_code_at_the_spans_first_position():
    rng = np.random.default_rng(23)
    text = list(random_text(rng, 6000))
    guide = "C" + random_text(rng, 19)
    for k, (b, i) in enumerate([(0, 0), (1, 1), (-1, 1), (1, 12), (-1, 18), (1, 19)]):
        site = bulged(guide, b, i, rng) + "CAG"
        text[500 + 800 * k:500 + 800 * k + len(site)] = site if k % 2 == 0 else su.revcomp(site)
    blob = fasta_of(["".join(text)])
    queries = [guide + "NNN", "T" + guide[1:] + "NNN", "N" * 23]  # a site that starts with T is none of the pattern's
    off, rows = check_bulges([blob], "VNNNNNNNNNNNNNNNNNNNNRG", queries, (0, 20), 2, 1, 1)
    assert set(rows["bulge"][:int(off[1])].tolist()) == {-1, 0, 1}
    assert not (rows["site"] & np.uint64(3) == 3).any()  # V at position 0 of every window, whatever its length


# ---- query counts and cutting ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def query_case():
    rng = np.random.default_rng(77)
    text = list(random_text(rng, 6000))
    drawn = []
    for k in range(40):  # 40 guides, each with one bulged site in the text
        guide = random_text(rng, 20)
        b, i = [(1, 1 + k % 19), (-1, 1 + k % 18), (0, 0)][k % 3]
        site = bulged(guide, b, i, rng) + "NGG".replace("N", "ACGT"[k % 4])
        text[100 + 140 * k:100 + 140 * k + len(site)] = site if k % 2 else su.revcomp(site)
        drawn.append(guide + "NNN")
    blob = fasta_of(["".join(text)])
    records = lu.parse([blob])
    pool = [random_text(rng, 20) + "NNN" for _ in range(257 - 40 - 60 - 10)] + [mutate(rng, q[:20], 1) + "NNN" for q in drawn] + \
           [mutate(rng, q[:20], 2) + "NNN" for q in drawn[:20]] + drawn + drawn[:10]  # duplicated queries at the end
    assert len(pool) == 257
    want = bu.brute_force(records, NGG, pool, (0, 20), 2, 1, 1)
    return blob, pool, want


@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1, 65, 257])
def test_query_counts(query_case, n):
    blob, pool, want = query_case
    queries = pool[-n:]
    part = bu.of_queries(want, len(pool) - n, n)
    with ca.Genome.open([blob]) as g:
        off, rows = check_bulges([blob], NGG, queries, (0, 20), 2, 1, 1, genome=g, want=part)
        assert len(rows) > 0
        off2, rows2 = g.search_bulges(NGG, queries, (0, 20), 2, 1, 1)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs
        if n == 65:  # one call = the concatenation of n single-query calls
            parts = [g.search_bulges(NGG, [q], (0, 20), 2, 1, 1)[1] for q in queries]
            for k, p in enumerate(parts):
                p["query"] = k
            assert np.concatenate(parts).tobytes() == rows.tobytes() and {-1, 0, 1} == set(rows["bulge"].tolist())
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()


# ---- more queries than a piece holds ---------------------------------------------------------------------------------------

PIECE_BULGES = 1 << 19  # BulgeSearch::kPieceQueries: 19 bits of query in a hit word


def two_piece_case():
    """2^19 + 1 queries over a pool of 1025 (query k is pool[k % 1025]) against one record of 400 random bases, NGG, span
    (0, 20), max_dist 1, D = R = 1.  Three pool queries are read off forward sites of the record: pool[513], the single query
    of the second piece (2^19 mod 1025 = 513), copies a site; pool[7] is a site of 21 bases less one base (a DNA bulge),
    pool[11] a site of 19 bases with one base put in (an RNA bulge).  -> (blob, pool, which, offsets, rows), the expected
    bytes being the pool's brute force, tiled.  No device needed."""
    rng = np.random.default_rng(5)
    text = random_text(rng, 400)
    records = [(b"rec0 some text", text.encode())]
    _, _, _, t = su.candidates(records, NGG)
    assert 16 <= len(t) <= 64  # at most one workgroup and one wave of survivors
    sites = [p for p in range(1, 400 - 23) if text[p + 21:p + 23] == "GG"]
    a, b, c = (int(p) for p in rng.choice(sites, size=3, replace=False))
    pool = [random_text(rng, 20) + "NNN" for _ in range(1025)]
    pool[513] = text[a:a + 20] + "NNN"
    pool[7] = text[b - 1:b + 8] + text[b + 9:b + 20] + "NNN"
    pool[11] = text[c + 1:c + 10] + "ACGT"[int(rng.integers(0, 4))] + text[c + 10:c + 20] + "NNN"
    p_off, p_rows, _ = bu.brute_force(records, NGG, pool, (0, 20), 1, 1, 1)
    n = PIECE_BULGES + 1
    which = np.arange(n) % 1025
    counts = np.diff(p_off.astype(np.int64))[which]
    want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    has = np.flatnonzero(counts)
    want_rows = np.concatenate([p_rows[int(p_off[which[k]]):int(p_off[which[k] + 1])] for k in has])
    want_rows["query"] = np.repeat(has, counts[has])
    return fasta_of([text]), pool, which, want_off, want_rows


def test_more_queries_than_a_piece_holds():
    """The two-piece path of the bulged search: the rows of the second piece are written behind the first piece's, to host
    memory and to device memory, and not at all when they do not fit."""
    import torch
    blob, pool, which, want_off, want_rows = two_piece_case()
    n, total = len(which), len(want_rows)
    first = want_rows[:int(want_off[PIECE_BULGES])]
    assert want_off[n] - want_off[PIECE_BULGES] >= 1 and which[PIECE_BULGES] == 513  # the second piece has rows
    assert (first["bulge"] == -1).any() and (first["bulge"] == 1).any()
    pat, pq = ca.search_prepare(NGG, pool)
    q = np.ascontiguousarray(pq[which])
    bg = _lib.SearchBulges(0, 20, 1, 1)
    with ca.Genome.open([blob]) as g:
        off, rows = g.search_bulges(pat, q, (0, 20), 1, 1, 1)
        assert off.tobytes() == want_off.tobytes() and rows.tobytes() == want_rows.tobytes()
        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        d_hits = torch.full((total * 32,), 0xA5, dtype=torch.uint8, device="cuda")  # exactly n_total rows
        assert g.search_bulges_device(pat, d_q, d_off, d_hits, (0, 20), 1, 1, 1) == total
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        assert d_hits.cpu().numpy().tobytes() == want_rows.tobytes()
        poison = np.full(total * 32, 0xA5, dtype=np.uint8)
        off = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint64)
        n_total = C.c_size_t()
        assert _lib.lib.issl_genome_search_bulges(g._h, C.byref(pat), C.byref(bg), q.ctypes.data, n, 1, off.ctypes.data, poison.ctypes.data,
                                                  total - 1, C.byref(n_total)) == 0
        assert n_total.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
