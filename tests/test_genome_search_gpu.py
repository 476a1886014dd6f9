"""GPU: issl_genome_search* against the brute force of tests/search_util.py, byte for byte, and against the independently
pinned chain index -> report -> locate (IsslIndex.landings) under the extraction's own pattern."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import landing_util as ldu
import locate_util as lu
import search_util as su

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslSearchGenome")
EXTRACTION = "VNNNNNNNNNNNNNNNNNNNNRG"
NGG = "N" * 21 + "GG"
TILE = 4096      # kPosPerBlock: text positions per workgroup
PIECE = 1 << 22  # kPieceQueries: queries per piece (a call with more scans the text once per piece)
GROUP = 4        # kQueryGroup: queries a wave fetches at once inside a piece; the group after it is fetched ahead, which
                 # starts at 2 * GROUP, and what is left of n behind the last whole group is walked one by one


def random_text(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def fasta_of(seqs):
    return b"".join(b">rec%d some text\n%s\n" % (k, s.encode()) for k, s in enumerate(seqs))


def mutate(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), size=k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def check_search(blobs, pattern, queries, max_dist, genome=None):
    """One search and one profile on the device equal the brute force, byte for byte.  -> (offsets, rows)"""
    want_off, want_rows, want_prof = su.brute_force_fasta(blobs, pattern, queries, max_dist)
    g = genome or ca.Genome.open(blobs)
    try:
        off, rows = g.search(pattern, queries, max_dist)
        prof = g.search_profile(pattern, queries, max_dist)
    finally:
        if genome is None:
            g.close()
    assert off.dtype == np.uint64 and off.tobytes() == want_off.tobytes()
    assert rows.dtype == ca.SEARCH_HIT_DTYPE and len(rows) == len(want_rows)
    if rows.tobytes() != want_rows.tobytes():
        bad = int(np.flatnonzero(rows != want_rows)[0])
        raise AssertionError(f"row {bad}: got {rows[bad]}, want {want_rows[bad]}")
    assert prof.dtype == np.uint64 and prof.shape == want_prof.shape and prof.tobytes() == want_prof.tobytes()
    return off, rows


# ---- tile edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [23, 32])
@pytest.mark.parametrize("extra", ["4095", "4096", "4097", "4096+L-1", "8193"])
def test_tile_edges(L, extra):
    n = {"4095": 4095, "4096": 4096, "4097": 4097, "4096+L-1": TILE + L - 1, "8193": 8193}[extra]
    rng = np.random.default_rng(n * 100 + L)
    text = list(random_text(rng, n))
    lo, hi = TILE - 2 * L, min(n, TILE + 2 * L)
    text[lo:hi] = "A" * (hi - lo)  # A^L on strand 0 and T^L on strand 1 at every window start from 4096 - L to 4096 (and around)
    planted = random_text(rng, L)
    text[0:L] = planted                                  # position 0, strand 0
    if hi < n - L:                                       # the last possible start: strand 1, one mismatch -- or A^L where the
        text[n - L:n] = su.revcomp(mutate(rng, planted, 1))  # stretch of A reaches the record's end
    text = "".join(text)
    queries = ["A" * L, "T" * L, "N" * L, planted]
    off, rows = check_search([fasta_of([text])], "N" * L, queries, 1)
    a_rows = rows[int(off[0]):int(off[1])]
    starts = set(a_rows["pos"][(a_rows["strand"] == 0) & (a_rows["dist"] == 0)].tolist())
    assert set(range(TILE - L, min(TILE, n - L) + 1)) <= starts
    t_rows = rows[int(off[1]):int(off[2])]
    assert set(range(TILE - L, min(TILE, n - L) + 1)) <= set(t_rows["pos"][(t_rows["strand"] == 1) & (t_rows["dist"] == 0)].tolist())
    assert int(off[3]) - int(off[2]) == 2 * (n - L + 1)  # the all-N query: every window, both strands
    mine = su.as_tuples(rows[int(off[3]):], L)
    assert (3, 0, 0, 0, 0, planted) in mine
    assert any(r[2] == n - L and r[3] == 1 and r[4] == 1 for r in mine) if hi < n - L else n - L in starts


def test_short_and_empty_records_and_an_empty_genome():
    queries = ["ACGTACGT", "NNNNNNNN"]
    for blob in (b"", b"\n\n", b">only\n", b">a\nACGTACG\n", b">e\n>s\nACG\n>t\nACGTACGT\n>u\n", b">a\nACGTACGT\n"):
        off, rows = check_search([blob], "NNNNNNNN", queries, 2)
        assert len(rows) == (4 if b"ACGTACGT" in blob else 0)  # ACGTACGT is its own reverse complement
    with ca.Genome.open([b">a\nACGTACGT\n"]) as g:
        off, rows = g.search("NNNNNNNN", [], 2)  # n == 0
        assert off.tolist() == [0] and len(rows) == 0 and g.search_profile("NNNNNNNN", [], 2).shape == (0, 3)


# ---- pattern lengths and alphabet -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_text():
    rng = np.random.default_rng(11)
    text = list(random_text(rng, 6000))
    text[3000:3100] = "A" * 100
    text[5000:5100] = "T" * 100
    return "".join(text)


@pytest.mark.parametrize("L", [1, 20, 23, 24, 31, 32])
def test_pattern_lengths(one_text, L):
    rng = np.random.default_rng(L)
    pattern = ("N" * L + "RG")[-L:]
    records = lu.parse([fasta_of([one_text])])
    _, _, _, t = su.candidates(records, pattern)
    assert len(t) > 100
    drawn = ["".join("ACGT"[c] for c in t[i]) for i in rng.choice(len(t), size=12, replace=False)]
    queries = drawn[:4] + [mutate(rng, q, min(L, 2)) for q in drawn[4:8]] + [mutate(rng, q, min(L, 4)) for q in drawn[8:]]
    queries += ["N" * L, "n" * (L // 2) + "G" * (L - L // 2)]
    check_search([fasta_of([one_text])], pattern, queries, min(L, 3))
    # every bit of a packed word in use: poly-A / poly-T stretches under the all-N pattern
    check_search([fasta_of([one_text])], "N" * L, ["T" * L, "A" * L, "T" * (L - 1) + "C"], min(L, 1))


def test_all_iupac_codes_five_prime_pam_and_all_n_query():
    rng = np.random.default_rng(5)
    pattern = "ACGTRYSWKMBDHVN"
    text = list(random_text(rng, 50000))
    instances = ["".join(rng.choice(list(su.IUPAC[c])) for c in pattern) for _ in range(24)]
    for k, inst in enumerate(instances):
        at = 1000 + 2000 * k
        text[at:at + 15] = inst if k % 2 == 0 else su.revcomp(inst)
    text = "".join(text)
    blob = fasta_of([text[:20000], text[20000:]])
    off, rows = check_search([blob], pattern, ["N" * 15] + instances[:6] + [mutate(rng, i, 2) for i in instances[6:12]], 2)
    assert int(off[1]) >= 24 and {0, 1} == set(rows["strand"][:int(off[1])].tolist())
    check_search([blob], pattern.lower(), ["n" * 15], 0)
    # Cas12a: TTTV in front of a 20-nt protospacer
    cas12a = "TTTV" + "N" * 20
    records = lu.parse([blob])
    _, _, _, t = su.candidates(records, cas12a)
    assert len(t) > 200
    guides = ["NNNN" + "".join("ACGT"[c] for c in t[i][4:]) for i in rng.choice(len(t), size=16, replace=False)]
    guides += ["NNNN" + mutate(rng, g[4:], 3) for g in guides[:8]] + ["N" * 24]
    check_search([blob], cas12a, guides, 4)
    # SaCas9: NNGRRT behind a 21-nt guide
    check_search([blob], "N" * 21 + "NNGRRT", ["N" * 27, text[100:121] + "NNNNNN"], 6)


# ---- records -----------------------------------------------------------------------------------------------------------

def test_many_short_records():
    """4100 records of 30 bases -- more than a 4096-entry record table holds -- with would-be hits across the first
    boundaries and characters outside ACGT inside windows."""
    rng = np.random.default_rng(4100)
    L = 12
    seqs = [random_text(rng, 30) for _ in range(4100)]
    across = [seqs[k][-6:] + seqs[k + 1][:6] for k in range(4)]           # would lie across the boundary k | k + 1
    inside = [seqs[0][:L], seqs[1][18:], seqs[4099][18:], su.revcomp(seqs[2050][9:21])]
    for k, ch in ((10, "N"), (11, "R"), (12, "n"), (13, "-"), (14, "U")):   # a window through position 15 of these is none
        seqs[k] = seqs[k][:15] + ch + seqs[k][16:]
    broken = [seqs[k][10:22].upper().replace("N", "A").replace("R", "A").replace("-", "A").replace("U", "A") for k in (10, 11, 12, 13, 14)]
    blob = fasta_of(seqs)
    queries = across + inside + broken + ["N" * L]
    off, rows = check_search([blob], "N" * L, queries, 0)
    per_query = np.diff(off.astype(np.int64))
    assert per_query[:4].tolist() == [0, 0, 0, 0] and (per_query[4:8] >= 1).all()
    assert per_query[-1] == 2 * (4095 * 19 + 5 * 7)  # 19 windows per record, 7 where the character at 15 is bad
    last = rows[int(off[-2]):]
    assert int(last["record"].max()) == 4099 and int(last["pos"].max()) == 18
    check_search([blob], "N" * 10 + "GG", inside[:2] + ["N" * L], 3)


# ---- query counts and cutting -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def query_case():
    rng = np.random.default_rng(77)
    blob = ldu.repeat_genome(77, mbp=0.03, records=3)
    records = lu.parse([blob])
    rec, pos, strand, t = su.candidates(records, NGG)
    drawn = ["".join("ACGT"[c] for c in t[i][:20]) + "NNN" for i in rng.choice(len(t), size=400, replace=False)]
    pool = drawn + [mutate(rng, q[:20], 2) + "NNN" for q in drawn[:300]] + [random_text(rng, 20) + "NNN" for _ in range(300)]
    pool += pool[:25]  # duplicated queries
    assert len(pool) == 1025
    want = su.brute_force(records, NGG, pool, 3)
    return blob, records, pool, want


@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1, 63, 64, 65, 257, 1025])
def test_query_counts(query_case, n):
    blob, records, pool, _ = query_case
    queries = pool[-n:]  # the duplicates are at the end
    with ca.Genome.open([blob]) as g:
        off, rows = check_search([blob], NGG, queries, 3, genome=g)
        off2, rows2 = g.search(NGG, queries, 3)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs
        assert len(rows) > 0
        if n == 65:  # one call = the concatenation of n single-query calls
            parts = [g.search(NGG, [q], 3)[1] for q in queries]
            for k, p in enumerate(parts):
                p["query"] = k
            assert np.concatenate(parts).tobytes() == rows.tobytes()
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()


def test_duplicated_queries_get_the_same_list(query_case):
    blob, records, pool, want = query_case
    off, rows, _ = want
    for k in range(25):
        a, b = rows[int(off[k]):int(off[k + 1])].copy(), rows[int(off[1000 + k]):int(off[1001 + k])].copy()
        a["query"] = b["query"] = 0
        assert a.tobytes() == b.tobytes()
    assert any(off[k + 1] > off[k] for k in range(25))


def test_more_queries_than_a_piece_holds(query_case):
    """2^22 + 1 queries are two pieces; query k is pool[k % 1025], so the expected rows are the pool's, tiled.  A genome of
    one wave of survivors keeps it quick."""
    rng = np.random.default_rng(3)
    text = random_text(rng, 400)
    records = [(b"rec0 some text", text.encode())]
    _, _, _, t = su.candidates(records, NGG)
    assert 16 <= len(t) <= 64
    drawn = ["".join("ACGT"[c] for c in t[i][:20]) + "NNN" for i in rng.choice(len(t), size=16, replace=False)]
    pool = drawn + [random_text(rng, 20) + "NNN" for _ in range(1025 - 16)]
    p_off, p_rows, p_prof = su.brute_force(records, NGG, pool, 1)
    n = PIECE + 1
    which = np.arange(n) % 1025
    counts = np.diff(p_off.astype(np.int64))[which]
    want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    has = np.flatnonzero(counts)
    want_rows = np.concatenate([p_rows[int(p_off[which[k]]):int(p_off[which[k] + 1])] for k in has])
    want_rows["query"] = np.repeat(has, counts[has])
    pat, q = ca.search_prepare(NGG, pool)
    with ca.Genome.open([fasta_of([text])]) as g:
        off, rows = g.search(pat, q[which], 1)
    assert off.tobytes() == want_off.tobytes() and rows.tobytes() == want_rows.tobytes() and len(rows) >= n // 1025 * 16


# ---- many hits, the capacity rule ---------------------------------------------------------------------------------------

def test_many_hits_profile_and_capacity():
    rng = np.random.default_rng(20)
    text = random_text(rng, 20000)
    blob = fasta_of([text])
    queries = ["NNNN", "ANNN", "NNNT", "NCNN", "nnnn", "NNGN", "ACGT", "NNNN"]
    want_off, want_rows, want_prof = su.brute_force_fasta([blob], "NNNN", queries, 4)
    assert len(want_rows) == 8 * 2 * (20000 - 3)  # every window-strand hits every query
    with ca.Genome.open([blob]) as g:
        check_search([blob], "NNNN", queries, 4, genome=g)
        pat, q = ca.search_prepare("NNNN", queries)
        total = len(want_rows)
        poison = np.full(total * 32, 0xA5, dtype=np.uint8)
        off = np.full(9, 0xFFFFFFFF, dtype=np.uint64)
        n = C.c_size_t()
        rc = _lib.lib.issl_genome_search(g._h, C.byref(pat), q.ctypes.data, 8, 4, off.ctypes.data, poison.ctypes.data, total - 1, C.byref(n))
        assert rc == 0 and n.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
        rc = _lib.lib.issl_genome_search(g._h, C.byref(pat), q.ctypes.data, 8, 4, off.ctypes.data, poison.ctypes.data, total, C.byref(n))
        assert rc == 0 and poison.tobytes() == want_rows.tobytes()


# ---- device entry points -------------------------------------------------------------------------------------------------

def test_device_entry_points(query_case):
    import torch
    blob, records, pool, want = query_case
    want_off, want_rows, want_prof = want
    pat, q = ca.search_prepare(NGG, pool)
    d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_off = torch.full((len(pool) + 1,), -1, dtype=torch.int64, device="cuda")
    with ca.Genome.open([blob]) as g:
        total = g.search_device(pat, d_q, d_off, None, 3)  # the counting call
        assert total == len(want_rows) and d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert g.search_device(pat, d_q, d_off, d_hits[:(total - 1) * 32], 3) == total
        assert bool((d_hits == 0xA5).all())  # they do not fit: nothing is written
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_device(NGG, d_q, d_off, d_hits, 3, stream=stream.cuda_stream) == total
        rows = d_hits.cpu().numpy().view(ca.SEARCH_HIT_DTYPE)
        assert rows.tobytes() == want_rows.tobytes()
        d_counts = torch.full((len(pool) * 4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        g.search_profile_device(pat, d_q, d_counts, 3, stream=stream.cuda_stream)
        prof = d_counts.cpu().numpy().view(np.uint64).reshape(len(pool), 4)
        assert prof.tobytes() == want_prof.tobytes()
        by_dist = np.zeros_like(prof)  # the profile is the rows counted by dist
        np.add.at(by_dist, (rows["query"], rows["dist"]), 1)
        assert np.array_equal(by_dist, prof)
        assert g.search_device(pat, d_q[:0], d_off[:1], None, 3) == 0 and int(d_off[0]) == 0  # n == 0


# ---- the cross-check against index -> report -> locate ------------------------------------------------------------------

def _landing_set(ix, genome, guides, max_dist):
    offsets, rows = ix.landings(guides, genome, None, max_dist=max_dist)
    out = np.zeros(len(rows), dtype=[("guide", "<u4"), ("record", "<u4"), ("pos", "<u8"), ("strand", "<u4"), ("dist", "<u4"), ("site", "<u8")])
    for f in out.dtype.names:
        out[f] = rows[f]
    return np.sort(out, order=list(out.dtype.names))


def _search_set(genome, guides, max_dist):
    texts = lu.sig_text(guides)
    parts = []
    for strand, queries in ((0, [t.decode() + "NNN" for t in texts]), (1, ["NNN" + t.decode() for t in texts])):
        _, rows = genome.search(EXTRACTION, queries, max_dist)
        rows = rows[rows["strand"] == strand]
        part = np.zeros(len(rows), dtype=[("guide", "<u4"), ("record", "<u4"), ("pos", "<u8"), ("strand", "<u4"), ("dist", "<u4"), ("site", "<u8")])
        part["guide"], part["record"], part["pos"], part["strand"], part["dist"] = rows["query"], rows["record"], rows["pos"], strand, rows["dist"]
        part["site"] = rows["site"] & np.uint64((1 << 40) - 1) if strand == 0 else rows["site"] >> np.uint64(6)
        parts.append(part)
    out = np.concatenate(parts)
    return np.sort(out, order=list(out.dtype.names))


@pytest.mark.parametrize("name", ["bowtie", "repeat"])
def test_extraction_pattern_reproduces_the_landings(name):
    """The rows of issl_offtarget_landings come from an index of the extraction's sites, the scorer's scan and locate; the
    search knows none of the three.  Under the extraction's forward pattern -- strand 0 with guide + NNN, strand 1 with
    NNN + guide, where the reference's odd cut is t[3:23] -- the two must list the same (guide, record, pos, strand, dist,
    site), nothing left out on either side."""
    blob = (ROOT / "tests" / "golden" / "bowtie" / "genome.fa").read_bytes() if name == "bowtie" else ldu.repeat_genome(9, mbp=0.1, records=4)
    rng = np.random.default_rng(len(blob))
    truth = lu.brute_force(lu.parse([blob]))
    assert len(truth) > 500
    own = truth["site"][rng.choice(len(truth), size=48, replace=False)]
    texts = [t.decode() for t in lu.sig_text(own)]
    texts += [mutate(rng, t, 1 + k % 4) for k, t in enumerate(texts[:32])]
    guides = ca.encode_guides(texts)
    ix = ca.IsslIndex.build_from_fasta([blob])
    try:
        with ca.Genome.open([blob]) as genome:
            seen = 0
            for max_dist in (0, 2, 4):
                want = _landing_set(ix, genome, guides, max_dist)
                got = _search_set(genome, guides, max_dist)
                assert len(want) >= 48 and len(np.unique(want)) == len(want)
                assert got.tobytes() == want.tobytes(), (max_dist, len(got), len(want))
                assert {0, 1} == set(want["strand"].tolist())
                seen = max(seen, int(want["dist"].max()))
            assert seen >= 2
    finally:
        ix.close()


# ---- the executable ------------------------------------------------------------------------------------------------------

def test_cli_prints_the_brute_force(tmp_path, query_case):
    blob, records, pool, _ = query_case
    queries = pool[:40] + pool[400:420] + ["n" * 23]
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(blob)
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\r\n".join(queries[:30]) + "\r\n" + "\n".join(queries[30:]) + "\n\n")
    want_off, want_rows, want_prof = su.brute_force(records, NGG, queries, 2)
    assert len(want_rows) > 2000
    r = subprocess.run([EXE, NGG, str(qfile), "2", str(fasta)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == su.format_rows(records, queries, want_rows)
    r = subprocess.run([EXE, "--profile", NGG.lower(), str(qfile), "2", str(fasta)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == su.format_profile(queries, want_prof)
