"""issl_genome_search_bulges* where the text is not A C G T: a bad byte at every offset of a bulged site, at the tile edge,
records that end inside a window, genomes shorter than some or all of the window lengths L + b, and the settings that use all
seven launches (max_dna = max_rna = 3).  A call runs one launch per b with its own window length, its own win_mask and its own
"does the text hold such a window" test, so every case has sites of every b side by side.  Rows, offsets and profile are
compared byte for byte with tests/bulge_util.py.  The tests that need a device carry the gpu mark; the others assert on the
brute force alone that the cases say what they are meant to say."""
import ctypes as C
import functools

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import bulge_util as bu
import locate_util as lu
import search_util as su
import test_bulge_gpu as tb  # check_bulges, bulged, mutate, random_text, fasta_of

gpu = pytest.mark.gpu
NGG = tb.NGG
TILE = tb.TILE
GROUP = tb.GROUP
L, G = 23, 20
CPF1 = "TTTV" + "N" * 20  # a 5' PAM: L = 24, span (4, 20)
BAD = "NR-U"              # an assembly gap, an ambiguity code, an alignment gap, a base of RNA
ALL_B = (-3, -2, -1, 0, 1, 2, 3)


def planted_found(rows, plants, query=0):
    """The plants [(start, strand, b)] that `query` has a row for: at the plant's own start, strand and bulge."""
    mine = rows[rows["query"] == query]
    have = set(zip(mine["pos"].tolist(), mine["strand"].tolist(), mine["bulge"].tolist()))
    return {p for p in plants if p in have}


# ---- a bad byte at every offset ----------------------------------------------------------------------------------------

SWEEP = {"ngg": (NGG, (0, G), list(range(L + 4))), "cpf1": (CPF1, (4, G), [0, 4, 24 - 1, 24, 24 + 2])}


@functools.lru_cache(maxsize=None)
def sweep_clean(name):
    """One guide planted for every b in -3..3 at break point 10 on both strands, 60 bases apart, in 6 000 random bases (the
    plants lie on both sides of text position 4096).  -> (text, plants [(start, strand, b)], queries)"""
    pattern, span, _ = SWEEP[name]
    rng = np.random.default_rng(3100 + len(pattern))
    guide = tb.random_text(rng, G)
    text = list(tb.random_text(rng, 6000))
    plants = []
    at = 3718
    for b in ALL_B:
        for strand in (0, 1):
            site = tb.bulged(guide, b, 10, rng)
            site = site + "TGG" if name == "ngg" else "TTTA" + site
            assert len(site) == len(pattern) + b
            text[at:at + len(site)] = site if strand == 0 else su.revcomp(site)
            plants.append((at, strand, b))
            at += 60
    pad = "N" * span[0], "N" * (len(pattern) - span[0] - G)
    queries = [pad[0] + guide + pad[1], pad[0] + tb.mutate(rng, guide, 1) + pad[1], "N" * len(pattern)]
    return "".join(text), tuple(plants), tuple(queries)


@functools.lru_cache(maxsize=None)
def sweep_case(name, o):
    """The clean text with a bad byte at offset o from every plant's window start (o is None: the clean text).
    -> (blob, queries, the brute force, plants)"""
    pattern, span, _ = SWEEP[name]
    text, plants, queries = sweep_clean(name)
    if o is not None:
        text = list(text)
        for start, _, _ in plants:
            text[start + o] = BAD[o % 4]
        text = "".join(text)
    blob = tb.fasta_of([text])
    return blob, queries, bu.brute_force(lu.parse([blob]), pattern, list(queries), span, 2, 3, 3), plants


SWEEP_PARAMS = [(name, o) for name in SWEEP for o in SWEEP[name][2]]


@pytest.mark.parametrize("name,o", SWEEP_PARAMS)
def test_the_sweep_loses_the_windows_over_the_byte_and_no_other(name, o):
    """On the brute force alone.  A window of Lp + b bases covers offset o when Lp + b > o.  The shortest window has Lp - 3
    bases, so every plant is lost for o < Lp - 3 (o = 0 is one of these offsets, not the only one); from Lp - 3 to Lp + 2 the
    plants with Lp + b <= o stay and the longer ones go; at Lp + 3 the byte lies behind every window and all stay."""
    pattern = SWEEP[name][0]
    Lp = len(pattern)
    _, _, (_, clean_rows, _), plants = sweep_case(name, None)
    assert planted_found(clean_rows, plants) == set(plants) and len(plants) == 14
    _, _, (_, rows, _), _ = sweep_case(name, o)
    stay = {p for p in plants if Lp + p[2] <= o}
    assert planted_found(rows, plants) == stay
    if Lp - 3 <= o < Lp + 3:
        assert stay and set(plants) - stay  # at least one survives, at least one is lost
        assert {p[1] for p in stay} == {0, 1}
    assert len(stay) == 2 * max(0, min(7, o - (Lp - 3) + 1))
    # the all-N query loses rows as well and keeps most of them
    clean_n, with_n = int((clean_rows["query"] == 2).sum()), int((rows["query"] == 2).sum())
    assert clean_n // 2 < with_n <= clean_n


@gpu
@pytest.mark.parametrize("name,o", SWEEP_PARAMS)
def test_a_bad_byte_at_every_offset(name, o):
    pattern, span, _ = SWEEP[name]
    blob, queries, want, _ = sweep_case(name, o)
    tb.check_bulges([blob], pattern, list(queries), span, 2, 3, 3, want=want)


@gpu
def test_the_clean_sweep_texts():
    for name, (pattern, span, _) in SWEEP.items():
        blob, queries, want, _ = sweep_case(name, None)
        tb.check_bulges([blob], pattern, list(queries), span, 2, 3, 3, want=want)


# ---- the same at the tile edge ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_case(k):
    """A plant of b = 3 (26 bases) whose window starts at 4096 - 25 + k in a text of 4096 + 40 bases; the bad byte at text
    position 4095, at 4096 and at the window's last base.  -> (start, strand, queries, [(bad position or None, blob, brute
    force)])"""
    rng = np.random.default_rng(4096 + k)
    guide = tb.random_text(rng, G)
    site = tb.bulged(guide, 3, 10, rng) + "TGG"
    start, strand = TILE - 25 + k, k % 2
    text = list(tb.random_text(rng, TILE + 40))
    text[start:start + 26] = site if strand == 0 else su.revcomp(site)
    queries = [guide + "NNN", "N" * L]
    out = []
    for n, bad in enumerate((None, TILE - 1, TILE, start + 25)):
        mine = list(text)
        if bad is not None:
            mine[bad] = BAD[(k + n) % 4]
        blob = tb.fasta_of(["".join(mine)])
        out.append((bad, blob, bu.brute_force(lu.parse([blob]), NGG, queries, (0, G), 2, 3, 3)))
    return start, strand, queries, out


EDGE_K = (0, 12, 24, 25)


@pytest.mark.parametrize("k", EDGE_K)
def test_the_tile_edge_cases_lose_the_plant_when_the_byte_is_inside(k):
    start, strand, _, cases = edge_case(k)
    assert start <= TILE <= start + 25  # k = 0: the window's last base is position 4096; k = 25: its first
    for bad, _, (_, rows, _) in cases:
        inside = bad is not None and start <= bad < start + 26
        assert planted_found(rows, [(start, strand, 3)]) == (set() if inside else {(start, strand, 3)}), bad
    assert [bad is not None and start <= bad < start + 26 for bad, _, _ in cases] == [False, k != 25, True, True]


@gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_a_bad_byte_at_the_tile_edge(k):
    _, _, queries, cases = edge_case(k)
    for _, blob, want in cases:
        tb.check_bulges([blob], NGG, queries, (0, G), 2, 3, 3, want=want)


# ---- record ends -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def record_ends_case():
    """Records of L - 4 .. L + 4 bases, each a site of its own length (19 bases: too short for any window; 27: a site of 26
    and one more base), on alternating strands, an empty record behind each; a site cut in two by a record end, with and
    without an empty record between the halves; one long record last.  -> (blob, records, queries, the brute force, lengths)"""
    rng = np.random.default_rng(99)
    guide = tb.random_text(rng, G)
    seqs = []
    for n in range(L - 4, L + 5):
        b = n - L
        if b < -3:
            s = (guide + "TGG")[-n:]
        elif b > 3:
            s = tb.bulged(guide, 3, 10, rng) + "TGG" + "A"
        else:
            s = tb.bulged(guide, b, 10, rng) + "TGG"
        assert len(s) == n
        seqs += [s if n % 2 else su.revcomp(s), ""]
    site = guide + "TGG"
    seqs += [tb.random_text(rng, 40) + site[:12], site[12:] + tb.random_text(rng, 40)]
    seqs += [tb.random_text(rng, 40) + su.revcomp(site)[:9], "", su.revcomp(site)[9:] + tb.random_text(rng, 40)]
    long = list(tb.random_text(rng, 300))
    long[100:121] = tb.bulged(guide, -2, 5, rng) + "AGG"
    long[200:225] = su.revcomp(tb.bulged(guide, 2, 15, rng) + "CGG")
    long[277:300] = guide + "GGG"  # ends with the record
    seqs.append("".join(long))
    blob = tb.fasta_of(seqs)
    records = lu.parse([blob])
    assert [len(s) for _, s in records] == [len(s) for s in seqs]
    queries = [guide + "NNN", tb.mutate(rng, guide, 1) + "NNN", "N" * L]
    return blob, records, queries, bu.brute_force(records, NGG, queries, (0, G), 2, 3, 3), [len(s) for s in seqs]


def test_the_record_ends_case_cuts_the_bulges_by_the_records_length():
    _, records, _, (_, rows, _), lengths = record_ends_case()
    mine = rows[rows["query"] == 0]
    some_not_all = 0
    for k, n in enumerate(range(L - 4, L + 5)):
        got = set(mine["bulge"][mine["record"] == 2 * k].tolist())
        assert lengths[2 * k] == n and lengths[2 * k + 1] == 0
        assert got <= {b for b in ALL_B if L + b <= n}, n  # no window is longer than its record
        assert (min(n - L, 3) in got) == (n >= L - 3), n     # the site that fits exactly
        some_not_all += 0 < len(got) < 7
    assert some_not_all >= 1
    assert max(mine["bulge"][mine["record"] == 2 * 5].tolist()) == 1  # L + 1 bases: rows for b <= 1 only
    cut = [r for r in range(18, 23)]
    assert not np.isin(mine["record"], cut).any() and [lengths[r] for r in cut] == [52, 51, 49, 0, 54]
    assert planted_found(mine[mine["record"] == 23], [(100, 0, -2), (200, 1, 2), (277, 0, 0)]) == {(100, 0, -2), (200, 1, 2), (277, 0, 0)}
    ends = rows["pos"].astype(np.int64) + L + rows["bulge"] - np.array(lengths, dtype=np.int64)[rows["record"]]
    assert (ends <= 0).all() and (ends == 0).any()  # no window reaches past its record; some end with it


@gpu
def test_record_ends():
    blob, _, queries, want, _ = record_ends_case()
    tb.check_bulges([blob], NGG, queries, (0, G), 2, 3, 3, want=want)
    tb.check_bulges([blob], NGG, queries, (0, G), 2, 1, 2)  # other launches: the same records under other window lengths


WHOLE = (0, 5, L - 3, L, L + 1, L + 3)


@functools.lru_cache(maxsize=None)
def whole_genome(n):
    """A genome of exactly n bases in one record: a site of n bases where there is one."""
    rng = np.random.default_rng(500 + n)
    guide = tb.random_text(rng, G)
    text = (tb.bulged(guide, n - L, 10, rng) + "TGG") if n >= L - 3 else guide[:n]
    assert len(text) == n
    return tb.fasta_of([text if n % 2 else su.revcomp(text)]), [guide + "NNN", "N" * L]


def test_the_whole_genomes_skip_some_launches_and_all():
    for n in WHOLE:
        blob, queries = whole_genome(n)
        for D, R in ((3, 3), (3, 0), (0, 3), (1, 1)):
            _, rows, _ = bu.brute_force_fasta([blob], NGG, queries, (0, G), 2, D, R)
            fit = {b for b in range(-R, D + 1) if L + b <= n}
            assert set(rows["bulge"].tolist()) <= fit
            assert (n - L in fit) == (n - L in set(rows["bulge"][rows["query"] == 0].tolist())), (n, D, R)
    assert not len(bu.brute_force_fasta([whole_genome(L - 3)[0]], NGG, whole_genome(L - 3)[1], (0, G), 2, 3, 0)[1])  # all skipped


@gpu
@pytest.mark.parametrize("n", WHOLE)
def test_genomes_shorter_than_some_windows_or_all(n):
    blob, queries = whole_genome(n)
    for D, R in ((3, 3), (3, 0), (0, 3), (1, 1)):
        tb.check_bulges([blob], NGG, queries, (0, G), 2, D, R)
    if n == 0:
        tb.check_bulges([b""], NGG, queries, (0, G), 2, 3, 3)
        tb.check_bulges([b">a\n>b\n\n>c\n"], NGG, queries, (0, G), 2, 3, 3)


# ---- seven slots -----------------------------------------------------------------------------------------------------------

def wave_groups(n):
    """The query groups of a call with n queries as k_bulge forms them: wave w of a workgroup's four takes the queries
    [n * w / 4, n * (w + 1) / 4) and fetches them kQueryGroup at a time from its first one on; what is left goes one by one."""
    out = []
    for w in range(4):
        lo, hi = n * w // 4, n * (w + 1) // 4
        out += [(q, q + GROUP) for q in range(lo, hi - GROUP + 1, GROUP)]
    return out


SEVEN_COUNTS = (1, 4, 5, 9, 16, 17, 20)  # 16: a whole group per wave; 17: a group and one query; 20: five queries per wave


@functools.lru_cache(maxsize=None)
def seven_case():
    """L = 23, span (0, 20), D = R = 3, max_dist 3 on 8 000 bases in two records, planted as test_bulge_gpu.ngg_case plants it
    but for b in +-3 too: two guides, every b at break points 1, 7 + k and the last legal one (G - 1 for DNA, G - 1 - r for
    RNA), every second plant on strand 1, half of the bulged ones with a mismatch; a homopolymer tie.  20 queries, of which
    the guides, the run, a guide with a mismatch, a guide named twice and the all-N query have rows and the random ones none."""
    rng = np.random.default_rng(2027)
    text = list(tb.random_text(rng, 8000))
    guides = [tb.random_text(rng, G) for _ in range(2)]
    run = tb.random_text(rng, 8) + "AAAA" + tb.random_text(rng, 8)
    plants = []
    for k, guide in enumerate(guides):
        plants.append(guide + "TGG")
        for b in (-3, -2, -1, 1, 2, 3):
            for i in (1, 7 + k, G - 1 - max(-b, 0)):
                site = tb.bulged(guide, b, i, rng)
                plants.append((tb.mutate(rng, site, 1) if (i + k) % 2 else site) + "AGG")
    plants.append(run[:10] + "A" + run[10:] + "CGG")
    plants.append(run[:9] + run[10:] + "CGG")
    at = 100
    for k, site in enumerate(plants):
        s = site if k % 2 == 0 else su.revcomp(site)
        text[at:at + len(s)] = s
        at += 190
    assert at < 7900
    text = "".join(text)
    blob = tb.fasta_of([text[:4080], text[4080:]])
    records = lu.parse([blob])
    rand = lambda: tb.random_text(rng, G) + "NNN"  # noqa: E731
    queries = [guides[0] + "NNN", rand(), rand(), rand(), rand(), guides[1] + "NNN", rand(), run + "NNN", "N" * L, rand(), rand(), rand(),
               tb.mutate(rng, guides[0], 1) + "NNN", rand(), rand(), rand(), guides[1] + "NNN", rand(), rand(), rand()]
    assert len(queries) == 20
    return blob, records, queries, bu.brute_force(records, NGG, queries, (0, G), 3, 3, 3)


def test_the_seven_slot_case_has_every_bulge_and_mixed_groups():
    _, _, queries, (offsets, rows, profile) = seven_case()
    planted = rows[np.isin(rows["query"], (0, 5, 7))]
    for strand in (0, 1):
        assert set(planted["bulge"][planted["strand"] == strand].tolist()) == set(ALL_B)
    assert ((planted["bulge"] != 0) & (planted["dist"] > 0)).any()
    for b, last in ((1, 19), (2, 19), (3, 19), (-1, 18), (-2, 17), (-3, 16)):
        seen = set(planted["at"][planted["bulge"] == b].tolist())
        assert 1 in seen and last in seen and seen - {1, last}, (b, seen)
    assert profile.shape == (20, 7, 4) and (profile[8].sum(axis=1) > 100).all()  # the all-N query in every slot
    has = np.diff(offsets.astype(np.int64)) > 0
    assert has.tolist() == [k in (0, 5, 7, 8, 12, 16) for k in range(20)]
    # a block of four consecutive queries of which one has rows and one has none
    assert any(has[k:k + 4].any() and not has[k:k + 4].all() for k in range(0, 20, 4))
    # ... and the groups the kernel forms: none for fewer than 13 queries; from 16 on groups of which one query alone has rows
    assert not any(wave_groups(n) for n in (1, 4, 5, 9)) and len(wave_groups(16)) == len(wave_groups(17)) == len(wave_groups(20)) == 4
    for n in (16, 17, 20):
        assert any(int(has[lo:hi].sum()) == 1 for lo, hi in wave_groups(n)), n


@gpu
@pytest.mark.parametrize("n", SEVEN_COUNTS)
def test_seven_slots_query_counts(n):
    blob, _, queries, want = seven_case()
    part = bu.of_queries(want, 0, n)
    with ca.Genome.open([blob]) as g:
        off, rows = tb.check_bulges([blob], NGG, queries[:n], (0, G), 3, 3, 3, genome=g, want=part)
        assert len(rows) > 0
        off2, rows2 = g.search_bulges(NGG, queries[:n], (0, G), 3, 3, 3)
        assert off2.tobytes() == off.tobytes() and rows2.tobytes() == rows.tobytes()  # the same bytes on two runs


def check_device_and_capacity(blob, pattern, queries, span, max_dist, D, R, want):
    """The device entry points (one on a torch stream) and the capacity rule at n_total - 1, in host and in device memory."""
    import torch
    want_off, want_rows, want_prof = want
    pat, q = ca.search_prepare(pattern, queries)
    bg = _lib.SearchBulges(span[0], span[1], D, R)
    total = len(want_rows)
    assert total > 1
    with ca.Genome.open([blob]) as g:
        poison = np.full(total * 32, 0xA5, dtype=np.uint8)
        off = np.full(len(queries) + 1, 0xFFFFFFFF, dtype=np.uint64)
        n = C.c_size_t()
        args = (g._h, C.byref(pat), C.byref(bg), q.ctypes.data, len(queries), max_dist, off.ctypes.data, poison.ctypes.data)
        assert _lib.lib.issl_genome_search_bulges(*args, total - 1, C.byref(n)) == 0
        assert n.value == total and off.tobytes() == want_off.tobytes()
        assert (poison == 0xA5).all()  # cap one below n_total: nothing is written
        assert _lib.lib.issl_genome_search_bulges(*args, total, C.byref(n)) == 0 and poison.tobytes() == want_rows.tobytes()
        d_q = torch.from_numpy(q.view(np.int64).reshape(-1, 2).copy()).cuda()
        d_off = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda")
        assert g.search_bulges_device(pat, d_q, d_off, None, span, max_dist, D, R) == total  # the counting call
        assert d_off.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_hits = torch.full((total * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert g.search_bulges_device(pat, d_q, d_off, d_hits[:(total - 1) * 32], span, max_dist, D, R) == total
        assert bool((d_hits == 0xA5).all())
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert g.search_bulges_device(pattern, d_q, d_off, d_hits, span, max_dist, D, R, stream=stream.cuda_stream) == total
        assert d_hits.cpu().numpy().view(ca.BULGE_HIT_DTYPE).tobytes() == want_rows.tobytes()
        d_counts = torch.full((want_prof.size,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the fill runs on torch's stream, the search on `stream`)
        g.search_bulges_profile_device(pat, d_q, d_counts, span, max_dist, D, R, stream=stream.cuda_stream)
        assert d_counts.cpu().numpy().view(np.uint64).tobytes() == want_prof.tobytes()


@gpu
def test_seven_slots_device_rows_profile_and_capacity():
    blob, _, queries, want = seven_case()
    assert want[2].shape == (20, 7, 4)
    check_device_and_capacity(blob, NGG, queries, (0, G), 3, 3, 3, want)


@functools.lru_cache(maxsize=None)
def wide_case():
    """L = 29, span (0, 29), D = R = 3: windows of 26 .. 32 bases, every one of which the pattern admits, on random text of
    4 200 bases; a plant of every b on alternating strands at break points 1, 14 and the last legal one; two of b = 3 (32 bases:
    every bit of a packed word) lie at text positions 4063 .. 4094, the last window that needs no halo, and 4095 .. 4126, the
    window that is all halo but its first base."""
    rng = np.random.default_rng(2929)
    guide = tb.random_text(rng, 29)
    text = list(tb.random_text(rng, 4200))
    at = 150
    for k, (b, i) in enumerate([(-3, 1), (-2, 14), (-1, 27), (0, 0), (1, 14), (2, 28), (3, 1), (3, 14), (3, 28), (-3, 25), (1, 1)]):
        site = tb.bulged(guide, b, i, rng)
        start = {7: TILE - 1, 8: TILE - 33}.get(k, at)
        text[start:start + len(site)] = site if k % 2 == 0 else su.revcomp(site)
        at += 300
    text[2000], text[TILE + 40] = "N", "Y"
    blob = tb.fasta_of(["".join(text)])
    queries = [guide, tb.mutate(rng, guide, 2), tb.random_text(rng, 29)]
    return blob, queries, bu.brute_force(lu.parse([blob]), "N" * 29, queries, (0, 29), 3, 3, 3)


@functools.lru_cache(maxsize=None)
def inner_case():
    """L = 26 with a PAM on both sides, span (3, 20): g0 > 0 meets r = 3.  5 000 bases in two records."""
    rng = np.random.default_rng(2626)
    guide = tb.random_text(rng, G)
    text = list(tb.random_text(rng, 5000))
    at = 120
    for k, (b, i) in enumerate([(b, i if b else 0) for b in ALL_B for i in (1, G - 1 - max(-b, 0))]):
        site = "TT" + "ACGT"[k % 4] + tb.bulged(guide, b, i, rng) + "ACGT"[(k + 1) % 4] + "GG"
        text[at:at + len(site)] = site if k % 2 == 0 else su.revcomp(site)
        at += 330
    text[2600] = "S"
    text = "".join(text)
    blob = tb.fasta_of([text[:4090], text[4090:]])
    queries = ["NNN" + guide + "NNN", "NNN" + tb.mutate(rng, guide, 1) + "NNN", "N" * 26, "NNN" + tb.random_text(rng, G) + "NNN"]
    return blob, queries, bu.brute_force(lu.parse([blob]), "TTN" + "N" * 20 + "NGG", queries, (3, G), 3, 3, 3)


def test_the_wide_and_the_inner_case_have_every_bulge():
    _, _, (off, rows, prof) = wide_case()
    mine = rows[rows["query"] == 0]
    assert set(mine["bulge"].tolist()) == set(ALL_B) and set(mine["strand"].tolist()) == {0, 1}
    assert {TILE - 33, TILE - 1} <= set(mine["pos"][mine["bulge"] == 3].tolist()) and prof.shape == (3, 7, 4)
    assert {1, 14, 28} <= set(mine["at"][mine["bulge"] > 0].tolist()) and int(mine["at"][mine["bulge"] == -3].max()) == 25
    _, _, (off, rows, prof) = inner_case()
    mine = rows[rows["query"] == 0]
    for strand in (0, 1):
        assert set(mine["bulge"][mine["strand"] == strand].tolist()) == set(ALL_B)
    assert int(mine["at"][mine["bulge"] == -3].max()) == G - 1 - 3 and 1 in set(mine["at"][mine["bulge"] == -3].tolist())
    assert prof.shape == (4, 7, 4) and int(off[4] - off[3]) == 0 and (prof[2].sum(axis=1) > 0).all()


@gpu
def test_windows_of_32_bases_on_random_text():
    blob, queries, want = wide_case()
    tb.check_bulges([blob], "N" * 29, queries, (0, 29), 3, 3, 3, want=want)
    check_device_and_capacity(blob, "N" * 29, queries, (0, 29), 3, 3, 3, want)


@gpu
def test_a_span_inside_the_pattern_with_three_rna_bases():
    blob, queries, want = inner_case()
    tb.check_bulges([blob], "TTN" + "N" * 20 + "NGG", queries, (3, G), 3, 3, 3, want=want)
