"""GPU: a full survivor queue in all four genome-search kernels.  An all-N pattern admits every window on both strands, so
the first workgroup's queue holds all 2 x 4096 tags; the four units share the compaction that fills it and must return the
brute force of tests/search_util.py, each in its own row type, for every split of the queries among the four waves and
the groups of four."""
import numpy as np
import pytest

import crackling_amd as ca
import bulge_variant_util as bvu
import search_util as su
import variant_util as vu

pytestmark = pytest.mark.gpu

TILE = 4096  # kPosPerBlock: text positions per workgroup
L, MAX_DIST = 20, 2
CASES = {"all_n": ("N" * L, (0, L)), "ngg": ("N" * 17 + "NGG", (0, 17))}  # pattern, the span the bulge forms take
COUNTS = (1, 3, 4, 5, 16, 17)  # the edges of the four-way wave split and of the query group of 4


def pool_of(text):
    """17 queries read off the text, strands alternating (an odd query is the reverse complement of its window): windows
    the NGG pattern admits on that strand, one across the tile boundary and the last of the text among them."""
    plus = [p for p in range(len(text) - L + 1) if text[p + 18:p + 20] == "GG"]
    minus = [p for p in range(len(text) - L + 1) if text[p:p + 2] == "CC"]
    near = lambda ps, x: min(ps, key=lambda p: abs(p - x))
    places = [plus[0], minus[0], near(plus, TILE - 10), near(minus, TILE - 10), plus[-1], minus[-1]]
    places += [near(plus if k % 2 == 0 else minus, 450 * (k - 5)) for k in range(6, 16)] + [len(text) - L]
    assert len(places) == 17
    return [text[p:p + L] if k % 2 == 0 else su.revcomp(text[p:p + L]) for k, p in enumerate(places)]


@pytest.fixture(scope="module")
def full_queue():
    """The genome, and per case the brute force for the whole pool: the first n queries own its first offsets[n] rows."""
    rng = np.random.default_rng(8193)
    text = "".join("ACGT"[c] for c in rng.integers(0, 4, size=2 * TILE + 1))
    queries = pool_of(text)
    want = {}
    for name, (pattern, _) in CASES.items():
        off, rows, prof = su.brute_force([(b"rec0", text.encode())], pattern, queries, MAX_DIST)
        assert set(rows["strand"].tolist()) == {0, 1} and len(rows) >= 16  # (NGG does not admit the text's last window)
        want[name] = (off, rows, prof)
    cand = su.candidates([(b"rec0", text.encode())], CASES["all_n"][0])[1]
    assert (cand < TILE).sum() == 2 * TILE  # the first tile's queue is full
    with ca.Genome.open([b">rec0\n%s\n" % text.encode()]) as g:
        yield g, queries, want


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_a_full_queue_gives_the_brute_force_in_every_unit(full_queue, case, n):
    g, queries, want = full_queue
    pattern, span = CASES[case]
    off, rows, prof = want[case]
    queries, off, rows, prof = queries[:n], off[:n + 1], rows[:int(off[n])], prof[:n]
    as_variants = vu.from_plain(rows, L)
    per_query = np.diff(off.astype(np.int64))
    for got, want_rows, got_prof in (
            (g.search(pattern, queries, MAX_DIST), rows, g.search_profile(pattern, queries, MAX_DIST)),
            (g.search_variants(pattern, queries, MAX_DIST, 0), as_variants, g.search_variants_profile(pattern, queries, MAX_DIST, 0)),
            (g.search_bulges(pattern, queries, span, MAX_DIST, 0, 0), rows, g.search_bulges_profile(pattern, queries, span, MAX_DIST, 0, 0)),
            (g.search_bulges_variants(pattern, queries, span, MAX_DIST, 0, 0, 0), bvu.from_variants(as_variants),
             g.search_bulges_variants_profile(pattern, queries, span, MAX_DIST, 0, 0, 0))):
        got_off, got_rows = got
        assert got_off.tobytes() == off.tobytes()
        assert len(got_rows) == len(want_rows) and got_rows.tobytes() == want_rows.tobytes()
        got_prof = got_prof.reshape(n, MAX_DIST + 1)  # the bulge forms: one bulge, b = 0
        assert got_prof.tobytes() == prof.tobytes() and np.array_equal(got_prof.sum(axis=1).astype(np.int64), per_query)
