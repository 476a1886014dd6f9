"""The scan's distance tests on EVERY placement of mismatches: the neighbourhood of tests/neighbourhood_util.py -- one
centre, every set of up to four mismatching positions in each of the three kinds (low bit, high bit, both), a mixed family
out to six -- through every compiled threshold and budget of count_near / count_near12, both runtime comparators, the
short units' two and four fields and the previous-slice filter: hit lists row for row and MIT / CFD as 64-bit patterns
against the CPU oracle.  tests/test_neighbourhood_construction.py (no GPU) shows that the fixture holds what this module
relies on: every subset of the compared positions within the budget, per slice, class and kind.

One item is one (slice width, layout, max_dist); inside it the knobs that choose the code: pruned or whole buckets,
compiled or runtime threshold, short last units or full ones, the one-launch binning or the general one.

What this cannot see: a network that is too LAX (it accepts a count above the threshold) costs k_verify work and loses no
hit; raw_records of issl_stats bounds it in chunks only."""
import numpy as np
import pytest

import crackling_amd as ca
import neighbourhood_util as nu

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "sorted": {"sorted_layout": 1, "compact": 0, "host_cold": 0},
    "compact": {"compact": 1, "host_cold": 0, "keep_lists": 1},
    "list": {"sorted_layout": 0, "inline_sigs": 0, "host_cold": 0},
}
SORTED = ("sorted", "compact")
KNOBS = ("prune", "scan_generic", "tail_shapes", "small_bin")
DEFAULTS = (-1, 0, 1, 1)


def _write_index(path, sigs, occ, width):
    ix = ca.IsslIndex.build_from_sites(sigs, occ, slice_width=width)
    ix.write(path)
    ix.close()


@pytest.fixture(scope="module", params=[8, 4, 2])
def world(request, tmp_path_factory):
    w = nu.World(tmp_path_factory.mktemp("placements"), request.param, _write_index)
    yield w
    w.close()


@pytest.fixture(scope="module", params=list(LAYOUTS))
def device_index(request, world):
    ix = ca.IsslIndex.open(world.path)
    for key, value in LAYOUTS[request.param].items():
        ix.set_option(key, value)
    ix.upload(0)
    assert ix.get_option("is_sorted") == (request.param in SORTED) and ix.get_option("is_compact") == (request.param == "compact")
    yield ix, request.param
    ix.close()


def _sweep(layout, dist):
    """(prune, scan_generic, tail_shapes, small_bin) of one item."""
    out = []
    if layout in SORTED and dist <= 5:
        for generic in (0, 1):
            for tail in (1, 0):
                for small in ((0, 1) if dist <= 4 else (1,)):
                    out.append((1, generic, tail, small))
    out += [(0, 0, 1, 1), (0, 1, 1, 1)]
    return out


@pytest.mark.parametrize("dist", range(8))
def test_every_placement_against_the_oracle(world, device_index, dist):
    (ix, layout), n = device_index, world.n
    try:
        for knobs in _sweep(layout, dist):
            for knob, value in zip(KNOBS, knobs):
                ix.set_option(knob, value)
            pruned = (0 if knobs[0] == 0 else 1 if dist <= 2 else 2 if dist <= 4 else 3)
            for batch, guides in n.batches.items():
                for thr in (0.0, 75.0):
                    where = (world.width, layout, dist, knobs, batch, thr)
                    wmit, wcfd, whits = world.want(batch, dist, thr)
                    hits = ix.dump_hits(guides, dist, thr, "and")
                    assert ix.stats()["pruned"] == pruned, where   # (a fall back to whole buckets is no pruned run)
                    if hits.shape != whits.shape or not np.array_equal(hits, whits):
                        pytest.fail("hit list differs from the oracle's: %r\n%s" % (where, _difference(hits, whits, guides, n.sigs)))
                    mit, cfd = ix.score(guides, dist, thr, "and")
                    assert ix.stats()["pruned"] == pruned, where
                    assert np.array_equal(mit.view(np.uint64), wmit.view(np.uint64)), ("MIT not bit-identical",) + where
                    assert np.array_equal(cfd.view(np.uint64), wcfd.view(np.uint64)), ("CFD not bit-identical",) + where
                    if batch == "A":   # eight copies of the centre: every field of a short unit's pass carried it
                        per_row = [hits[hits[:, 0] == g, 1:] for g in range(len(guides))]
                        assert all(np.array_equal(r, per_row[0]) for r in per_row[1:]), ("rows of batch A differ",) + where
                        assert (mit.view(np.uint64) == mit.view(np.uint64)[0]).all() and (cfd.view(np.uint64) == cfd.view(np.uint64)[0]).all(), where
    finally:
        for knob, value in zip(KNOBS, DEFAULTS):
            ix.set_option(knob, value)


def _difference(hits, whits, guides, sigs):
    """The first rows that one list has and the other has not, with the placement: which positions of the site differ from
    the guide, and by which xor."""
    def keyed(h):
        return {tuple(int(x) for x in r) for r in h}
    got, want = keyed(hits), keyed(whits)
    lines = ["%d rows, oracle %d; columns: guide, slice, position in bucket, site, distance, occurrences" % (len(hits), len(whits))]
    for name, rows in (("missing", sorted(want - got)), ("unexpected", sorted(got - want))):
        for r in rows[:8]:
            x = int(guides[r[0]]) ^ int(sigs[r[3]]) if r[0] < len(guides) and r[3] < len(sigs) else 0
            placed = [(p, (x >> (2 * p)) & 3) for p in range(20) if (x >> (2 * p)) & 3]
            lines.append("%s %r: guide ^ site as (position, xor) %r" % (name, r, placed))
        if len(rows) > 8:
            lines.append("... and %d more %s" % (len(rows) - 8, name))
    return "\n".join(lines)
