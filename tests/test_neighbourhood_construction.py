"""The fixture of tests/test_scan_placements.py, checked on the CPU: the site set is what neighbourhood_util says, the
oracle's hit lists are the brute-force ones row for row, the sites realise EVERY subset of mismatching positions that a
distance test of the scan can meet within its budget -- per slice, class and kind of mismatch, over the positions the
kernels compare --, the guides reach short last units of every shape in both classes, and batch A has short units to fill.
A failure here is a fixture regression, not a kernel's."""
from math import comb

import numpy as np
import pytest

import crackling_amd as ca
import neighbourhood_util as nu
import pruned_model as pm

WIDTHS = [8, 4, 2]


def _write_index(path, sigs, occ, width):
    ix = ca.IsslIndex.build_from_sites(sigs, occ, slice_width=width)
    ix.write(path)
    ix.close()


@pytest.fixture(scope="module", params=WIDTHS)
def world(request, tmp_path_factory):
    w = nu.World(tmp_path_factory.mktemp("neighbourhood"), request.param, _write_index)
    yield w
    w.close()


# ---- the positions the kernels compare, relative to the first position of slice s (mod 20) ------------------------------
# Sorted layouts ("Other slice widths"; scan_word / scan_word_sorted_narrow, fine_order): the pruned
# scan leaves the successor unit (the four positions behind the slice) in memory and counts TWELVE positions: with 8-bit
# slices all the others; with 4-bit (2-bit) slices the previous slice's two (one) and the ten (eleven) behind the
# successor unit -- the two (three) before the previous slice are in no plane.  The whole-bucket scan of a sorted image
# counts those twelve and the successor unit: SIXTEEN.
TWELVE = {8: [8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19],
          4: [-2, -1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
          2: [-1, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]}
SUCCESSOR = {8: [4, 5, 6, 7], 4: [2, 3, 4, 5], 2: [1, 2, 3, 4]}
# List-order images (scan_word): the first sixteen of the positions outside the slice, ascending; what is LEFT OUT, by slice
LIST_ORDER_LEFT_OUT = {8: {s: [] for s in range(5)},
                       4: {**{s: [18, 19] for s in range(9)}, 9: [16, 17]},
                       2: {**{s: [17, 18, 19] for s in range(17)}, 17: [16, 18, 19], 18: [16, 17, 19], 19: [16, 17, 18]}}


def twelve(s, width):
    return [(s * (width // 2) + o) % 20 for o in TWELVE[width]]


def sixteen_sorted(s, width):
    return [(s * (width // 2) + o) % 20 for o in SUCCESSOR[width] + TWELVE[width]]


def sixteen_list_order(s, width):
    return [p for p in range(20) if p not in nu.slice_positions(s, width) and p not in LIST_ORDER_LEFT_OUT[width][s]]


# the two stream words restated (issl_kernels.hpp), to read the lists above off them
def _gather_even16(x):
    return sum(((x >> (2 * i)) & 1) << i for i in range(16))


def _scan_word(sig, s, width):
    sh = width * s
    rem = ((sig & ((1 << sh) - 1)) | ((sig >> (sh + width)) << sh)) & 0xFFFFFFFF
    return _gather_even16(rem) | (_gather_even16(rem >> 1) << 16)


def _scan_word_sorted_narrow(sig, s, width):
    sh = (width * (s + 1)) % 40
    a = ((sig >> sh) | (sig << (40 - sh))) & ((1 << 40) - 1)
    prev = (a >> (40 - 2 * width)) & ((1 << width) - 1)
    mid = (a >> 8) & ((1 << (24 - width)) - 1)
    rem = (a & 0xFF) | (prev << 8) | (mid << (8 + width))
    return _gather_even16(rem) | (_gather_even16(rem >> 1) << 16)


def _word_positions(word, s, width):
    """Position held by each of the word's sixteen places (low plane; the high plane must agree)."""
    held = {}
    for p in range(20):
        low, high = word(1 << (2 * p), s, width), word(2 << (2 * p), s, width)
        assert high == low << 16
        if low:
            assert bin(low).count("1") == 1
            held[low.bit_length() - 1] = p
    assert sorted(held) == list(range(16))
    return [held[i] for i in range(16)]


def test_the_position_lists_are_the_stream_words():
    for width in WIDTHS:
        for s in range(40 // width):
            succ = nu.successor_positions(s, width)
            assert succ == [(s * (width // 2) + o) % 20 for o in SUCCESSOR[width]]
            assert sorted(_word_positions(_scan_word, s, width)) == sorted(sixteen_list_order(s, width))
            if width == 8:   # the sorted image keeps the same word; the pruned scan skips the successor slice's quad
                assert sorted(twelve(s, 8)) == sorted(set(_word_positions(_scan_word, s, 8)) - set(succ))
                assert sorted(sixteen_sorted(s, 8)) == sorted(sixteen_list_order(s, 8))
            else:            # quad 0: the successor unit; quads 1..3: the twelve, the previous slice's positions first
                held = _word_positions(_scan_word_sorted_narrow, s, width)
                assert held[:4] == succ and held[4:] == twelve(s, width)
                per = width // 2
                assert held[4:4 + per] == nu.slice_positions((s - 1) % (20 // per), width)
                assert held == sixteen_sorted(s, width)


def test_the_site_set():
    n = nu.fixture()
    assert len(n.sigs) == nu.N_SITES == len(np.unique(n.sigs))
    assert (np.diff(nu.text_order_key(n.sigs).astype(np.int64)) > 0).all()
    assert np.array_equal(n.occ, 1 + np.arange(nu.N_SITES) % 3)
    d = (nu.codes(n.sigs) != nu.codes(n.guides[:1])[0]).sum(axis=1)
    assert np.cumsum(np.bincount(d)).tolist() == nu.CUMULATIVE[2]   # (2-bit slices: every site within 19 is met)
    assert np.bincount(d)[1] == 3 * 20 and np.bincount(d)[5:].tolist() == [comb(20, 5), comb(20, 6)]   # 5, 6: the mixed family alone
    assert len(n.guides) == 11 == len(np.unique(n.guides))
    dist_to_sites = (nu.codes(n.sigs)[None, :, :] != nu.codes(n.guides)[:, None, :]).sum(axis=2)
    assert dist_to_sites.min() == 0 and dist_to_sites.max() == 10   # the rejecting side too
    # mutants that share slice 0 and the byte behind it with the centre (no substitution in the first 8 / 6 / 5 positions):
    # they ride in its passes; the others fall in neighbouring groups
    for width, sharing in ((8, 5), (4, 6), (2, 6)):
        lead = np.uint64((1 << (width + 8)) - 1)
        assert int((((n.guides[1:] ^ n.guides[0]) & lead) == 0).sum()) == sharing, width


def test_oracle_counts_of_the_centre(world):
    for dist, want in enumerate(nu.CUMULATIVE[world.width]):
        _, _, hits = world.want("C", dist, 0.0)
        assert len(hits) == want, (world.width, dist)
    _, _, hits = world.want("C", 7, 0.0)
    assert len(hits) == nu.CUMULATIVE[world.width][6]
    if world.width == 8:
        for dist, want in nu.BATCH_B_ROWS_WIDTH8.items():
            assert len(world.want("B", dist, 0.0)[2]) == want


@pytest.mark.parametrize("dist", range(8))
def test_oracle_hit_list_is_the_brute_force_one(world, dist):
    n = world.n
    _, _, hits = world.want("B", dist, 0.0)
    want = nu.brute_force(n.sigs, n.occ, n.guides, dist, world.width)
    assert hits.shape == want.shape and np.array_equal(hits, want), (world.width, dist)


def _up_to(masks, k):
    """The masks with at most k bits set (a few sites of the mixed family are of one kind too, at five and six positions)."""
    return masks[np.array([bin(int(m)).count("1") <= k for m in masks], dtype=bool)]


@pytest.mark.parametrize("width", WIDTHS)
def test_every_placement_within_the_budget_is_a_site(width):
    n = nu.fixture()
    full12 = {k: nu.subsets_up_to(12, k) for k in range(5)}
    full16 = {k: nu.subsets_up_to(16, k) for k in range(5)}
    for k in range(5):
        assert len(full12[k]) == sum(comb(12, j) for j in range(k + 1))
        assert len(full16[k]) == sum(comb(16, j) for j in range(k + 1))
    for s in range(40 // width):
        for v in (1, 2, 3):
            # the pruned scan: class 0 in the centre's own successor-byte group, class 1 in the groups one mismatch away
            seen = {cls: nu.placements_seen(n.sigs, n.centre, v, s, width, twelve(s, width), cls) for cls in (0, 1)}
            for dist in range(1, 5):
                for cls in range(pm.successor_tolerance(dist) + 1):
                    budget = dist - cls
                    assert np.array_equal(_up_to(seen[cls], budget), full12[budget]), (width, s, v, dist, cls)
            # whole buckets, on a sorted image and on a list-order one
            for positions in (sixteen_sorted(s, width), sixteen_list_order(s, width)):
                got = nu.placements_seen(n.sigs, n.centre, v, s, width, positions)
                for dist in range(1, 5):
                    assert np.array_equal(_up_to(got, dist), full16[dist]), (width, s, v, dist)


def _units_reached(n, width, max_dist, guides):
    """{(shape of the last unit, class)}, whether a group of several units is among them, and per slice the shapes the
    FIRST guide meets by class, over the groups that the pruned scan lets the guides visit."""
    tables = pm.site_tables(n.sigs, width)
    gc = pm._codes(guides)
    k = pm.successor_tolerance(max_dist)
    x = np.arange(256)[:, None] ^ np.arange(256)[None, :]
    diff = (x | (x >> 1)) & 0x55
    away = (diff & 1) + ((diff >> 2) & 1) + ((diff >> 4) & 1) + ((diff >> 6) & 1)
    seen, several, per_slice = set(), False, {}
    for s, sites in enumerate(tables):
        gv, gb = pm._slice_and_successor(gc, s, width)
        s1 = np.cumsum(sites, axis=1)
        s0 = s1 - sites
        for g, (value, byte) in enumerate(zip(gv, gb)):
            for other in np.flatnonzero((away[byte] <= k) & (sites[value] > 0)):
                units, _, shape = pm.group_units(s0[value, other], s1[value, other], s1[value, -1], 1)
                seen.add((int(shape), int(away[byte, other])))
                several |= int(units) > 1
                if g == 0:   # the first guide's own group, and the groups one mismatch away that it visits
                    per_slice.setdefault(s, {0: set(), 1: set(), 2: set()})[int(away[byte, other])].add(int(shape))
    return seen, several, per_slice


@pytest.mark.parametrize("width", WIDTHS)
def test_the_guides_reach_every_shape_in_both_classes(width):
    n = nu.fixture()
    seen, several, _ = _units_reached(n, width, 4, n.guides)
    assert seen >= {(shape, cls) for shape in (8, 16, 32) for cls in (0, 1)}, (width, seen)
    assert several or width == 2
    seen, _, _ = _units_reached(n, width, 2, n.guides)
    assert seen >= {(shape, 0) for shape in (8, 16, 32)} and all(cls == 0 for _, cls in seen), (width, seen)


@pytest.mark.parametrize("width", WIDTHS)
def test_batch_a_fills_short_units(width):
    """Eight copies of the centre in one group: where that group ends in a short unit, its passes carry the centre in every
    field.  With 8- and 4-bit slices the centre's OWN group has a short last unit in slice 0 and in other slices.  With
    2-bit slices its own group (a fifth position fixed: four times the sites) ends in a full unit in every slice, whatever
    the centre; there the short units it fills are those of groups one mismatch away, in several slices, from max_dist 3 on."""
    n = nu.fixture()
    assert len(n.batches["A"]) == 8 and (n.batches["A"] == n.guides[0]).all()
    _, _, met = _units_reached(n, width, 4, n.guides[:1])
    cls = 0 if width != 2 else 1
    short = [s for s, by_class in met.items() if by_class[cls] - {32}]
    assert (0 in short or width == 2) and len(short) >= 2, (width, met)
    if width == 2:
        assert all(by_class[0] == {32} for by_class in met.values())
