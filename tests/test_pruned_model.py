"""The models of tests/pruned_model.py against what can be known without a GPU: the host index's bucket table, the CPU
oracle's hit lists, a brute-force count, and groups worked out by hand."""
import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
import pruned_model as pm
from synth import random_sites, random_guides, text_order_key


@pytest.mark.parametrize("width", [8, 4, 2])
def test_tolerance_four_is_the_whole_bucket(width):
    sigs, occ = random_sites(50_000, seed=811)
    guides = random_guides(sigs, 400, seed=812)
    ix = ca.IsslIndex.build_from_sites(sigs, occ, slice_width=width)
    try:
        assert pm.planned_comparisons(sigs, guides, 4, width, k=4) == ix.count_candidates(guides)
    finally:
        ix.close()
    few = pm.planned_comparisons(sigs, guides, 2, width)
    some = pm.planned_comparisons(sigs, guides, 4, width)
    more = pm.planned_comparisons(sigs, guides, 5, width)
    assert 0 < few < some < more < pm.planned_comparisons(sigs, guides, 4, width, k=4)


@pytest.mark.parametrize("width", [8, 4, 2])
def test_fast_count_is_the_brute_force_count(width):
    rng = np.random.default_rng(5 + width)
    sites = rng.integers(0, 1 << 40, size=300, dtype=np.uint64)
    sites[100:] = (sites[100:] & ~np.uint64(0xFFFFF)) | (sites[7] & np.uint64(0xFFFFF))   # many share ten positions
    guides = np.concatenate([random_guides(sites, 60, seed=3), sites[:5]])
    s, g = np.repeat(sites, len(guides)), np.tile(guides, len(sites))
    for dist in range(6):
        assert pm.planned_comparisons(sites, guides, dist, width) == int(pm.visits(s, g, dist, width).sum()) > 0, dist


@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    """Sites around 100 centres with one to six substitutions, so that guides have hits at every distance, and 30 k random ones."""
    rng = np.random.default_rng(4242)
    centres = rng.integers(0, 1 << 40, size=100, dtype=np.uint64)
    near = centres.repeat(200)
    for k in range(6):
        where = rng.random(len(near)) < (1.0 if k == 0 else 0.6)
        near[where] ^= rng.integers(1, 4, size=int(where.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, 20, size=int(where.sum())).astype(np.uint64))
    sigs = np.unique(np.concatenate([near, rng.integers(0, 1 << 40, size=30_000, dtype=np.uint64)]))
    sigs = sigs[np.argsort(text_order_key(sigs), kind="stable")]
    occ = rng.integers(1, 4, size=len(sigs)).astype(np.uint32)
    guides = np.concatenate([centres, random_guides(sigs, 200, seed=4243)])
    return tmp_path_factory.mktemp("model"), sigs, occ, guides


@pytest.mark.parametrize("width", [8, 4, 2])
def test_every_hit_of_the_oracle_lies_where_the_rule_lets_its_guide_look(clustered, width):
    tmp, sigs, occ, guides = clustered
    path = tmp / f"clustered{width}.issl"
    ix = ca.IsslIndex.build_from_sites(sigs, occ, slice_width=width)
    ix.write(path)
    ix.close()
    oracle = ou.OracleIndex(path)
    try:
        for dist in range(6):
            hits = oracle.score(guides, dist, 0.0, "and", want_hits=True)[2]
            assert len(hits) > 50, dist   # (the guides do have neighbours)
            assert (hits[:, 4] == dist).any(), dist
            seen = pm.visits(sigs[hits[:, 3]], guides[hits[:, 0]], dist, width)
            assert seen.any(axis=1).all(), (dist, int((~seen.any(axis=1)).sum()))
            if width == 8 and dist in (3, 5):   # five slices: the rule is tight, one mismatch less behind the slice loses a hit
                assert not pm.visits(sigs[hits[:, 3]], guides[hits[:, 0]], dist, width, k=pm.successor_tolerance(dist) - 1).any(axis=1).all()
    finally:
        oracle.close()


def test_tolerance_and_small_batch_limit():
    assert [pm.successor_tolerance(d) for d in range(6)] == [0, 0, 0, 1, 1, 2]
    assert [pm.small_batch_limit(w, 4) for w in (8, 4, 2)] == [102, 51, 25] and pm.small_batch_limit(8, 5) == 0
    with pytest.raises(ValueError):
        pm.successor_tolerance(6)


# a group that starts its bucket and is `rest` long, in a bucket that goes on for 5000 candidates behind it
@pytest.mark.parametrize("rest,units,counted,shape", [
    (1, 1, 512, 8), (512, 1, 512, 8), (513, 1, 1024, 16), (1024, 1, 1024, 16), (1025, 1, 2048, 32), (2048, 1, 2048, 32),
    (2049, 2, 2048 + 512, 8), (2048 + 513, 2, 2048 + 1024, 16), (2048 + 1025, 2, 4096, 32), (3 * 2048, 3, 3 * 2048, 32)])
def test_units_of_a_group_by_hand(rest, units, counted, shape):
    assert tuple(int(x) for x in pm.group_units(0, rest, rest + 5000)) == (units, counted, shape)
    # without the short shapes every unit counts 2048
    assert tuple(int(x) for x in pm.group_units(0, rest, rest + 5000, tail_shapes=0)) == (units, 2048 * units, 32)


def test_units_of_groups_that_start_inside_a_lane_group_or_end_their_bucket():
    # [33, 40): covered from 32 on, span 8
    assert tuple(int(x) for x in pm.group_units(33, 40, 9000)) == (1, 512, 8)
    # [33, 545): span 513 although the group has 512 candidates
    assert tuple(int(x) for x in pm.group_units(33, 545, 9000)) == (1, 1024, 16)
    # [33, 2080): span 2048, one full unit and nothing behind it; one candidate more and a short unit follows
    assert tuple(int(x) for x in pm.group_units(33, 2080, 9000)) == (1, 2048, 32)
    assert tuple(int(x) for x in pm.group_units(33, 2081, 9000)) == (2, 2048 + 512, 8)
    # the bucket ends inside the last unit: [3980, 4100) of 4100 is covered from 3968 on, 132 candidates are left of the cap of 512
    assert tuple(int(x) for x in pm.group_units(3980, 4100, 4100)) == (1, 132, 8)
    assert tuple(int(x) for x in pm.group_units(3980, 4100, 4100, tail_shapes=0)) == (1, 132, 32)
    # ... and [100, 2300) of 2400: from 96 on one full unit, then 156 of the group and 100 of its neighbour
    assert tuple(int(x) for x in pm.group_units(100, 2300, 2400)) == (2, 2048 + 256, 8)
    got = pm.group_units(np.array([0, 33]), np.array([1, 545]), np.array([5001, 9000]))
    assert [list(map(int, x)) for x in got] == [[1, 1], [512, 1024], [8, 16]]


def test_unit_model_on_one_bucket_by_hand():
    """Slice 0 = AAAA: 40 sites with successor byte 5 and 600 with 6 (one position apart); the other twelve positions are A or C
    in the sites and G in the guide, so no other slice brings the guide and a site together."""
    rng = np.random.default_rng(9)
    free = np.unique(rng.integers(0, 1 << 12, size=3000, dtype=np.uint64))[:640]
    spread = np.zeros(640, dtype=np.uint64)
    for j in range(12):
        spread |= ((free >> np.uint64(j)) & np.uint64(1)) << np.uint64(2 * j)
    sites = (spread << np.uint64(16)) | (np.where(np.arange(640) < 40, 5, 6).astype(np.uint64) << np.uint64(8))
    guide = np.array([(0xAAAAAA << 16) | (6 << 8)], dtype=np.uint64)
    assert pm.planned_comparisons(sites, guide, 4, 8) == 640 and pm.planned_comparisons(sites, guide, 2, 8) == 600
    # byte 5: [0, 40) of 640, one unit of 512; byte 6: [40, 640), covered from 32 on, span 608: one unit of 1024 that the bucket ends in
    assert pm.unit_model(sites, guide, 4, 8) == (2, 512 + 608)
    assert pm.unit_model(sites, guide, 4, 8, tail_shapes=0) == (2, 640 + 608)
    assert pm.unit_model(sites, guide, 2, 8) == (1, 608)
    assert pm.unit_model(sites, guide, 5, 8) == (2, 640 + 608)            # max_dist 5: full shapes only
    nine = guide.repeat(9)
    assert pm.unit_model(sites, nine, 4, 8, item_guides=512) == (2, 9 * 1120)
    assert pm.unit_model(sites, nine, 4, 8, item_guides=8) == (4, 9 * 1120)      # two chunks of guides per group
    assert pm.unit_model(sites, nine, 4, 8, small_batch=True) == (18, 9 * 1120)  # every placement a group of its own
