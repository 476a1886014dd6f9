"""The fixtures of tests/test_replay_many_hits.py, checked with the CPU oracle alone: every row of many_hit_util.ROWS has
exactly the hits per slice it was laid out for and the property that takes it into its branch of k_replay_mid /
k_replay_big (the kernels' id groups restated in numpy), and the thresholds chosen from the oracle put a walk's end into
each of the four places the GPU tests want.  A failure here is a fixture regression, not a kernel's."""
import numpy as np
import pytest

import many_hit_util as mh
from many_hit_util import ROW, ROWS


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return mh.main_case(tmp_path_factory)


@pytest.fixture(scope="module")
def rows(case):
    """Per row: the oracle's hits of its centre at max_dist 4, threshold 0 (columns guide, slice, pos, id, dist, occ)."""
    hits = case.hits("centres", "and", 0.0)
    return {r[0]: hits[hits[:, 0] == i] for i, r in enumerate(ROWS)}


def _slice0(rows, name):
    h = rows[name]
    return h[h[:, 1] == 0, 3]


def test_the_constants_are_the_sources():
    src = mh.source_constants()
    for name in ("REPLAY_LDS", "MID_HITS", "MID_SLICE", "MID_DIRECT", "BIG_SMALL", "BIG_BUILDS", "HEAD_RUN", "PREFIX_SINGLE", "SCAN_CHUNK"):
        assert src[name] == getattr(mh, name), name
    assert src["HEAD_MAX_IS_MIN_OF_4_THREADS_AND_LDS"]
    assert mh.head_max(256) == 1024 and mh.head_max(1024) == 4096


def test_neighbourhood_counts_by_brute_force():
    """The constructor itself, without the oracle: first exactly matching slice of every site, by arithmetic."""
    rng = np.random.default_rng(3)
    centre = int(mh.far_apart_centres(1, rng, a_at_4=[0])[0])
    for shape in ("spread", "piled", "piled+outliers"):
        counts = [700, 5, 0, 33, 64]
        near = mh.neighbourhood(centre, counts, shape, rng)
        d = mh.mismatches(near, centre)
        assert d.min() >= 1 and d.max() <= 4
        x = near ^ np.uint64(centre)
        exact = np.stack([((x >> np.uint64(8 * s)) & np.uint64(0xFF)) == 0 for s in range(5)], axis=1)
        assert np.bincount(np.argmax(exact, axis=1), minlength=5).tolist() == counts and exact.any(axis=1).all()
    fill = mh.filler_between(centre, 5000, rng)
    key, ckey = mh.text_order_key(fill), mh.text_order_key(np.array([centre], dtype=np.uint64))[0]
    assert len(fill) > 4900 and (mh.mismatches(fill, centre) > 4).all() and (key > ckey).all()
    first_outlier = (int(ckey) | (3 << 30)) & ~((1 << 30) - 1)   # position 4 is bits 30..31 of the key; the centre has A there
    assert (key < np.uint64(first_outlier)).all()


def test_every_row_has_its_hits_per_slice(case, rows):
    for i, (name, counts, shape, n_fill, _) in enumerate(ROWS):
        h = rows[name]
        assert len(h) == sum(counts), name                                              # the exact total
        assert np.bincount(h[:, 1], minlength=5).tolist() == counts, name               # the exact per-slice counts
        assert h[:, 4].min() >= 1 and h[:, 4].max() <= 4, name                          # the centre itself is not a site
        for s in range(5):                                                              # scoring order: ids ascend inside a slice
            ids = h[h[:, 1] == s, 3].astype(np.int64)
            assert (np.diff(ids) > 0).all(), (name, s)
        assert set(mh.SPECIAL_SMALL) <= set(h[:, 5].tolist()) and set(mh.SPECIAL_BIG) <= set(h[:, 5].tolist()), name
    # the batch: every centre three times, and once moved by a substitution in slice 0
    per_guide = np.bincount(case.hits("guides", "and", 0.0)[:, 0], minlength=len(case.guides))
    n = len(ROWS)
    totals = np.array([sum(r[1]) for r in ROWS])
    assert per_guide[:n].tolist() == totals.tolist()
    assert sorted(per_guide[2 * n:].tolist()) == sorted(np.repeat(totals, 2).tolist())
    assert (per_guide[n:2 * n] < totals).all() and (per_guide[n:2 * n] > 0).all()   # (what had four substitutions is out of reach)
    few = np.bincount(case.hits("few", "and", 0.0)[:, 0], minlength=len(case.few))
    assert few.max() <= 8 and (few == 0).any() and (few > 0).any()


def test_every_row_reaches_its_branch(rows):
    """Row -> branch, from the oracle's ids and the kernels' grouping restated in numpy (many_hit_util.id_groups,
    big_slice_plan)."""
    kernel = {r[0]: mh.replay_kernel(r[1]) for r in ROWS}
    # hits per guide: kReplayLds, kMidHits, kBigSmall
    assert len(rows["t512"]) == mh.REPLAY_LDS and kernel["t512"] == "wave"
    assert len(rows["t513"]) == mh.REPLAY_LDS + 1 and kernel["t513"] == "mid"
    assert [len(rows[n]) for n in ("t2047", "t2048", "t2049")] == [mh.MID_HITS - 1, mh.MID_HITS, mh.MID_HITS + 1]
    assert [kernel[n] for n in ("t2047", "t2048", "t2049")] == ["mid", "mid", "big256"]
    assert all(np.bincount(rows[n][:, 1]).max() <= mh.MID_SLICE for n in ("t2047", "t2048", "t2049"))   # (kMidHits alone decides)
    assert len(rows["big16384"]) == mh.BIG_SMALL and kernel["big16384"] == "big256"
    assert len(rows["big16385"]) == mh.BIG_SMALL + 1 and kernel["big16385"] == "big1024"
    # hits in one slice, k_replay_mid: kMidDirect, kMidSlice, the quarter branch, a late start
    for name, want in (("direct256", mh.MID_DIRECT), ("direct257", mh.MID_DIRECT + 1), ("slice1024", mh.MID_SLICE), ("slice1025", mh.MID_SLICE + 1)):
        assert len(_slice0(rows, name)) == want and mh.REPLAY_LDS < len(rows[name]) <= mh.MID_HITS, name
    assert [kernel[n] for n in ("direct256", "direct257", "slice1024", "slice1025")] == ["mid", "mid", "mid", "big256"]
    for name in ("direct257", "slice1024"):   # spread ids: ranked inside the groups (no group holds more than a quarter)
        ids = _slice0(rows, name)
        assert mh.id_groups(ids)[1].max() * 4 <= len(ids), name
    ids = _slice0(rows, "quarter")
    shift, sizes = mh.id_groups(ids)
    assert kernel["quarter"] == "mid" and mh.MID_DIRECT < len(ids) <= mh.MID_SLICE
    assert sizes.max() * 4 > len(ids) and np.count_nonzero(sizes) >= 3 and shift > 0     # max group > len / 4
    assert len(ids) > 512                                                               # ... and rank_against_all<4>, not <2>
    assert kernel["late"] == "mid" and len(_slice0(rows, "late")) == 40 and np.bincount(rows["late"][:, 1]).tolist()[1:3] == [3, 2]
    assert mh.MID_DIRECT < np.bincount(rows["late"][:, 1])[3] <= mh.MID_SLICE
    # hits in one slice, k_replay_big<256, 2048>
    p256, p257 = mh.big_slice_plan(_slice0(rows, "head256"), 256), mh.big_slice_plan(_slice0(rows, "head257"), 256)
    assert kernel["head256"] == kernel["head257"] == "big256"
    assert len(_slice0(rows, "head256")) == 256 and p256["groups"] == 0 and p256["head"] == 0          # len > THREADS is false
    assert len(_slice0(rows, "head257")) == 257 and p257["groups"] > 0                                   # ... true: groups counted
    lds = mh.BIG_BUILDS[256]
    a, b = mh.big_slice_plan(_slice0(rows, "lds2048"), 256), mh.big_slice_plan(_slice0(rows, "lds2049"), 256)
    assert kernel["lds2048"] == kernel["lds2049"] == "big256"
    assert len(_slice0(rows, "lds2048")) == lds and a["head"] >= mh.HEAD_RUN and len(a["runs"]) == 1    # head, then the rest sorted in LDS
    assert len(_slice0(rows, "lds2049")) == lds + 1 and b["head"] >= mh.HEAD_RUN and b["group_order"] and not a["group_order"]
    assert b["runs"] == [(b["head"], lds + 1 - b["head"], False)]                       # head, group order, ONE run from g_done on
    r = mh.big_slice_plan(_slice0(rows, "runs256"), 256)
    assert kernel["runs256"] == "big256" and r["head"] >= mh.HEAD_RUN and len(r["runs"]) >= 3 and r["runs"][0][0] == r["head"]
    assert not any(x[2] for x in r["runs"]) and sum(x[1] for x in r["runs"]) + r["head"] == 5000
    assert min(a["head"], b["head"]) > 256                                              # cnt > THREADS: rank_sort_slice<4>
    ids = _slice0(rows, "network")
    plan = mh.big_slice_plan(ids, 256)
    assert kernel["network"] == "big256" and mh.id_groups(ids)[1].max() > lds                           # max group > 2048
    assert [r for r in plan["runs"] if r[2]] == [(0, int(mh.id_groups(ids)[1][0]), True)] and plan["head"] == 0
    assert len(plan["runs"]) >= 2                                                       # and a run behind the network's
    ids = _slice0(rows, "headskip")
    plan = mh.big_slice_plan(ids, 256)
    assert kernel["headskip"] == "big256" and plan["groups"] == 1 and plan["head"] == 0
    assert mh.head_max(256) < plan["first_group"] <= lds                                # first group > kHeadMax: counted, not walked
    assert len(plan["runs"]) >= 2 and plan["runs"][0] == (0, plan["first_group"], False)  # runs from group 0: g_done stays 0
    assert np.count_nonzero(mh.id_groups(ids)[1][1:]) >= 2                              # at least 2 non-empty groups behind it
    # ... and k_replay_big<1024, 7680>
    lds = mh.BIG_BUILDS[1024]
    a, b = mh.big_slice_plan(_slice0(rows, "lds7680"), 1024), mh.big_slice_plan(_slice0(rows, "lds7681"), 1024)
    assert kernel["lds7680"] == kernel["lds7681"] == "big1024"
    assert len(_slice0(rows, "lds7680")) == lds and a["head"] >= mh.HEAD_RUN and len(a["runs"]) == 1
    assert len(_slice0(rows, "lds7681")) == lds + 1 and b["head"] >= mh.HEAD_RUN and b["group_order"] and not a["group_order"]
    assert b["runs"] == [(b["head"], lds + 1 - b["head"], False)]
    r = mh.big_slice_plan(_slice0(rows, "runs1024"), 1024)
    assert kernel["runs1024"] == "big1024" and r["head"] >= mh.HEAD_RUN and len(r["runs"]) >= 3 and r["runs"][0][0] == r["head"]
    assert not any(x[2] for x in r["runs"]) and sum(x[1] for x in r["runs"]) + r["head"] == 17000
    h = rows["twoheads"]
    assert kernel["twoheads"] == "big1024"
    for s in (0, 1):
        plan = mh.big_slice_plan(h[h[:, 1] == s, 3], 1024)
        assert np.count_nonzero(h[:, 1] == s) > mh.MID_SLICE and mh.HEAD_RUN <= plan["head"] < np.count_nonzero(h[:, 1] == s), s
    p0, p1 = (mh.big_slice_plan(h[h[:, 1] == s, 3], 1024) for s in (0, 1))
    assert (p0["groups"], p0["head"]) != (p1["groups"], p1["head"])                     # state that would show if it were carried over
    # every kernel has several rows
    assert sorted(set(kernel.values())) == ["big1024", "big256", "mid", "wave"]


def test_the_chosen_thresholds_end_walks_in_all_four_places(case):
    chosen, table = mh.choose_thresholds(case)
    assert set(chosen) == set(mh.SITUATIONS) and chosen["none"] == 0.0
    for sit in mh.SITUATIONS[:3]:
        got = [row for (row, thr), s in table.items() if thr == chosen[sit] and s == sit]
        assert got, "fixture error: no row ends its walk in situation '%s'" % sit
    # the kept counts behind the choice are the oracle's: an exit leaves hits unscored, threshold 0 none
    full = np.bincount(case.hits("centres", "and", 0.0)[:, 0], minlength=len(ROWS))
    for sit in mh.SITUATIONS[:3]:
        kept = np.bincount(case.hits("centres", "and", chosen[sit])[:, 0], minlength=len(ROWS))
        assert (kept <= full).all() and (kept < full).any()
    # the 1024-thread build takes part: a walk of one of its rows ends behind its head, in the first slice or later
    assert any(s in ("first_run", "later") and mh.replay_kernel(ROWS[ROW[row]][1]) == "big1024" and thr in chosen.values()
               for (row, thr), s in table.items())


def test_prefix_fixture(tmp_path_factory):
    case = mh.prefix_case(tmp_path_factory)
    hits = case.hits("pool", "and", 0.0)
    per_guide = np.bincount(hits[:, 0], minlength=len(case.pool))
    for i, (name, counts, _, _, _) in enumerate(mh.PREFIX_ROWS):
        assert np.bincount(hits[hits[:, 0] == i, 1], minlength=5).tolist() == counts, name
    assert [mh.replay_kernel(r[1]) for r in mh.PREFIX_ROWS] == ["mid", "big256", "big256"]
    assert mh.PREFIX_ROWS[1][1][0] > mh.MID_SLICE and sum(mh.PREFIX_ROWS[1][1]) <= mh.MID_HITS      # handed on by k_replay_mid
    filler = per_guide[len(mh.PREFIX_ROWS):]
    assert filler.max() <= 8 and np.count_nonzero(filler) >= 2048 and (filler == 0).any()           # no or few hits
    for n in (mh.PREFIX_SINGLE - 1, mh.PREFIX_SINGLE):   # m = n + 1 on both sides of the one-workgroup prefix sum
        guides, which = mh.prefix_batch(case, n, 9)
        assert len(guides) == n and np.array_equal(guides, case.pool[which])
        many = np.flatnonzero(which < len(mh.PREFIX_ROWS))
        for at in (0, 7, 8, mh.SCAN_CHUNK - 1, mh.SCAN_CHUNK, n - 1):
            assert at in many
        run = np.arange(5 * 8192 + 64, 5 * 8192 + 72)
        assert run[0] % 8 == 0 and np.isin(run, many).all()                                          # eight counts of ONE thread
        assert len(many) > 2048                                                                      # longer than k_replay_mid's grid
        assert np.count_nonzero(which[many] == 1) > 600                                              # ... a third of it handed-on guides
        grouped = np.add.reduceat(per_guide[which], np.arange(0, n, mh.SCAN_CHUNK))
        assert len(grouped) == 128 and (grouped > 0).all()                                           # hit_slots 0: no chunk's sum is 0
