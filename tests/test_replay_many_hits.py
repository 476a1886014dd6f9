"""The many-hit side of the scoring tail -- k_replay_mid, both builds of k_replay_big, the grouping pass that feeds them --
at every size it switches at, as tests/test_replay_network.py does for k_replay: one guide per row of many_hit_util.ROWS
(hits per guide around 512, 2048 and 16384; hits in one slice around 256, 1024, 2048 and 7680; ids piled up in one of the
256 id groups; a head pass that is counted and not walked; two head passes in one guide), every one of them three times in
the batch and once more after a substitution in slice 0.  Doubles bit for bit and hit lists in order against the CPU
oracle, for five methods, thresholds that end the walk inside the head pass, in the first run behind it, later, and
nowhere (chosen from the ORACLE's kept counts: many_hit_util.choose_thresholds), hit slots off, narrow and wide, three
image layouts and both scan modes; and many-hit guides in batches on both sides of the one-workgroup prefix sum.

That every row reaches the branch it is there for is asserted from the oracle's ids in tests/test_many_hit_construction.py
(no GPU needed); test_the_fixture_is_what_the_kernels_see repeats the counts with the GPU's own hit list.

A workgroup that takes a second guide after one it handed on: the main batch lists fewer many-hit guides than the replays
have workgroups (every workgroup takes one), so this is test_many_hit_guides_beyond_the_one_workgroup_prefix_sum's part
here -- 700 handed-on guides among 2100 listed -- beside tests/test_gpu_parity.py::
test_replay_workgroups_that_take_several_mid_size_guides, which stays as it is."""
import numpy as np
import pytest

import crackling_amd as ca
import many_hit_util as mh
from many_hit_util import ROWS
from test_layouts import _open as open_layout   # (sets the options of test_layouts.LAYOUTS[name])
from test_offtarget_report import _cols as report_columns

pytestmark = pytest.mark.gpu

METHODS = ["and", "or", "avg", "mit", "cfd"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return mh.main_case(tmp_path_factory)


def _open(path, hit_slots=None, layout=None):
    ix = open_layout(path, layout) if layout else ca.IsslIndex.open(path)
    if hit_slots is not None:
        ix.set_option("hit_slots", hit_slots)
    return ix.upload(0)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("mit", "cfd")):
        bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        assert len(bad) == 0, (what, name, bad[:10].tolist())


def test_the_fixture_is_what_the_kernels_see(case):
    """The exact totals and per-slice counts of every row, from the oracle and from issl_dump_hits; the four exit
    situations occur (from the oracle's kept counts alone: a fixture error otherwise, never a skip)."""
    ohits = case.hits("guides", "and", 0.0)
    ix = _open(case.path)
    try:
        hits = ix.dump_hits(case.guides, 4, 0.0, "and")
    finally:
        ix.close()
    for name, h in (("oracle", ohits), ("gpu", hits)):
        for i, row in enumerate(ROWS):
            assert np.bincount(h[h[:, 0] == i, 1], minlength=5).tolist() == row[1], (name, row[0])
    assert (hits[:, 5] >= 0xFFFFFF).any() and (hits[:, 5] == 255).any()   # saturated occurrence counts among the scored hits
    chosen, table = mh.choose_thresholds(case)
    for sit in mh.SITUATIONS[:3]:
        assert any(s == sit for (row, thr), s in table.items() if thr == chosen[sit]), "fixture error: nothing ends in '%s'" % sit
    assert chosen["none"] == 0.0 and len(set(chosen.values())) == 4


@pytest.mark.parametrize("hit_slots", [0, 1, 2])
@pytest.mark.parametrize("situation", mh.SITUATIONS)
@pytest.mark.parametrize("method", METHODS)
def test_sums_match_the_oracle_bit_for_bit(case, method, situation, hit_slots):
    """(The thresholds were read off method and's kept counts; under the other methods the same thresholds end the walks
    elsewhere -- the oracle says where, the kernels must agree.)"""
    thr = mh.choose_thresholds(case)[0][situation]
    want = case.scores("guides", method, thr)
    ix = _open(case.path, hit_slots)
    try:
        for rep in range(2):   # (the second batch of a handle may run with wide slots: most of these guides are beyond the narrow ones)
            _same(ix.score(case.guides, 4, thr, method), want, (method, thr, hit_slots, rep))
    finally:
        ix.close()


def test_one_handle_from_many_hit_batches_to_lean_ones_and_back(case):
    """hit_slots = 1 on one handle: a batch of many-hit guides alone (more than an eighth of it beyond 512 hits: the handle
    moves to 2048 slots), a mixed batch, few-hit guides only (the lane turns lean), the mixed batch again (mispredicted:
    run again with the whole tail inside the call)."""
    per_guide = np.bincount(case.hits("centres", "and", 0.0)[:, 0], minlength=len(ROWS))
    assert np.count_nonzero(per_guide > mh.REPLAY_LDS) * 8 > len(ROWS)
    assert np.bincount(case.hits("few", "and", 0.0)[:, 0], minlength=len(case.few)).max() <= mh.REPLAY_LDS
    ix = _open(case.path, 1)
    try:
        for thr in (75.0, 0.0):
            for step, key in enumerate(("centres", "mixed", "few", "mixed")):
                _same(ix.score(getattr(case, key), 4, thr, "and"), case.scores(key, "and", thr), (thr, step, key))
    finally:
        ix.close()


@pytest.mark.parametrize("situation", mh.SITUATIONS)
@pytest.mark.parametrize("method", METHODS)
def test_hit_lists_match_the_oracle_in_order(case, method, situation):
    """The DUMP builds and hit_terms: with the early exit (three places) and without."""
    thr = mh.choose_thresholds(case)[0][situation]
    ix = _open(case.path)
    try:
        assert np.array_equal(ix.dump_hits(case.guides, 4, thr, method), case.hits("guides", method, thr)), (method, thr)
    finally:
        ix.close()


@pytest.mark.parametrize("hit_slots", [0, 1, 2])
def test_off_target_report_of_the_same_guides(case, hit_slots):
    """k_profile's BIG path: the records of the report are the oracle's hits at threshold 0."""
    ohits = case.hits("guides", "and", 0.0)
    ix = _open(case.path, hit_slots)
    try:
        offsets, recs = ix.offtargets(case.guides, 4)
        assert np.array_equal(np.diff(offsets).astype(np.int64), np.bincount(ohits[:, 0], minlength=len(case.guides)))
        assert np.array_equal(report_columns(recs), ohits[:, [0, 1, 3, 4, 5]])
    finally:
        ix.close()


@pytest.mark.parametrize("prune", [-1, 0])
@pytest.mark.parametrize("layout", ["sorted", "compact", "list"])
def test_layouts_and_scan_modes(case, layout, prune):
    """The default sorted image, the compact one, and list order (keys are list positions there, not site ids)."""
    chosen = mh.choose_thresholds(case)[0]
    ix = _open(case.path, layout=layout)
    try:
        ix.set_option("prune", prune)
        for situation in mh.SITUATIONS:
            thr = chosen[situation]
            _same(ix.score(case.guides, 4, thr, "and"), case.scores("guides", "and", thr), (layout, prune, thr))
            assert np.array_equal(ix.dump_hits(case.guides, 4, thr, "and"), case.hits("guides", "and", thr)), (layout, prune, thr)
    finally:
        ix.close()


@pytest.mark.parametrize("hit_slots", [0, 1])
@pytest.mark.parametrize("n", [mh.PREFIX_SINGLE - 1, mh.PREFIX_SINGLE])
def test_many_hit_guides_beyond_the_one_workgroup_prefix_sum(tmp_path_factory, n, hit_slots):
    """n + 1 counts on both sides of 2^18: k_prefix_single (the many-hit guide list in guide order), or the three-kernel
    prefix sum, whose k_prefix_apply reserves list entries with one atomic per thread of eight counts -- the list is in
    no particular order and may differ between runs, the scores may not.  Three many-hit guides (k_replay_mid's, one it
    hands on, k_replay_big's) at the places many_hit_util.prefix_places names, 2100 entries in all: more than k_replay_mid
    has workgroups.  Without hit slots every hit of the filler goes through the prefix sum too."""
    case = mh.prefix_case(tmp_path_factory)
    guides, which = mh.prefix_batch(case, n, 9)
    ix = _open(case.path, hit_slots)
    try:
        for thr in (75.0, 0.0):
            omit, ocfd = case.scores("pool", "and", thr)
            first = ix.score(guides, 4, thr, "and")
            _same(first, (omit[which], ocfd[which]), (n, hit_slots, thr, "first"))
            again = ix.score(guides, 4, thr, "and")
            _same(again, first, (n, hit_slots, thr, "again"))
    finally:
        ix.close()
