"""The world of tests/test_handle_sequences.py, pinned on the CPU: every shape's premise from the oracle and from pruned_model,
every kind of guide present, the walk that takes every ordered pair of shapes, and the model of a handle's state on the sequences
whose outcome the source spells out.  No GPU."""
import numpy as np
import pytest

import handle_sequences_util as hs
import pruned_model as pm


@pytest.fixture(scope="module", params=hs.WIDTHS)
def world(request, tmp_path_factory):
    return hs.world(request.param, tmp_path_factory)


def test_constants_of_the_slots_are_those_of_the_replays():
    """kSlotHits = kReplayLds and kSlotHitsWide = kMidHits (issl_device.hpp says so in comments; the world relies on it), the
    placement counts are those of the issue's table, and both rings hold 64 batches."""
    c = hs.constants()
    assert c["kSlotHits"] == c["SLOT_HITS"] and c["kSlotHitsWide"] == c["MID_HITS"] and c["kSlotHits"] < c["kSlotHitsWide"]
    assert (c["kFineWays"], c["kFineWays2"]) == (13, 67) and c["kRing"] == c["kSpanRing"] == 64
    assert pm.SMALL_PAIRS == 512


def test_the_index_is_small_and_the_centres_have_their_rows(world):
    assert 20_000 <= len(world.sites) <= 60_000
    names = list(world.rows)
    centres = np.array([world.centre[k] for k in names], dtype=np.uint64)
    assert list(world.counts(centres, 4)) == [sum(world.rows[k]) for k in names]
    assert len(world.zero) == 64 and len(np.unique(world.low)) > 5000


def test_every_premise_holds(world):
    wanted = {"small", "small_d5", "over_small", "below_capacity", "above_capacity", "above_first", "whole_buckets", "clean", "one_above",
              "widen", "above_mid", "zero_hits", "one_guide", "repeated", "n0", "no_exit", "exits"}
    assert {s.premise for s in world.shapes} == wanted
    for shape in world.shapes:
        world.check_premise(shape)
    # the table of the issue, row by row
    by = world.by_name
    assert [by[k].dist for k in ("small_d2", "small_d4", "small_d5")] == [2, 4, 5]
    assert by["d6"].dist == 6 and by["noprune"].prune == 0
    assert {(s.entry, s.premise) for s in world.shapes if s.entry != "score"} == {
        (e, p) for e in ("dump_hits", "offtargets", "offtarget_profile") for p in ("widen", "clean")}
    for method in hs.METHODS:
        assert any(s.method == method and s.thr == 0.0 and s.premise == "no_exit" for s in world.shapes)
        assert any(s.method == method and s.thr == 75.0 and s.premise in ("exits", "widen") for s in world.shapes)
    # (and | 75.0 is the widening batch: it has the exits too)
    w = by["widen"]
    cnt = world.counts(w.guides, 4)
    kept = world.kept(w.guides, 4, 75.0, "and")
    assert (kept[cnt > world.c["SLOT_HITS"]] < cnt[cnt > world.c["SLOT_HITS"]]).all()
    growth = {s.name for s in world.tagged("growth")}
    assert growth == {"small_d5", "big1500", "big5000", "widen", "dump_many"} and len(world.tagged("ordinary")) == 3


def test_every_kind_of_guide_occurs(world):
    kinds = world.guide_kinds()
    assert all(v > 0 for v in kinds.values()), kinds


def test_expected_answers_are_cached_and_read_only(world):
    shape = world.by_name["widen"]
    a = world.expected(shape)
    assert world.expected(shape) is a and not a[0].flags.writeable
    assert world.expected(world.by_name["n0"])[0].shape == (0,)
    hits = world.expected(world.by_name["dump_many"])
    assert hits.shape[1] == 6 and len(hits) == world.counts(shape.guides, 4).sum()


@pytest.mark.parametrize("k", [1, 2, 3, 7, 33])
def test_eulerian_walk_takes_every_ordered_pair_once(k):
    walk = hs.eulerian_walk(k)
    assert len(walk) == k * k + 1 and walk[0] == walk[-1]
    pairs = list(zip(walk, walk[1:]))
    assert len(set(pairs)) == k * k and set(pairs) == {(i, j) for i in range(k) for j in range(k)}


def test_handle_model_on_the_sequences_the_source_spells_out(world):
    """finish_batches: a lane turns lean after a batch without a guide beyond kSlotHits hits and runs the next batch that has
    one twice; more than an eighth of such guides widens the slots, for good; max_dist 5 takes the plan's arrays from 13 to 67
    placements; capacities only grow."""
    c, by = world.c, world.by_name
    m = hs.HandleModel(world, "sorted")
    assert m.keys() == {"ws_cap_guides": 0, "ws_slot_width": 0, "ws_fine_ways": 0, "ws_lean": 0}
    assert m.call(by["n0"]) == 0 and m.keys()["ws_cap_guides"] == 0
    assert m.call(by["general"]) == 1
    assert m.keys() == {"ws_cap_guides": 1024, "ws_slot_width": c["kSlotHits"], "ws_fine_ways": 13, "ws_lean": 1}
    assert m.call(by["one_above"]) == 2 and m.keys()["ws_lean"] == 0 and m.keys()["ws_slot_width"] == c["kSlotHits"]
    assert m.call(by["one_above"]) == 1
    assert m.call(by["clean"]) == 1 and m.keys()["ws_lean"] == 1
    assert m.call(by["widen"]) == 2 and m.keys()["ws_slot_width"] == c["kSlotHitsWide"]
    assert m.call(by["small_d5"]) == 1 and m.keys()["ws_fine_ways"] == 67 and m.keys()["ws_lean"] == 1
    assert m.call(by["big1500"]) == 1 and m.keys()["ws_cap_guides"] == 1500
    assert m.call(by["big5000"]) == 2 and m.keys()["ws_cap_guides"] == 5000    # (it holds the many-hit centres)
    assert m.call(by["big1500"]) == 1 and m.keys()["ws_cap_guides"] == 5000 and m.keys()["ws_slot_width"] == c["kSlotHitsWide"]
    assert m.call(by["dump_clean"]) == 1 and m.keys()["ws_lean"] == 0           # (no slots in a dump: the lane is not lean after it)
    assert m.call(by["clean"]) == 1 and m.call(by["offtargets_many"]) == 1      # the counting call took the retry, the listing call none
    # a handle without slots, one that is never lean, the list-order image
    m = hs.HandleModel(world, "sorted", hit_slots=0)
    assert [m.call(by[k]) for k in ("clean", "widen")] == [1, 1] and m.keys()["ws_slot_width"] == c["kSlotHits"] and m.keys()["ws_lean"] == 0
    m = hs.HandleModel(world, "sorted", lean_tail=0)
    assert [m.call(by[k]) for k in ("clean", "widen")] == [1, 1] and m.keys()["ws_slot_width"] == c["kSlotHitsWide"]
    m = hs.HandleModel(world, "list", hit_slots=2)
    assert m.call(by["small_d5"]) == 1 and m.keys()["ws_fine_ways"] == 0 and m.keys()["ws_slot_width"] == c["kSlotHitsWide"]
    assert m.pruned(by["small_d5"]) == 0
    m = hs.HandleModel(world, "compact")
    assert [m.pruned(by[k]) for k in ("small_d2", "small_d4", "small_d5", "d6", "noprune", "n0")] == [1, 2, 3, 0, 0, 0]
    assert m.small_path(by["small_d4"]) and not m.small_path(by["over_small"]) and not m.small_path(by["small_d5"])
    assert not m.small_path(by["small_d4"], small_bin=0)
