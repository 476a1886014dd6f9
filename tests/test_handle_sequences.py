"""One resident handle, mixed call sequences, every call against the CPU oracle.

A production handle -- the resident server, an in-process caller -- keeps one issl_index for hours and sends it pages of any size,
max_dist, method and entry point in any order.  What the handle carries from one batch to the next (csrc/issl_pipeline.cpp:
ensure_workspace, enqueue_batch, finish_batches; the counters the kernels leave for each other) is pinned here by varying what
came BEFORE a call: every ordered pair of call shapes in steady state, every pair of allocation-changing shapes on a fresh handle,
seeded random walks with option changes, asynchronous sequences on 1, 2 and 3 lanes, and pages through one resident server.

The shapes, their premises and the model of the handle's state are in tests/handle_sequences_util.py and are pinned without a GPU
in tests/test_handle_sequences_model.py.  Bits and bytes: no tolerance anywhere.  The ws_* keys of issl_index_get_option and
issl_stats::scan_launches / pruned prove that a sequence reached the state it names."""
import ctypes as C
import os
import pathlib
import subprocess
import time

import numpy as np
import pytest

import crackling_amd as ca
import handle_sequences_util as hs
from crackling_amd._lib import lib, check
from crackling_amd.scorer import OFFTARGET_DTYPE, _method_code
from test_offtarget_report import _check_csr, _cols, _profile_of, _scores_from

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
COMBOS = [(layout, width) for width in hs.WIDTHS for layout in hs.LAYOUTS]
WS_KEYS = ("ws_cap_guides", "ws_slot_width", "ws_fine_ways", "ws_cap_chunks", "ws_cap_fitems", "ws_lean",
           "ws_scan_verified", "ws_scan_lds_buffers", "ws_scan_raw_top", "ws_raw_chunks")
CAPACITIES = ("ws_cap_guides", "ws_fine_ways", "ws_cap_chunks", "ws_cap_fitems")


@pytest.fixture(scope="module", params=COMBOS, ids=["%s-w%d" % c for c in COMBOS])
def combo(request, tmp_path_factory):
    layout, width = request.param
    return layout, hs.world(width, tmp_path_factory)


def _open(world, layout, **options):
    ix = ca.IsslIndex.open(world.path)
    # (expect_guides: a whole-suite run may ask for the workspace to be prepared beside the upload -- not here, where the keys
    # are read before the first batch)
    for key, value in {"expect_guides": 0, **hs.LAYOUTS[layout], **options}.items():
        ix.set_option(key, value)
    assert all(ix.get_option(k) == 0 for k in WS_KEYS)   # nothing scored, no device yet
    ix.upload(0)
    assert ix.get_option("is_sorted") == (0 if layout == "list" else 1) and ix.get_option("is_compact") == (1 if layout == "compact" else 0)
    assert all(ix.get_option(k) == 0 for k in WS_KEYS)   # before the first batch
    return ix


def _keys(ix):
    return {k: ix.get_option(k) for k in WS_KEYS}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_PROFILES = {}


def _profile_want(world, shape):
    key = (world.width, shape.name)
    if key not in _PROFILES:
        hits = world.expected(shape)[0]
        _PROFILES[key] = _profile_of(hits[:, 0], hits[:, 4], hits[:, 5], shape.n)
    return _PROFILES[key]


def _call(ix, shape, observe=None):
    """The shape's entry point.  observe: called after every LIBRARY call (issl_dump_hits and issl_offtargets are called for
    the count, then for the list); without it the package's own wrappers make the calls."""
    sigs, n = shape.guides, shape.n
    if shape.entry == "score":
        out = ix.score(sigs, shape.dist, shape.thr, shape.method)
    elif shape.entry == "offtarget_profile":
        out = ix.offtarget_profile(sigs, shape.dist)
    elif observe is None:
        return ix.dump_hits(sigs, shape.dist, shape.thr, shape.method) if shape.entry == "dump_hits" else ix.offtargets(sigs, shape.dist)
    elif shape.entry == "dump_hits":
        cnt = C.c_size_t()
        args = (ix._h, sigs.ctypes.data, n, shape.dist, shape.thr, _method_code(shape.method))
        check(lib.issl_dump_hits(*args, None, 0, C.byref(cnt)))
        observe()
        out = np.empty((cnt.value, 6), dtype=np.uint32)
        if cnt.value:
            check(lib.issl_dump_hits(*args, out.ctypes.data, cnt.value, C.byref(cnt)))
            observe()
        return out
    else:
        offsets = np.zeros(n + 1, dtype=np.uint64)
        cnt = C.c_size_t()
        args = (ix._h, sigs.ctypes.data, n, shape.dist, offsets.ctypes.data)
        check(lib.issl_offtargets(*args, None, 0, C.byref(cnt)))
        observe()
        recs = np.empty(cnt.value, dtype=OFFTARGET_DTYPE)
        if cnt.value:
            check(lib.issl_offtargets(*args, recs.ctypes.data, cnt.value, C.byref(cnt)))
            observe()
        return offsets, recs
    if observe is not None:
        observe()
    return out


def _compare(world, shape, got, ctx):
    """Every output of the call against the oracle's: scores as 64-bit patterns, hit lists and records element by element."""
    want = world.expected(shape)
    if shape.entry == "score":
        assert np.array_equal(_bits(got[0]), _bits(want[0])), ("MIT", ctx)
        assert np.array_equal(_bits(got[1]), _bits(want[1])), ("CFD", ctx)
    elif shape.entry == "dump_hits":
        assert got.shape == want.shape and np.array_equal(got, want), ("hits", ctx)
    elif shape.entry == "offtargets":
        offsets, recs = got
        hits, mit, cfd = want
        _check_csr(offsets, recs, shape.n)
        assert np.array_equal(_cols(recs), hits[:, [0, 1, 3, 4, 5]]), ("records", ctx)
        assert np.array_equal(recs["site"], world.sites[recs["id"]]), ("sites", ctx)
        gmit, gcfd = _scores_from(offsets, recs)   # the terms added up in record order: the reference's sums at threshold 0
        assert np.array_equal(_bits(gmit), _bits(mit)) and np.array_equal(_bits(gcfd), _bits(cfd)), ("terms", ctx)
    else:
        sites, occs = got
        ref = _profile_want(world, shape)
        assert np.array_equal(sites, ref[0]) and np.array_equal(occs, ref[1]), ("profile", ctx)


def _step(ix, world, model, shape, ctx):
    """One call with the shape's `prune`, its outputs against the oracle, and after every library call of it the ws_* keys and
    the statistics against the model: capacities only grow, guide capacity / slot width / placements / lean state are what the
    model says, and the batch ran twice exactly where a retry is predicted -- the lane was lean and the batch holds a guide beyond
    kSlotHits hits, the raw buffer overflowed (ws_cap_chunks rose), or the item list was too short on the one-workgroup path
    (ws_cap_fitems rose; the general path scans whole buckets that once: pruned = 0)."""
    ix.set_option("prune", shape.prune)
    plan = model.plan(shape)
    # (the handle's own knobs, wherever they come from: a whole-suite run may force any of them in the environment)
    small_bin, raw_chunks, fine_items = (ix.get_option(k) for k in ("small_bin", "raw_chunks", "fine_items"))
    state = {"before": _keys(ix), "i": 0, "stats": ix.stats()}
    total = int(world.counts(shape.guides, shape.dist).sum()) if shape.n else 0

    def observe():
        i, before, after, st = state["i"], state["before"], _keys(ix), ix.stats()
        state["i"], state["before"] = i + 1, after
        where = (ctx, "library call %d" % i, before, after, {k: st[k] for k in ("scan_launches", "pruned", "n_guides", "hits")})
        if shape.n == 0:   # an empty call returns before it touches the handle: state and statistics are the last call's
            assert after == before and st == state["stats"], where
            return
        assert st["n_guides"] == shape.n, where
        runs = model.batch(shape, plan[i])
        for k, v in model.keys().items():
            assert after[k] == v, (k, v, where)
        assert all(after[k] >= before[k] for k in CAPACITIES), where
        first_size = before["ws_cap_chunks"] or raw_chunks          # (a default handle sizes its first buffer from the launch: no overflow expected there)
        chunk_rise = bool(first_size) and after["ws_cap_chunks"] > first_size
        fit_rise = bool(fine_items) and after["ws_cap_fitems"] > max(before["ws_cap_fitems"], fine_items)
        mode = model.pruned(shape)
        if 0 < raw_chunks < 16 and before["ws_cap_chunks"] == 0 and total:   # fewer chunks than the scan waves own (16 per range): any noted candidate overflows
            assert chunk_rise, where
        if fine_items and mode and shape.n >= 64 and before["ws_cap_fitems"] <= fine_items:   # >= 64 x slices groups, 16 items
            assert fit_rise, where
        launches, pruned = runs, mode
        if chunk_rise or (fit_rise and model.small_path(shape, small_bin)):
            launches = 2
        elif fit_rise and runs == 1:   # (a batch that is run again for the lean tail's sake finds the enlarged list: pruned after all)
            pruned = 0
        if chunk_rise and fit_rise:   # (both knobs at once, one of them from the environment: the repeat with the longer list may overflow again)
            assert st["scan_launches"] in (2, 3), where
        else:
            assert st["scan_launches"] == launches, (launches, where)
        assert st["pruned"] == pruned, (pruned, where)
        assert st["hits"] == total, where

    got = _call(ix, shape, observe)
    assert state["i"] == (len(plan) if shape.n else 1), ctx   # every library call of the entry point was looked at
    _compare(world, shape, got, ctx)


def _model_for(ix, world, layout):
    return hs.HandleModel(world, layout, hit_slots=ix.get_option("hit_slots"), lean_tail=ix.get_option("lean_tail"))


# ------------------------------------------------------------------------------------------------
# a. every transition in steady state
# ------------------------------------------------------------------------------------------------

def test_every_ordered_pair_of_shapes_on_one_handle(combo):
    """An Eulerian circuit of the complete digraph on the shapes: k * k + 1 calls on ONE handle, every shape behind every shape
    (itself included) at least once, every call against the oracle and against the model of the handle's state."""
    layout, world = combo
    shapes = world.shapes
    walk = hs.eulerian_walk(len(shapes))
    assert len(walk) == len(shapes) ** 2 + 1
    ix = _open(world, layout)
    model = _model_for(ix, world, layout)
    try:
        prev = None
        for i, v in enumerate(walk):
            _step(ix, world, model, shapes[v], (layout, world.width, "call %d" % i, "%s after %s" % (shapes[v], prev)))
            prev = shapes[v]
        # (a whole-suite run may set ISSL_HIT_SLOTS=0 or ISSL_LEAN_TAIL=0 in the environment: the model follows the handle's options)
        assert ix.get_option("ws_slot_width") == (world.c["kSlotHitsWide"] if model.hit_slots else world.c["kSlotHits"])
        assert ix.get_option("ws_cap_guides") == max(s.n for s in shapes) and ix.get_option("ws_fine_ways") == (0 if layout == "list" else 67)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# b. every first-time growth
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knob", ["default", "raw_chunks", "fine_items"])
def test_every_pair_of_growth_shapes_on_a_fresh_handle(combo, knob):
    """The shapes that change an allocation -- the two batches above the guide capacity, max_dist 5 (13 -> 67 placements), the
    widening batch, issl_dump_hits (d_hitrec) -- as A, B, A on a fresh handle for every ordered pair, on a default handle, on one
    that starts with a raw buffer of 7 chunks (every first batch overflows it and is run again) and on one whose item list
    starts with 16 items (the one-workgroup path asks for the batch again, the general path scans whole buckets that once)."""
    layout, world = combo
    growth = world.tagged("growth")
    options = {"default": {}, "raw_chunks": {"raw_chunks": 7}, "fine_items": {"fine_items": 16}}[knob]
    for a in growth:
        for b in growth:
            ix = _open(world, layout, **options)
            model = _model_for(ix, world, layout)
            try:
                for i, shape in enumerate((a, b, a)):
                    _step(ix, world, model, shape, (layout, world.width, knob, "%s, %s, %s" % (a, b, a), "step %d" % i))
                keys = _keys(ix)
                assert keys["ws_cap_guides"] == max(a.n, b.n, hs.INITIAL_GUIDES)
                if layout != "list":
                    assert keys["ws_fine_ways"] == (67 if 5 in (a.dist, b.dist) else 13)
                    if knob == "fine_items":
                        assert keys["ws_cap_fitems"] > 16
                if knob == "raw_chunks":
                    assert keys["ws_cap_chunks"] >= 1024 + 16
            finally:
                ix.close()


# ------------------------------------------------------------------------------------------------
# c. seeded random walks
# ------------------------------------------------------------------------------------------------

WALK_CALLS = 200
WALK_OPTIONS = {"prune": (-1, 0, 1), "hit_slots": (0, 1, 2), "lean_tail": (0, 1), "small_bin": (0, 1), "item_guides": (8, 64, 512),
                "scan_blocks": (64, 300, 1024, 4096), "scan_threads": (256, 768, 1024), "scan_generic": (0, 1), "tail_shapes": (0, 1)}


def _walk_entry(rng, world):
    """(shape name, option change or None) of the next step."""
    change = None
    if rng.random() < 0.3:
        key = list(WALK_OPTIONS)[int(rng.integers(0, len(WALK_OPTIONS)))]
        change = (key, int(WALK_OPTIONS[key][int(rng.integers(0, len(WALK_OPTIONS[key])))]))
    return world.shapes[int(rng.integers(0, len(world.shapes)))].name, change


def _replay(ix, world, entry, ctx):
    """One step of a walk: the option change, then the call (with the handle's `prune`, not the shape's), against the oracle."""
    name, change = entry
    if change is not None:
        ix.set_option(*change)
    shape = world.by_name[name]
    _compare(world, shape, _call(ix, shape), ctx)
    st = ix.stats()
    assert st["scan_launches"] <= 2 and (st["n_guides"] == shape.n or shape.n == 0), (ctx, st["scan_launches"])


def test_seeded_random_walks(combo):
    """200 calls per walk over all shapes; between calls, with probability 0.3, one scheduling or path option of the live handle
    changes.  Every call against the oracle; no call takes more than two launches.  ISSL_SEQ_TRIALS / ISSL_SEQ_SEED run longer
    campaigns (profiles/handle_sequences_campaign.txt).  A failure names the seed, the step and the steps up to it: _replay()
    over that list on a fresh handle of the same layout and width repeats it."""
    layout, world = combo
    trials = int(os.environ.get("ISSL_SEQ_TRIALS", 2))
    seed = int(os.environ.get("ISSL_SEQ_SEED", 20260))
    for trial in range(trials):
        rng = np.random.default_rng([seed, trial, world.width, list(hs.LAYOUTS).index(layout)])
        ix = _open(world, layout)
        log = []
        try:
            for step in range(WALK_CALLS):
                log.append(_walk_entry(rng, world))
                try:
                    _replay(ix, world, log[-1], (layout, world.width))
                except (AssertionError, ca.IsslError) as e:
                    raise AssertionError("random walk failed: seed %d trial %d layout %s width %d step %d: %s\nsteps so far: %r"
                                         % (seed, trial, layout, world.width, step, e, log)) from e
        finally:
            ix.close()
        print("walk ok: seed %d trial %d %s w%d, %d calls, %d option changes" % (seed, trial, layout, world.width, len(log),
                                                                               sum(1 for _, c in log if c)))


# ------------------------------------------------------------------------------------------------
# d. asynchronous sequences
# ------------------------------------------------------------------------------------------------

ASYNC_ORDERS = {
    "many_hit_after_lean": ("clean", "zero_hits", "small_d4", "widen", "clean", "above_mid", "one_guide"),
    "above_capacity_between_small": ("small_d4", "big1500", "small_d2", "big5000", "one_guide", "general"),
    "dist5_between_dist4": ("small_d4", "small_d5", "general", "small_d5", "over_small", "d6", "small_d4"),
}
WRAP_CYCLE = ("small_d2", "one_guide", "zero_hits", "repeated", "small_d4", "clean", "one_above")


def _async_sequence(ix, world, names, ctx):
    """Enqueue the batches back to back, one finish(); False: the same batches again (include/issl_hip.h).  Every batch's
    outputs against the oracle.  -> rounds it took."""
    import torch
    bufs = []
    for name in names:
        shape = world.by_name[name]
        d_g = torch.from_numpy(shape.guides.view(np.int64).copy()).cuda()
        d_m = torch.full((shape.n,), -7.0, dtype=torch.float64, device="cuda:0")
        bufs.append((shape, d_g, d_m, torch.full_like(d_m, -7.0)))
    torch.cuda.synchronize()
    for rounds in range(1, 7):
        for shape, d_g, d_m, d_c in bufs:
            ix.score_device_async(d_g, d_m, d_c, shape.dist, shape.thr, shape.method)
        if ix.finish():
            break
    else:
        raise AssertionError(("the batches kept asking to be enqueued again", ctx))
    assert ix.stats()["n_batches"] == len(bufs), ctx
    for i, (shape, _, d_m, d_c) in enumerate(bufs):
        assert shape.entry == "score"
        _compare(world, shape, (d_m.cpu().numpy(), d_c.cpu().numpy()), (ctx, "batch %d" % i, shape.name))
    return rounds


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_asynchronous_sequences(combo, lanes):
    """Batches of different shapes in flight together on 1, 2 and 3 lanes: a many-hit batch behind lean ones (finish() says
    "again" once where the lane had turned lean), batches above the guide capacity between small ones (the workspace is
    reallocated between batches in flight), max_dist 5 between max_dist 4 (the plan's arrays grow alone); then all of it in one go,
    and more than 64 batches per lane and per handle, so that the span ring and the event ring wrap."""
    layout, world = combo
    c = world.c
    ix = _open(world, layout, lanes=lanes, prune=1)
    try:
        lean_on = ix.get_option("lean_tail") == 1 and ix.get_option("hit_slots") != 0
        # (a whole-suite run that forces short buffers on every handle adds repeats of its own: results only then)
        exact = ix.get_option("raw_chunks") == 0 and ix.get_option("fine_items") == 0
        for order, names in ASYNC_ORDERS.items():
            rounds = _async_sequence(ix, world, names, (layout, world.width, lanes, order))
            if order == "many_hit_after_lean" and lanes == 1 and exact:   # fresh handle: not lean when enqueued, nothing to repeat
                assert rounds == 1
        if lanes == 1:   # (two workspaces take the batches in turn: which of them grew depends on the count so far)
            assert ix.get_option("ws_cap_guides") == world.by_name["big5000"].n
            assert ix.get_option("ws_fine_ways") == (0 if layout == "list" else 67)
        # a clean sequence: every lane turns lean; then the many-hit batches behind lean ones: finish() says "again", once
        # (test_lean_retry_ends_on_two_workspaces_with_an_odd_number_of_batches)
        rounds = _async_sequence(ix, world, ("clean", "small_d4") * 2, (layout, world.width, lanes, "clean"))
        assert rounds == 1 or not exact
        if lean_on:
            assert ix.get_option("ws_lean") == 1
        rounds = _async_sequence(ix, world, ASYNC_ORDERS["many_hit_after_lean"], (layout, world.width, lanes, "lean, then many hits"))
        if lean_on and exact:
            assert rounds == 2, rounds
        if lean_on:
            assert lanes != 1 or ix.get_option("ws_lean") == 0
        everything = sum(ASYNC_ORDERS.values(), ())
        _async_sequence(ix, world, everything, (layout, world.width, lanes, "all orders in one go"))
        # both rings wrap: an event pair per batch (scan_events = 1), more than kRing batches, more than kSpanRing per lane
        ix.set_option("scan_events", 1)
        n_wrap = (c["kSpanRing"] + 6) * (1 if lanes == 1 else 2)
        assert n_wrap > c["kRing"]
        names = tuple(WRAP_CYCLE[i % len(WRAP_CYCLE)] for i in range(n_wrap))
        _async_sequence(ix, world, names, (layout, world.width, lanes, "rings wrap"))
        # and the synchronous entry points behind all that
        for name in ("dump_many", "offtargets_clean", "profile_many", "widen", "n0"):
            shape = world.by_name[name]
            _compare(world, shape, _call(ix, shape), (layout, world.width, lanes, "synchronous", name))
    finally:
        ix.close()


@pytest.mark.parametrize("lanes", [2, 3])
def test_lean_retry_ends_on_two_workspaces_with_an_odd_number_of_batches(combo, lanes):
    """Regression, the shortest sequence: two workspaces take the asynchronous batches in turn, by a count that runs on over
    every finish().  Both lean; then clean, many-hit, clean -- an odd number.  finish() says "again" (the many-hit batch met a
    lean workspace) and the repeat lands the other way round: the many-hit batch on the workspace that saw only clean batches.
    That one must not be lean for the repeat -- it was, the first workspace turned lean again over ITS clean batches, and
    finish() said "again" for ever."""
    layout, world = combo
    ix = _open(world, layout, lanes=lanes, prune=1)
    try:
        # (a whole-suite run may switch the lean tail off in the environment, or force short buffers that add repeats of their own:
        # then the sequence only has to END -- _async_sequence gives up after six rounds -- with the oracle's results)
        lean_on = ix.get_option("lean_tail") == 1 and ix.get_option("hit_slots") != 0
        exact = ix.get_option("raw_chunks") == 0 and ix.get_option("fine_items") == 0
        rounds = _async_sequence(ix, world, ("clean", "clean"), (layout, world.width, lanes, "both lean"))
        assert rounds == 1 or not exact
        assert ix.get_option("ws_lean") == (1 if ix.get_option("hit_slots") else 0)   # (the flag; the lean_tail option decides at the enqueue)
        rounds = _async_sequence(ix, world, ("clean", "widen", "clean"), (layout, world.width, lanes, "odd"))
        assert rounds == (2 if lean_on else 1) or not exact
        rounds = _async_sequence(ix, world, ("clean", "widen", "clean"), (layout, world.width, lanes, "odd again"))
        assert rounds <= 2 or not exact
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# e. the resident server
# ------------------------------------------------------------------------------------------------

SERVER_PAGES = ((8, "clean"), (8, "small_d2"), (4, "general"), (8, "widen"), (8, "clean"), (8, "big1500"), (4, "cfd_exits"), (4, "clean"),
                (8, "zero_hits"), (8, "small_d5"), (4, "above_mid"), (8, "one_guide"), (8, "avg_no_exit"), (4, "small_d4"))


def test_pages_of_every_kind_through_one_resident_server(tmp_path, tmp_path_factory):
    """One `isslScoreOfftargets --serve` process, fourteen pages through ISSL_SERVER: sizes 1 ... 1500, max_dist 2 ... 5, all
    five methods, thresholds 0 / 50 / 75, two indexes (8- and 4-bit slices) resident side by side; clean pages, a many-hit page,
    clean pages again.  Every page's stdout is, byte for byte, format_scores over the oracle's doubles."""
    exe = str(ROOT / "bin" / "isslScoreOfftargets")
    worlds = {w: hs.world(w, tmp_path_factory) for w in hs.WIDTHS}
    sock = str(tmp_path / "issl.sock")
    server = subprocess.Popen([exe, "--serve", sock], stderr=subprocess.PIPE)
    try:
        for _ in range(100):
            if os.path.exists(sock):
                break
            time.sleep(0.05)
        assert os.path.exists(sock)
        env = dict(os.environ, ISSL_SERVER=sock, ISSL_TIMING="1")
        seen = set()
        for i, (width, name) in enumerate(SERVER_PAGES):
            world = worlds[width]
            shape = world.by_name[name]
            assert shape.entry == "score"
            query = tmp_path / ("page%d.txt" % i)
            query.write_text("".join(s + "\n" for s in ca.decode_guides(shape.guides)))
            r = subprocess.run([exe, str(world.path), str(query), str(shape.dist), "%g" % shape.thr, shape.method], capture_output=True,
                               env=env, cwd=str(tmp_path), timeout=120)
            assert r.returncode == 0, (i, name, r.stderr.decode())
            mit, cfd = world.expected(shape)
            assert r.stdout.decode() == ca.format_scores(shape.guides, mit, cfd, shape.method), (i, width, name)
            assert (b'"resident": true' in r.stderr) == (width in seen), (i, r.stderr)
            seen.add(width)
        assert server.poll() is None
    finally:
        subprocess.run([exe, "--stop", sock], capture_output=True, timeout=60)
        try:
            server.wait(timeout=20)
        except subprocess.TimeoutExpired:
            server.kill()
    assert server.returncode == 0
