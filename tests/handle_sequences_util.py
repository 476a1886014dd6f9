"""A small world for tests of a long-lived handle (tests/test_handle_sequences.py on the GPU, tests/test_handle_sequences_model.py
on the CPU): one index per slice width, a list of call SHAPES -- a call with everything that decides which path it takes --, what
the CPU oracle says about every shape (computed once, shared, never changed), and a model of the state an issl_index carries from
one batch to the next (csrc/issl_pipeline.cpp: ensure_workspace, enqueue_batch, finish_batches).

The index: random background (synth.random_sites) and neighbourhoods with exact hit counts (many_hit_util.neighbourhood) around
centres that lie far apart, so that a centre has exactly the hits of its row within four mismatches -- whatever the slice width:
a site within four substitutions of a 20-mer leaves at least one 8-bit slice (six 4-bit slices) untouched, so the reference finds
it once.  The sizes the kernels switch at come from the source (many_hit_util.source_constants)."""
import pathlib
import re

import numpy as np

import many_hit_util as mh
import pruned_model as pm
from synth import random_sites, text_order_key

ROOT = pathlib.Path(__file__).resolve().parent.parent
WIDTHS = (8, 4)
LAYOUTS = {"sorted": {}, "compact": {"compact": 1}, "list": {"sorted_layout": 0}}   # the options set before the upload
METHODS = ("mit", "cfd", "and", "or", "avg")
INITIAL_GUIDES = 1024     # ensure_workspace: the first allocation holds max(n, 1024) guides
N_BACKGROUND = 30_000


def constants():
    """kSlotHits, kSlotHitsWide, kMidHits, the two placement counts and the ring sizes, as the source states them."""
    c = mh.source_constants()
    src = ROOT / "crackling_amd" / "csrc"
    text = (src / "issl_device.hpp").read_text() + (src / "issl_index.hpp").read_text()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    return {"SLOT_HITS": c["REPLAY_LDS"], "MID_HITS": c["MID_HITS"], "kSlotHits": const("kSlotHits"), "kSlotHitsWide": const("kSlotHitsWide"),
            "kFineWays": const("kFineWays"), "kFineWays2": const("kFineWays2"), "kRing": const("kRing"), "kSpanRing": const("kSpanRing")}


def _even(total):
    return [total // 5 + (1 if s < total % 5 else 0) for s in range(5)]


def rows():
    """name -> hits per 8-bit slice of the centre's neighbourhood."""
    c = constants()
    s, m = c["SLOT_HITS"], c["MID_HITS"]
    return {"handful": [2, 1, 1, 1, 0], "below": _even(s - 1), "at": _even(s), "above": _even(s + 1), "between": _even((s + m) // 2),
            "mid_top": _even(m), "above_mid": _even(m + 1)}


class Shape:
    """One call.  entry: score | dump_hits | offtargets | offtarget_profile; prune: the `prune` option the call is made with
    (1: the pruned scan wherever the image and max_dist allow it, 0: whole buckets); tags: what the shape is in the lists below."""

    def __init__(self, name, entry, guides, dist=4, thr=75.0, method="and", prune=1, premise=None, tags=()):
        self.name, self.entry, self.guides = name, entry, np.ascontiguousarray(guides, dtype=np.uint64)
        self.guides.setflags(write=False)
        self.dist, self.thr, self.method, self.prune, self.premise, self.tags = dist, float(thr), method, prune, premise, tuple(tags)
        self.n = len(self.guides)

    def __repr__(self):
        return self.name


class World:
    def __init__(self, width, directory):
        import crackling_amd as ca
        import oracle_util as ou
        self.width, self.n_slices = width, 40 // width
        self.c = constants()
        rng = np.random.default_rng(9100 + width)
        self.rows = rows()
        names = list(self.rows)
        centres = mh.far_apart_centres(len(names), rng)
        self.centre = {name: centres[i] for i, name in enumerate(names)}
        sites, occ = [], []
        for name in names:
            near = mh.neighbourhood(self.centre[name], self.rows[name], "spread", rng)
            sites.append(near)
            occ.append(rng.integers(1, 4, size=len(near)).astype(np.uint32))
        bg, bg_occ = random_sites(N_BACKGROUND, 9200 + width)
        keep = np.isin(bg, mh.clear_of(bg, centres))
        self.background = bg[keep]
        sig = np.concatenate(sites + [self.background])
        occ = np.concatenate(occ + [bg_occ[keep]])
        sig, first = np.unique(sig, return_index=True)
        occ = occ[first]
        order = np.argsort(text_order_key(sig), kind="stable")
        self.sites, self.occ = sig[order], occ[order]
        self.path = pathlib.Path(directory) / ("world_w%d.issl" % width)
        ix = ca.IsslIndex.build_from_sites(self.sites, self.occ, slice_width=width)
        ix.write(self.path)
        ix.close()
        self.oracle = ou.OracleIndex(self.path)
        self._expected, self._counts = {}, {}
        # guides with few hits: background sites after 0..3 substitutions; guides without any: random 20-mers the oracle finds nothing for
        picks = self.background[rng.integers(0, len(self.background), size=5200)]
        for k in range(3):
            sub = rng.integers(1, 4, size=len(picks)).astype(np.uint64) << (2 * rng.integers(0, 20, size=len(picks))).astype(np.uint64)
            picks = np.where(rng.random(len(picks)) < 0.5, picks ^ sub, picks)
        self.low = picks
        cand = rng.integers(0, 1 << 40, size=400, dtype=np.uint64)
        self.zero = cand[self.counts(cand, 4) == 0][:64]
        self.shapes = self._make_shapes(rng)
        self.by_name = {s.name: s for s in self.shapes}
        assert len(self.by_name) == len(self.shapes)

    # -- the oracle's answers --------------------------------------------------------------------
    def counts(self, guides, dist):
        """Hits per guide before any early exit: the oracle's hit list at threshold 0.0 and the same max_dist."""
        key = (np.asarray(guides, dtype=np.uint64).tobytes(), dist)
        if key not in self._counts:
            _, _, hits = self.oracle.score(guides, dist, 0.0, "and", want_hits=True)
            self._counts[key] = np.bincount(hits[:, 0], minlength=len(guides))
            self._counts[key].setflags(write=False)
        return self._counts[key]

    def expected(self, shape):
        """score: (mit, cfd); dump_hits: the hit list; offtargets / offtarget_profile: (hit list at threshold 0, mit, cfd)."""
        if shape.name not in self._expected:
            if shape.n == 0:
                empty = np.empty(0, dtype=np.float64)
                want = (np.empty((0, 6), dtype=np.uint32), empty, empty) if shape.entry != "score" else (empty, empty)
                want = want[0] if shape.entry == "dump_hits" else want
            elif shape.entry == "score":
                want = self.oracle.score(shape.guides, shape.dist, shape.thr, shape.method)
            elif shape.entry == "dump_hits":
                want = self.oracle.score(shape.guides, shape.dist, shape.thr, shape.method, want_hits=True)[2]
            else:
                mit, cfd, hits = self.oracle.score(shape.guides, shape.dist, 0.0, "and", want_hits=True)
                want = (hits, mit, cfd)
            for a in (want if isinstance(want, tuple) else (want,)):
                a.setflags(write=False)
            self._expected[shape.name] = want
        return self._expected[shape.name]

    def kept(self, guides, dist, thr, method):
        """Hits per guide that the reference scores before it stops (all of them at threshold 0.0)."""
        _, _, hits = self.oracle.score(guides, dist, thr, method, want_hits=True)
        return np.bincount(hits[:, 0], minlength=len(guides))

    # -- the shapes --------------------------------------------------------------------------------
    def _make_shapes(self, rng):
        limit = pm.small_batch_limit(self.width, 4)
        c, low, zero = self.centre, self.low, self.zero
        many_centres = np.array([c[k] for k in ("above", "between", "mid_top", "above_mid")], dtype=np.uint64)
        many = rng.permutation(np.concatenate([many_centres, [c["handful"], c["below"], c["at"]], low[:13], zero[:4]]))   # 24 guides, 4 beyond the slots
        clean = np.concatenate([low[100:160], [c["handful"], c["below"], c["at"]], zero[:1]])                            # 64 guides, none beyond
        out = [
            Shape("small_d2", "score", low[:limit], 2, 75.0, "and", premise="small", tags=("ordinary",)),
            Shape("small_d4", "score", low[5:5 + limit], 4, 75.0, "and", premise="small", tags=("ordinary",)),
            Shape("small_d5", "score", low[9:9 + limit], 5, 75.0, "and", premise="small_d5", tags=("growth",)),
            Shape("over_small", "score", low[:limit + 1], 4, 75.0, "and", premise="over_small"),
            Shape("general", "score", low[200:900], 4, 75.0, "and", premise="below_capacity", tags=("ordinary",)),
            Shape("big1500", "score", low[:1500], 3, 50.0, "or", premise="above_capacity", tags=("growth",)),
            Shape("big5000", "score", np.concatenate([low[:4990], many_centres, zero[:6]]), 4, 75.0, "and", premise="above_first", tags=("growth",)),
            Shape("d6", "score", low[300:500], 6, 75.0, "and", premise="whole_buckets"),
            Shape("noprune", "score", low[400:700], 4, 75.0, "and", prune=0, premise="whole_buckets"),
            Shape("clean", "score", clean, 4, 0.0, "mit", premise="clean"),
            Shape("one_above", "score", np.concatenate([low[700:760], [c["above"], c["below"], c["at"]], zero[:2]]), 4, 75.0, "and", premise="one_above"),
            Shape("widen", "score", many, 4, 75.0, "and", premise="widen", tags=("growth",)),
            Shape("above_mid", "score", np.concatenate([low[800:809], [c["above_mid"]]]), 4, 0.0, "and", premise="above_mid"),
            Shape("zero_hits", "score", zero[:50], 4, 75.0, "and", premise="zero_hits"),
            Shape("one_guide", "score", [c["handful"]], 4, 75.0, "and", premise="one_guide"),
            Shape("repeated", "score", np.repeat(c["handful"], 33), 4, 0.0, "and", premise="repeated"),
            Shape("n0", "score", np.empty(0, dtype=np.uint64), 4, 75.0, "and", premise="n0"),
            Shape("dump_many", "dump_hits", many, 4, 0.0, "and", premise="widen", tags=("growth",)),
            Shape("dump_clean", "dump_hits", clean, 4, 75.0, "and", premise="clean"),
            Shape("offtargets_many", "offtargets", many, 4, 0.0, "and", premise="widen"),
            Shape("offtargets_clean", "offtargets", clean, 4, 0.0, "and", premise="clean"),
            Shape("profile_many", "offtarget_profile", many, 4, 0.0, "and", premise="widen"),
            Shape("profile_clean", "offtarget_profile", clean, 4, 0.0, "and", premise="clean"),
        ]
        for method in METHODS:   # every method with and without early exits, on the many-hit guides
            out.append(Shape("%s_no_exit" % method, "score", many, 4, 0.0, method, premise="no_exit"))
            if not (method == "and"):   # (and | 75.0 is "widen")
                out.append(Shape("%s_exits" % method, "score", many, 4, 75.0, method, premise="exits"))
        return out

    def tagged(self, tag):
        return [s for s in self.shapes if tag in s.tags]

    def reduced_shapes(self):
        """The growth shapes and three ordinary ones: what the all-pairs walk of the other widths and layouts takes."""
        return self.tagged("growth") + self.tagged("ordinary")

    # -- premises, from the oracle and from pruned_model (no GPU) -----------------------------------
    def check_premise(self, shape):
        s, m = self.c["SLOT_HITS"], self.c["MID_HITS"]
        cnt = self.counts(shape.guides, shape.dist) if shape.n else np.empty(0, dtype=np.int64)
        p = shape.premise
        if p == "small":
            assert 0 < shape.n <= pm.small_batch_limit(self.width, shape.dist) and shape.prune == 1
            assert pm.successor_tolerance(shape.dist) == (0 if shape.dist <= 2 else 1)
        elif p == "small_d5":   # a batch of the small path's size at max_dist 5: that path never takes it (67 ways: the general path)
            assert 0 < shape.n <= pm.small_batch_limit(self.width, 4) and shape.dist == 5 and shape.prune == 1
            assert pm.small_batch_limit(self.width, 5) == 0 and pm.successor_tolerance(5) == 2
        elif p == "over_small":
            assert shape.n == pm.small_batch_limit(self.width, shape.dist) + 1 and shape.prune == 1
        elif p == "below_capacity":
            assert pm.small_batch_limit(self.width, shape.dist) < shape.n < INITIAL_GUIDES and shape.prune == 1 and shape.dist <= 4
        elif p == "above_capacity":
            assert INITIAL_GUIDES < shape.n
        elif p == "above_first":
            assert shape.n > self.by_name["big1500"].n > INITIAL_GUIDES
        elif p == "whole_buckets":
            assert shape.dist == 6 or shape.prune == 0
        elif p == "clean":
            assert cnt.max() <= s and cnt.max() >= s - 1 and cnt.min() == 0
        elif p == "one_above":
            assert (cnt > s).sum() == 1 and (cnt > s).sum() <= shape.n // 8
        elif p == "widen":   # finish_batches: overflowed > n / 8
            assert (cnt > s).sum() > shape.n // 8
        elif p == "above_mid":
            assert (cnt > m).sum() == 1
        elif p == "zero_hits":
            assert shape.n > 1 and cnt.sum() == 0
        elif p == "one_guide":
            assert shape.n == 1 and cnt[0] > 0
        elif p == "repeated":
            assert shape.n > 1 and len(np.unique(shape.guides)) == 1 and cnt[0] > 0
        elif p == "n0":
            assert shape.n == 0
        elif p == "no_exit":
            assert shape.thr == 0.0 and np.array_equal(self.kept(shape.guides, shape.dist, 0.0, shape.method), cnt)
        elif p == "exits":
            kept = self.kept(shape.guides, shape.dist, shape.thr, shape.method)
            assert shape.thr == 75.0 and (kept[cnt > s] < cnt[cnt > s]).all() and (cnt > s).any()
        else:
            raise AssertionError("shape %s has no premise" % shape.name)
        if shape.prune == 1 and shape.dist <= 5:
            assert shape.n <= (1 << 18) // (self.n_slices // 5)   # prune_max_guides: the pruned plan takes the batch

    def guide_kinds(self):
        """How many guides of the shapes are of each kind the issue lists (hits within four mismatches)."""
        s, m = self.c["SLOT_HITS"], self.c["MID_HITS"]
        guides = np.unique(np.concatenate([sh.guides for sh in self.shapes if sh.dist == 4]))
        cnt = self.counts(guides, 4)
        return {"handful": int(((cnt >= 1) & (cnt <= 8)).sum()), "just_below": int((cnt == s - 1).sum()), "at": int((cnt == s).sum()),
                "just_above": int((cnt == s + 1).sum()), "between": int(((cnt > s + 1) & (cnt < m)).sum()),
                "above_mid": int((cnt > m).sum()), "none": int((cnt == 0).sum())}


_WORLDS = {}


def world(width, tmp_path_factory):
    if width not in _WORLDS:
        _WORLDS[width] = World(width, tmp_path_factory.mktemp("handle_sequences_w%d" % width))
    return _WORLDS[width]


def eulerian_walk(k):
    """A closed walk over k shapes that takes every ordered pair (i, j), i == j included, exactly once: k * k + 1 stops
    (Hierholzer on the complete digraph with loops)."""
    nxt = [0] * k            # the next unused successor of every vertex
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    return walk[::-1]


# ------------------------------------------------------------------------------------------------
# what a handle carries from batch to batch
# ------------------------------------------------------------------------------------------------

class HandleModel:
    """Lane 0's workspace as issl_pipeline.cpp keeps it, for the keys that follow from the calls alone: ws_cap_guides,
    ws_slot_width, ws_fine_ways, ws_lean -- and where a batch is run twice because the lane had been lean.  (ws_cap_chunks and
    ws_cap_fitems depend on what the scan meets; the tests tie them to scan_launches instead.)
    options: hit_slots, lean_tail and small_bin as the handle has them (issl_index_get_option)."""

    def __init__(self, world, layout, hit_slots=1, lean_tail=1):
        self.w, self.c = world, world.c
        self.sorted = layout != "list"
        self.hit_slots, self.lean_tail = hit_slots, lean_tail
        self.cap_guides = self.slot_width = self.fine_ways = self.lean = 0

    def keys(self):
        return {"ws_cap_guides": self.cap_guides, "ws_slot_width": self.slot_width, "ws_fine_ways": self.fine_ways, "ws_lean": self.lean}

    def plan(self, shape):
        """The library calls of the shape's entry point, as `dump` flags of their batches: issl_dump_hits is called for the
        count and again for the list (unless nothing is kept), issl_offtargets counts with a plain scoring batch (k_verify's
        per-guide counts) and lists with a dump; n = 0 launches nothing."""
        if shape.n == 0:
            return []
        if shape.entry in ("score", "offtarget_profile"):
            return [False]
        if shape.entry == "dump_hits":
            return [True, True] if len(self.w.expected(shape)) else [True]
        return [False, True] if int(self.w.counts(shape.guides, shape.dist).sum()) else [False]

    def batch(self, shape, dump):
        """One batch through ensure_workspace, enqueue_batch and finish_batches.  -> runs (2: mispredicted lean tail)."""
        n = shape.n
        if self.cap_guides == 0:
            self.slot_width = self.c["kSlotHits"]
        if self.hit_slots == 2:
            self.slot_width = self.c["kSlotHitsWide"]       # (force_wide: our batches are far from kSlotBytesMax)
        self.cap_guides = max(self.cap_guides, n, INITIAL_GUIDES) if n > self.cap_guides else self.cap_guides
        if self.sorted:
            mode3 = shape.prune != 0 and shape.dist == 5
            self.fine_ways = max(self.fine_ways, self.c["kFineWays2"] if mode3 else self.c["kFineWays"])
        slot_hits = 0 if dump or not self.hit_slots else self.slot_width
        over = int((self.w.counts(shape.guides, shape.dist) > self.c["kSlotHits"]).sum())
        runs = 2 if (self.lean and slot_hits and self.lean_tail and over) else 1
        if self.slot_width == self.c["kSlotHits"] and self.hit_slots and over > n // 8:
            self.slot_width = self.c["kSlotHitsWide"]
        self.lean = 1 if (over == 0 and slot_hits) else 0
        return runs

    def pruned(self, shape):
        """issl_stats::pruned of the call when the item list has room: the mode the shape names."""
        if not self.sorted or shape.prune == 0 or shape.dist > 5 or shape.n == 0:
            return 0
        return 1 if shape.dist <= 2 else 2 if shape.dist <= 4 else 3

    def small_path(self, shape, small_bin=1):
        return bool(small_bin) and self.pruned(shape) in (1, 2) and shape.n * self.w.n_slices <= pm.SMALL_PAIRS

    def call(self, shape):
        """-> runs of the call's LAST batch that the lean tail explains (what issl_stats::scan_launches reports, other retries
        aside).  The Python entry points make two library calls where they first ask for a count."""
        runs = 0
        for dump in self.plan(shape):
            runs = self.batch(shape, dump)
        return runs
