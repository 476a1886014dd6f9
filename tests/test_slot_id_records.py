"""Raw records of the pruned scan carry the slot's id -- slice << 22 | guide -- instead of a slot number: every case scores a
batch on the GPU and compares MIT and CFD as 64-bit patterns with the CPU oracle.

One index of ~4 000 sites per slice width (5, 10 and 20 slices): ~2 000 random sites and, on slice-0 values of their own,
three constructed successor-byte groups whose sizes are exact because the random sites are kept out of them:
  * value 1, byte AAAA (a bucket's first group: it starts on a lane group): 512 sites  -> one short unit of 8 candidates per lane
  * value 2, byte AAAA: 1024 sites                                                    -> one short unit of 16 per lane
  * value T.., byte TTTT: the site TTTTTTTTTTTTTTTTTTTT alone -- what a padding slot's word (all T) matches exactly
Filler guides have slice-0 value 0 and so stay out of all three.

Slices.  A hit has at most max_dist mismatching slices in front of its first exact one, so "first exact in slice s" can be
built for s <= 4 only: guide s has one substitution in each of the slices 0 .. s-1.  Beyond that (ten and twenty slices) guide
s has its four substitutions in the four slices in front of s: bucket s notes the site under id slice s -- the values 16..19
among them -- and k_verify has to see in it the duplicate of a lower slice's record."""
import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
import pruned_model as pm
from synth import random_guides, random_guides_fast, random_sites, text_order_key

pytestmark = pytest.mark.gpu

ALL_T = np.uint64((1 << 40) - 1)
V_SHORT8, V_SHORT16, FILL = 1, 2, 0     # slice-0 values of the two short-unit groups and of the filler guides
BIG_BATCH = {8: 1 << 20, 4: 1 << 19, 2: 1 << 18}   # by slice width: all the guides a pruned launch takes (prune_max_guides), so the id's guide
                                                    # field goes up to 2^20 - 1; guides and oracle take ~2 s on this index, the GPU less


def _sub(sig, pos, step=1):
    """The signature with the base at `pos` replaced by another one."""
    code = (int(sig) >> (2 * pos)) & 3
    return (int(sig) & ~(3 << (2 * pos))) | (((code + step) & 3) << (2 * pos))


class World:
    def __init__(self, tmp, width):
        self.width, self.p = width, width // 2
        p, rng = self.p, np.random.default_rng([2027, width])
        self.n_slices = 40 // width
        low = np.uint64((1 << width) - 1)
        self.t_value = int(ALL_T & low)
        base, _ = random_sites(2000, seed=300 + width)
        value, byte = (base & low).astype(np.int64), ((base >> np.uint64(2 * p)) & np.uint64(255)).astype(np.int64)
        keep = ~(((value == V_SHORT8) | (value == V_SHORT16)) & (byte == 0)) & ~((value == self.t_value) & (byte == 255)) & (base != ALL_T)
        base = base[keep]
        self.short = {}
        parts = [base, np.array([ALL_T], dtype=np.uint64)]
        for v, n in ((V_SHORT8, 512), (V_SHORT16, 1024)):
            free = rng.choice(1 << (2 * (16 - p)), size=n, replace=False).astype(np.uint64)
            g = np.uint64(v) | (free << np.uint64(2 * (p + 4)))
            g = g[np.argsort(text_order_key(g), kind="stable")]     # the group's order: list order = text order
            self.short[n] = g
            parts.append(g)
        sigs = np.unique(np.concatenate(parts))
        self.sigs = sigs[np.argsort(text_order_key(sigs), kind="stable")]
        self.occ = rng.integers(1, 4, size=len(self.sigs)).astype(np.uint32)
        self.limit = pm.small_batch_limit(width, 4)

        fill = random_guides(self.sigs, self.limit + 60, seed=17 + width)
        self.fill = (fill & ~low) | np.uint64(FILL)
        # slices: see the module's docstring; the sites are random ones with slice-0 value 0, the substitution goes to the slice's first position
        pool = base[(base & low) == np.uint64(FILL)]
        self.slice_guides, self.slice_sites = np.empty(self.n_slices, dtype=np.uint64), pool[np.arange(self.n_slices) % len(pool)]
        for s in range(self.n_slices):
            x = int(self.slice_sites[s])
            for j in range(max(0, s - 4), s):
                x = _sub(x, j * p, 1 + (s + j) % 3)
            self.slice_guides[s] = x
        # short units: a class-0 guide on site 8 of the group, a class-1 guide (one substitution in the successor byte, one
        # more behind it) on site 9 -- candidates 8 and 9 of the window share a lane at 8 and at 16 candidates per lane --,
        # and the first guide once more
        self.short_guides = {}
        for n, g in self.short.items():
            a, b = int(g[8]), _sub(_sub(int(g[9]), p, 2), p + 6)
            self.short_guides[n] = np.array([a, b, a], dtype=np.uint64)
        # group fill: guides that are T in slice 0 and in the byte behind it, with 0..4 other bases further on
        self.t_guides = np.empty(9, dtype=np.uint64)
        for k in range(9):
            x = int(ALL_T)
            for pos in rng.choice(np.arange(p + 4, 20), size=k % 5, replace=False):
                x = _sub(x, int(pos), 1 + k % 3)
            self.t_guides[k] = x
        assert len(np.unique(self.t_guides[1:])) == 8
        self.check_premises()

        self.path = tmp / f"slot_id_{width}.issl"
        host = ca.IsslIndex.build_from_sites(self.sigs, self.occ, slice_width=width)
        host.write(self.path)
        host.close()
        self.oracle = ou.OracleIndex(self.path)
        self._want = {}

    def _group(self, sigs, value, byte, tol):
        """Which of `sigs` have slice-0 value `value` and a successor byte within `tol` positions of `byte`."""
        low = np.uint64((1 << self.width) - 1)
        x = ((sigs >> np.uint64(2 * self.p)) & np.uint64(255)).astype(np.int64) ^ byte
        off = np.array([bin((int(v) | (int(v) >> 1)) & 0x55).count("1") for v in x])
        return ((sigs & low) == np.uint64(value)) & (off <= tol)

    def check_premises(self):
        for n, v in ((512, V_SHORT8), (1024, V_SHORT16)):
            assert int(self._group(self.sigs, v, 0, 0).sum()) == n
            units, _, shape = pm.group_units(0, n, int(((self.sigs & np.uint64((1 << self.width) - 1)) == np.uint64(v)).sum()))
            assert int(units) == 1 and int(shape) == (8 if n == 512 else 16)
            assert self._group(self.short_guides[n], v, 0, 1).all() and not self._group(self.short_guides[n][1:2], v, 0, 0).any()
            assert int(self._group(self.fill, v, 0, 1).sum()) == 0
        assert int(self._group(self.sigs, self.t_value, 255, 0).sum()) == 1
        assert self._group(self.t_guides, self.t_value, 255, 0).all()
        assert int(self._group(self.fill, self.t_value, 255, 1).sum()) == 0
        per = self.p
        for s, g in enumerate(self.slice_guides):   # exact in slice s, a substitution in each of the (up to four) slices in front
            x = int(g) ^ int(self.slice_sites[s])
            broken = [j for j in range(self.n_slices) if (x >> (2 * per * j)) & ((1 << (2 * per)) - 1)]
            assert broken == list(range(max(0, s - 4), s)), (s, broken)

    def want(self, guides, dist, thr=0.0):
        key = (guides.tobytes(), dist, thr)
        if key not in self._want:
            self._want[key] = self.oracle.score(guides, dist, thr, "and")
        return self._want[key]

    def has_hit(self, guides, dist):
        """Per guide: the oracle scored some site for it (an exact copy counts for CFD alone)."""
        mit, cfd = self.want(guides, dist)
        return (mit < 100.0) | (cfd < 100.0)

    def mixed(self):
        """Every constructed guide and 160 fillers: the batch of the cases that are about modes, layouts and options."""
        return np.concatenate([self.slice_guides, self.t_guides, self.short_guides[512], self.short_guides[1024], self.fill])


@pytest.fixture(scope="module", params=[8, 4, 2])
def world(request, tmp_path_factory):
    w = World(tmp_path_factory.mktemp("slot_id"), request.param)
    yield w
    w.oracle.close()


@pytest.fixture(scope="module")
def index(world):
    ix = ca.IsslIndex.open(world.path)
    ix.set_option("sorted_layout", 1).set_option("compact", 0).set_option("prune", 1)
    ix.upload(0)
    yield ix
    ix.close()


def _check(ix, world, guides, dist, thr=0.0, pruned=None):
    wmit, wcfd = world.want(guides, dist, thr)
    mit, cfd = ix.score(guides, dist, thr, "and")
    st = ix.stats()
    where = (world.width, len(guides), dist, thr)
    assert np.array_equal(mit.view(np.uint64), wmit.view(np.uint64)), ("MIT not bit-identical",) + where
    assert np.array_equal(cfd.view(np.uint64), wcfd.view(np.uint64)), ("CFD not bit-identical",) + where
    want_mode = (1 if dist <= 2 else 2 if dist <= 4 else 3) if pruned is None else pruned
    assert st["pruned"] == want_mode, where
    return st


def test_every_slice_reports_its_hits(world, index):
    """The slice guides alone (the one-launch binning) and among fillers (the general kernels), max_dist 4 and 5; every one
    of them has the hit it was built from."""
    for guides in (world.slice_guides[:world.limit], np.concatenate([world.fill[:world.limit], world.slice_guides])):
        for dist in (4, 5):
            _check(index, world, guides, dist)
            assert world.has_hit(guides, dist)[-world.n_slices:].all()


@pytest.mark.parametrize("extra", [0, 1])
def test_batches_around_the_small_bin_limit(world, index, extra):
    """limit and limit + 1 guides (102 and 103 of five slices): the one-launch binning and the general kernels; the guides
    of the two highest slices at both ends of the batch."""
    n = world.limit + extra
    guides = np.concatenate([world.slice_guides[-1:], world.fill[:n - 2], world.slice_guides[-2:-1]])
    assert len(guides) == n
    _check(index, world, guides, 4)


def test_large_batch_guide_at_both_ends(world, index):
    guides = random_guides_fast(world.sigs, BIG_BATCH[world.width], seed=5)
    guides[0], guides[-1] = world.slice_guides[-1], world.slice_guides[-2]
    _check(index, world, guides, 4, 75.0)


@pytest.mark.parametrize("fillers", [True, False])
def test_group_fill_and_padding_slots(world, index, fillers):
    """9, 8, 7 and 1 guides in the group that holds the all-T site, in this order: the slots that hold guides in one batch
    are padding in the next.  A padding slot matches that site in the scan; its records must be dropped."""
    tail = world.fill[:world.limit + 1] if fillers else world.fill[:0]
    for k in (9, 8, 7, 1):
        guides = np.concatenate([world.t_guides[:k], tail])
        assert int(world._group(guides, world.t_value, 255, 1).sum()) == k
        _check(index, world, guides, 4)
        assert world.has_hit(guides, 4)[:k].all()       # (on the all-T site)


@pytest.mark.parametrize("fillers", [True, False])
@pytest.mark.parametrize("tail_shapes", [1, 0])
def test_short_units_two_guides_of_a_pass_in_one_lane(world, index, fillers, tail_shapes):
    tail = world.fill[:world.limit + 1] if fillers else world.fill[:0]
    index.set_option("tail_shapes", tail_shapes)
    try:
        for picks in ((512,), (1024,), (512, 1024)):
            for m in (2, 3):    # without and with the repeated guide
                guides = np.concatenate([world.short_guides[n][:m] for n in picks] + [tail])
                _check(index, world, guides, 4)
                assert world.has_hit(guides, 4)[:m].all()
    finally:
        index.set_option("tail_shapes", 1)


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("dist", [2, 4, 5])
def test_prune_modes(world, index, dist, generic):
    index.set_option("scan_generic", generic)
    try:
        for thr in (0.0, 75.0):
            _check(index, world, world.mixed(), dist, thr)
    finally:
        index.set_option("scan_generic", 0)


OPTIONS = {
    "list_order": ({"sorted_layout": 0, "host_cold": 0}, {}, 0),        # no pruned plan: slot numbers in the records, as before
    "compact": ({"compact": 1, "host_cold": 0, "keep_lists": 1}, {}, 2),
    "compact_cold": ({"compact": 1, "host_cold": 1}, {}, 2),
    "item_guides": ({"sorted_layout": 1, "compact": 0}, {"item_guides": 8}, 2),
    "raw_chunks": ({"sorted_layout": 1, "compact": 0, "raw_chunks": 4}, {}, 2),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_layouts_and_options(world, name):
    before, after, mode = OPTIONS[name]
    ix = ca.IsslIndex.open(world.path)
    try:
        for key, value in before.items():
            ix.set_option(key, value)
        ix.set_option("prune", 1 if mode else 0)
        ix.upload(0)
        for key, value in after.items():
            ix.set_option(key, value)
        st = _check(ix, world, world.mixed(), 4, 0.0, pruned=mode)
        if name == "raw_chunks":    # waves without a chunk of their own: the spare chunk, then the batch once more
            assert st["scan_launches"] >= 2
        _check(ix, world, world.mixed()[::-1].copy(), 4, 75.0, pruned=mode)
    finally:
        ix.close()


def test_two_lanes(world, index):
    import torch
    batches = [world.mixed(), world.slice_guides, world.mixed()[::-1].copy(), world.short_guides[1024], world.t_guides[:7]] * 2
    index.set_option("lanes", 2)
    try:
        outs = []
        for g in batches:
            d_g = torch.from_numpy(g.view(np.int64)).cuda()
            d_m = torch.empty(len(g), dtype=torch.float64, device="cuda:0")
            outs.append((g, d_g, d_m, torch.empty_like(d_m)))
        while True:
            for g, d_g, d_m, d_c in outs:
                index.score_device_async(d_g, d_m, d_c, 4, 75.0, "and")
            if index.finish():
                break
        for g, d_g, d_m, d_c in outs:
            wmit, wcfd = world.want(g, 4, 75.0)
            assert np.array_equal(d_m.cpu().numpy().view(np.uint64), wmit.view(np.uint64))
            assert np.array_equal(d_c.cpu().numpy().view(np.uint64), wcfd.view(np.uint64))
    finally:
        index.set_option("lanes", 1)
