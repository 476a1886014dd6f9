"""The parts of the pruned scan beside its comparison passes -- noting, the short unit's set-up and masks, the full unit's
prologue -- on CONSTRUCTED groups of one small index: MIT / CFD as 64-bit patterns and hit lists row for row against the
CPU oracle, the comparison counters through synth.check_comparisons and the unit model of tests/pruned_model.py.

Every case is a bucket of slice 0 of its own (8-bit slices: positions 0..3 the slice, 4..7 the successor byte, 8..19 free):
a lead group of L sites, the target group of n, a trail group of >= 1100, their bytes one position apart and neighbours in
the bucket's order.  What a case is there for is asserted from the signatures alone (World.check, no GPU involved):

  boundaries   remainder 1, 511, 512, 513, 1023, 1024, 1025 (shapes 8 / 16 / 32, the window starting on a lane group or five
               candidates into one) x 1, 3, 4, 5, 31, 32, 33 guides of both classes: a partial last pass, exactly eight
               passes of four, a second mask batch that holds one guide
  rounds       one guide with >= 3 sites within its budget among one lane's candidates while another lane has hits in
               the same pass: second and third round of the noting loop (a full and a short unit)
  chunk        one (unit, guide) pair with > 127 hits: the pass crosses a chunk boundary; again with a record buffer too
               small for the wave's own chunk / for its later reservations (spare chunk, grow and re-run)
  straddle     windows that start late in a tile and reach into the next one (full and short)
  end          (an index of its own) the group that ends the stream: lanes beyond the last tile read the last tile instead
  duplicates   guides that are copies of a site: exact in the previous slice as well wherever slice >= 1 is exact"""
import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
import pruned_model as pm
from synth import check_comparisons, text_order_key
from test_pruned_units import _shape_of   # (the unit model that file pins: pruned_model + its shape rule)

pytestmark = pytest.mark.gpu

REMAINDERS = (1, 511, 512, 513, 1023, 1024, 1025)
GUIDE_COUNTS = (1, 3, 4, 5, 31, 32, 33)
FREE0 = 16              # bit of the first free position (8)
NF = 12                 # free positions


def _sig(value, byte, free):
    return np.uint64(value) | (np.uint64(byte) << np.uint64(8)) | (np.asarray(free, dtype=np.uint64) << np.uint64(FREE0))


def _dist(sites, guide):
    x = np.asarray(sites, dtype=np.uint64) ^ np.uint64(guide)
    x = (x | (x >> np.uint64(1))) & np.uint64(0x5555555555)
    return np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)


def _text_sorted(sigs):
    sigs = np.unique(np.asarray(sigs, dtype=np.uint64))
    return sigs[np.argsort(text_order_key(sigs), kind="stable")]


def _free_parts(rng, m, c0, keep=()):
    """m distinct free parts: c0 with A in front (the group's first site in text order), c0 with T in front (its last),
    between them `keep` and values with C or G in front -- half of them within three substitutions of c0."""
    lead = np.uint64(3)
    first, last = np.uint64(c0) & ~lead, np.uint64(c0) | lead
    if m <= 2:
        return np.array([first, last][:m], dtype=np.uint64)
    got = np.unique(np.array(list(keep), dtype=np.uint64))
    assert len(got) == len(keep) <= m - 2 and all(int(k) & 3 in (1, 2) for k in got)
    while len(got) < m - 2:
        r = rng.integers(0, 1 << (2 * NF), size=2 * m, dtype=np.uint64)
        near = np.full(2 * m, c0, dtype=np.uint64)
        for _ in range(3):
            near ^= rng.integers(0, 4, size=2 * m, dtype=np.uint64) << (np.uint64(2) * rng.integers(1, NF, size=2 * m).astype(np.uint64))
        r = np.where(np.arange(2 * m) % 2 == 0, r, near)
        r = (r & ~lead) | rng.integers(1, 3, size=2 * m, dtype=np.uint64)
        new = np.setdiff1d(np.unique(r), got)
        got = np.concatenate([got, rng.permutation(new)[:m - 2 - len(got)]])
    return np.concatenate([[first], got, [last]]).astype(np.uint64)


def _cluster(c0, positions):
    """c0 with every combination of bases at the given free positions (its last ones: neighbours in text order)."""
    out = [int(c0)]
    for p in positions:
        out = [(x & ~(3 << (2 * p))) | (b << (2 * p)) for x in out for b in range(4)]
    return out


class World:
    """Sites (text order, with occurrences), guides and the cases: per case its bucket value, target byte and guide range."""

    def __init__(self, seed=20267):
        rng = np.random.default_rng(seed)
        self.cases, site_parts, guide_parts, n_guides = [], [], [], 0

        def add(kind, span, lead, guides_of, keep=(), trail=1100, **more):
            nonlocal n_guides
            i = len(self.cases)
            value, byte = i, ((i * 20) & 0xFC) | (1 + i % 2)
            n = span - lead % 32
            c0 = int(rng.integers(0, 1 << (2 * NF)))
            if keep:
                c0 = (int(keep[0]) & ~3) | (c0 & 3)
            groups = {}
            for name, b, m, kp in (("lead", byte - 1, lead, ()), ("target", byte, n, keep), ("trail", byte + 1, trail, ())):
                groups[name] = _text_sorted(_sig(value, b, _free_parts(rng, m, c0, kp))) if m else np.empty(0, dtype=np.uint64)
                assert len(groups[name]) == m
                site_parts.append(groups[name])
            guides = np.array(guides_of(groups, byte), dtype=np.uint64)
            guide_parts.append(guides)
            self.cases.append(dict(kind=kind, span=span, lead=lead, n=n, trail=trail, value=value, byte=byte, g0=n_guides,
                                   g1=n_guides + len(guides), **more))
            n_guides += len(guides)

        def edge_guides(g):
            """g guides on the window's first, last and a middle site and on its neighbours just outside, 0..4 substitutions
            in the free positions, both classes (the byte's low position changed or not)."""
            def make(groups, byte):
                t = groups["target"]
                anchors = [t[0], t[-1], t[len(t) // 2], groups["trail"][0]] + ([groups["lead"][-1]] if len(groups["lead"]) else [])
                out = []
                for j in range(g):
                    x = int(anchors[j % len(anchors)])
                    subs = j % 3 if j < 5 else int(rng.integers(0, 5))
                    for pos in rng.choice(np.arange(1, NF), size=subs, replace=False):
                        x ^= int(rng.integers(1, 4)) << (FREE0 + 2 * int(pos))
                    if (j & 1) if j < 5 else int(rng.integers(0, 2)):
                        x ^= int(rng.integers(1, 4)) << 8
                    out.append(x)
                return out
            return make

        for k, rem in enumerate(REMAINDERS):
            for m, g in enumerate(GUIDE_COUNTS):
                lead = 0 if rem == 1 and m % 2 == 0 else 32 if rem == 1 else (0, 37)[(k + m) % 2]
                add("boundary", rem, lead, edge_guides(g), shape=_shape_of(rem), guides=g)
        for span, lead, g in ((2048 + 513, 37, 5), (2048 + 1, 0, 33), (4096, 5, 4)):
            add("boundary", span, lead, edge_guides(g), shape=_shape_of(span), guides=g)

        def centre_guides(extra_positions):
            """The cluster's centre (class 0), the centre with the byte's low position changed (class 1) and the centre with one
            substitution at each of the given free positions."""
            def make(groups, byte):
                centre = int(self._centre) << FREE0 | int(groups["target"][0]) & 0xFFFF
                out = [centre, centre ^ (2 << 8)]
                for pos in extra_positions:
                    out.append(centre ^ (1 << (FREE0 + 2 * pos)))
                return out
            return make

        for span, shape in ((1500, 32), (400, 8)):   # rounds: two clusters of 16 neighbours, one position apart
            self._centre = int(rng.integers(0, 1 << (2 * NF))) & ~3 | 1
            keep = _cluster(self._centre, (10, 11)) + _cluster(self._centre ^ (1 << (2 * 3)), (10, 11))
            add("rounds", span, 0, centre_guides(()), keep=keep, shape=shape)
        self._centre = int(rng.integers(0, 1 << (2 * NF))) & ~3 | 2
        add("chunk", 1800, 0, centre_guides((1, 2, 3, 4)), keep=_cluster(self._centre, (8, 9, 10, 11)), shape=32)
        add("straddle", 1200, 1500, edge_guides(5), shape=32, guides=5)
        add("straddle", 300, 2000, edge_guides(5), shape=8, guides=5)
        # (random sites keep out of the cases' buckets of slice 0; their other slices mix with the cases')
        used = len(self.cases)
        extra = rng.integers(0, 1 << 40, size=20000, dtype=np.uint64)
        extra = (extra & ~np.uint64(255)) | rng.integers(used, 256, size=len(extra), dtype=np.uint64)
        self.sigs = _text_sorted(np.concatenate(site_parts + [extra]))
        assert len(self.sigs) == sum(len(x) for x in site_parts) + len(np.unique(extra)) <= 300_000
        self.occ = rng.integers(1, 4, size=len(self.sigs)).astype(np.uint32)
        other = extra[rng.integers(0, len(extra), size=120)] ^ (rng.integers(0, 4, size=120, dtype=np.uint64) << np.uint64(30))
        self.guides = np.concatenate(guide_parts + [other])
        self.tables = pm.site_tables(self.sigs, 8)
        self._model = {}

    def bucket(self, c):
        """-> (the bucket's sites in scan order: by successor byte, ties in list order; s0, s1 of the target group)."""
        mine = self.sigs[(self.sigs & np.uint64(255)) == np.uint64(c["value"])]
        byte = ((mine >> np.uint64(8)) & np.uint64(255)).astype(np.int64)
        order = mine[np.argsort(byte, kind="stable")]
        s0 = int((byte < c["byte"]).sum())
        return order, s0, s0 + int((byte == c["byte"]).sum())

    def check(self):
        """Every case is what it is named after -- from the signatures, slice 0's bucket ordered by the byte behind it."""
        gvalue = (self.guides & np.uint64(255)).astype(np.int64)
        gbyte = ((self.guides >> np.uint64(8)) & np.uint64(255)).astype(np.int64)
        seen = set()
        for c in self.cases:
            order, s0, s1 = self.bucket(c)
            start = s0 & ~31
            assert s1 - s0 == c["n"] and s0 == c["lead"] and s1 - start == c["span"] and len(order) - s1 == c["trail"], c
            units, _, shape = pm.group_units(s0, s1, len(order), 1)
            assert int(shape) == c["shape"] == _shape_of(c["span"]) and int(units) == -(-c["span"] // 2048), c
            x = gbyte[gvalue == c["value"]] ^ c["byte"]
            landing = int((np.array([bin((v | (v >> 1)) & 0x55).count("1") for v in x]) <= 1).sum())
            assert landing == c["g1"] - c["g0"], c
            guides = self.guides[c["g0"]:c["g1"]]
            cls = np.array([bin(((int(g) >> 8 & 255) ^ c["byte"]) & 0xFF).count("1") > 0 for g in guides])
            if c["kind"] == "boundary":
                assert landing == c["guides"] and (landing < 3 or (cls.any() and not cls.all())), c   # both classes: gmid inside
                seen.add((c["span"] % 2048, c["lead"] % 32 != 0, landing))
                # hits just inside and just outside the window, at max_dist 4
                for site in (order[s0], order[s1 - 1], order[s1]) + ((order[s0 - 1],) if s0 else ()):
                    assert (_dist(guides, site) <= 4).any(), c
            last_start = start + (int(units) - 1) * 2048
            per_lane = c["shape"]
            if c["kind"] == "rounds":       # guide 0 against the last unit: a lane with >= 3 hits, and a second lane with hits
                for g in guides[:2]:
                    near = np.flatnonzero(_dist(order[s0:s1], g) <= 3) + s0
                    lanes = np.bincount((near[near >= last_start] - last_start) // per_lane, minlength=64)
                    assert lanes.max() >= 3 and (lanes > 0).sum() >= 2, (c, lanes)
                    if per_lane < 32:       # ... two of them in one group of 32 candidates
                        hit = np.flatnonzero(lanes) // (32 // per_lane)
                        assert len(np.unique(hit)) < len(hit), (c, lanes)
            if c["kind"] == "chunk":        # one guide, one unit: more hits than a chunk holds
                assert int(units) == 1
                assert int((_dist(order[s0:s1], guides[0]) <= 4).sum()) > 127, c
                assert int(sum((_dist(order[s0:s1], g) <= 4).sum() for g in guides)) > 3 * 127, c   # ... and two reservations more
            if c["kind"] == "straddle":     # the last unit starts late in a tile and ends in the next one
                g0 = (last_start >> 5) & 63
                assert g0 > 0 and g0 + (64 * per_lane // 32) > 64 and (s1 - 1 - (last_start & ~2047)) >= 2048, c
        for rem in REMAINDERS:
            assert all(any((rem, inside, n) in seen for inside in (False, True)) for n in GUIDE_COUNTS), rem
        assert {inside for _, inside, _ in seen} == {False, True}
        # duplicates: guides that are a site -- exact in every slice, so in slices 1..4 the previous slice is exact as well
        site_set = set(int(s) for s in self.sigs)
        assert sum(int(g) in site_set for g in self.guides) >= 50

    def model(self, dist):
        if dist not in self._model:
            self._model[dist] = pm.unit_model(self.tables, self.guides, dist, 8, 512, 1, False)
        return self._model[dist]


def end_world(shape, seed=20269):
    """A small index whose LAST bucket (slice 4, value TTTT) ends in a group that starts late in the stream's last tile, so
    that the window of its unit reaches past the stream: 1600 + 120 sites (shape 8) or 1000 + 1030 (shape 32).  Slice 4's
    successor byte is positions 0..3.  -> (sigs, occ, guides, (s0, s1, bucket length))"""
    rng = np.random.default_rng([seed, shape])
    lead, n = (1600, 120) if shape == 8 else (1000, 1030)
    tail = np.uint64(0xFF) << np.uint64(32)                      # positions 16..19 = T
    parts = []
    for byte, m in ((0xFE, lead), (0xFF, n)):                    # the two highest bytes: the target group is the last one
        mid = np.unique(rng.integers(0, 1 << 24, size=2 * m, dtype=np.uint64))[:m]
        assert len(mid) == m
        parts.append(np.uint64(byte) | (rng.permutation(mid) << np.uint64(8)) | tail)
    rest = rng.integers(0, 1 << 40, size=3000, dtype=np.uint64)
    rest = rest[(rest >> np.uint64(32)) != np.uint64(0xFF)]
    sigs = _text_sorted(np.concatenate(parts + [rest]))
    occ = rng.integers(1, 4, size=len(sigs)).astype(np.uint32)
    mine = sigs[(sigs >> np.uint64(32)) == np.uint64(0xFF)]
    byte = (mine & np.uint64(255)).astype(np.int64)
    order = mine[np.argsort(byte, kind="stable")]
    s0, s1 = int((byte < 0xFF).sum()), len(order)
    t = order[s0:]
    guides = []
    for j, x in enumerate([t[0], t[-1], t[len(t) // 2], order[s0 - 1]] * 3):
        x = int(x)
        for pos in rng.choice(np.arange(4, 16), size=j % 4, replace=False):
            x ^= int(rng.integers(1, 4)) << (2 * int(pos))
        if j & 1:
            x ^= int(rng.integers(1, 4))                          # position 0: the low position of slice 4's successor byte
        guides.append(x)
    return sigs, occ, np.array(guides, dtype=np.uint64), (s0, s1, len(order))


def check_end_world(shape):
    sigs, occ, guides, (s0, s1, blen) = end_world(shape)
    assert (sigs >> np.uint64(32)).max() == 0xFF                  # the last bucket of the last slice: the end of the stream
    units, _, got = pm.group_units(s0, s1, blen, 1)
    assert int(got) == shape and int(units) == 1
    tiles = -(-blen // 2048)
    assert (s0 & ~31) + 64 * shape > 2048 * tiles                 # the window reaches past the bucket's -- the stream's -- last tile
    return sigs, occ, guides


def _index(tmp, name, sigs, occ):
    ix = ca.IsslIndex.build_on_device(sigs, occ, device=0)
    path = tmp / name
    ix.write(path)
    return ix, path


class _Device:
    def __init__(self, tmp):
        self.w = World()
        self.w.check()
        self.ix, self.path = _index(tmp, "trim.issl", self.w.sigs, self.w.occ)
        assert self.ix.get_option("is_sorted") == 1
        self.oracle = ou.OracleIndex(self.path)
        self._want = {}

    def want(self, dist):
        if dist not in self._want:
            self._want[dist] = self.oracle.score(self.w.guides, dist, 0.0, "and", want_hits=True, hit_cap=1 << 23)
        return self._want[dist]


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    d = _Device(tmp_path_factory.mktemp("trim"))
    yield d
    d.ix.close()
    d.oracle.close()


def _score_and_check(ix, world, guides, want, dist, prune, hits=True):
    wmit, wcfd, whits = want
    mit, cfd = ix.score(guides, dist, 0.0, "and")
    st = check_comparisons(ix, guides, prune=prune if prune == 0 else None, site_sigs=world.tables if world else None, max_dist=dist)
    assert np.array_equal(mit.view(np.uint64), wmit.view(np.uint64)), "MIT not bit-identical"
    assert np.array_equal(cfd.view(np.uint64), wcfd.view(np.uint64)), "CFD not bit-identical"
    if hits:
        got = ix.dump_hits(guides, dist, 0.0, "and")
        assert got.shape == whits.shape and np.array_equal(got, whits)
    return st


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("dist", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("prune", [0, 1, -1])
def test_constructed_cases_against_oracle(dev, prune, dist, generic):
    ix, w = dev.ix, dev.w
    ix.set_option("prune", prune).set_option("scan_generic", generic)
    try:
        st = _score_and_check(ix, w, w.guides, dev.want(dist), dist, prune, hits=(prune != 0 or generic == 0))
        if prune == 1:
            assert st["pruned"] == (1 if dist <= 2 else 2 if dist <= 4 else 3)
        if st["pruned"]:
            tiles, cands = w.model(dist)
            assert (st["scan_tiles"], st["candidates"]) == (tiles, cands)
    finally:
        ix.set_option("prune", -1).set_option("scan_generic", 0)


@pytest.mark.parametrize("raw_chunks", [4, 20])
def test_small_record_buffer_spare_chunk_and_rerun(dev, raw_chunks):
    """The chunk case's guides (thousands of records) with a record buffer of 4 chunks (waves without a chunk of their own: the
    spare chunk, the overflow flag) and of 20 (own chunks, then reservations of 1, 2, 4 ... until they run out): the batch is
    run again with a larger buffer and gives the same lists."""
    c = next(c for c in dev.w.cases if c["kind"] == "chunk")
    pick = np.arange(c["g0"], c["g1"])
    wmit, wcfd, whits = dev.want(4)
    rows = whits[(whits[:, 0] >= c["g0"]) & (whits[:, 0] < c["g1"])].copy()
    rows[:, 0] -= c["g0"]
    ix = ca.IsslIndex.open(dev.path)
    ix.set_option("raw_chunks", raw_chunks).set_option("prune", 1)
    ix.upload(0)
    try:
        guides = dev.w.guides[pick]
        mit, cfd = ix.score(guides, 4, 0.0, "and")
        assert ix.stats()["scan_launches"] >= 2 and ix.stats()["pruned"] == 2
        assert np.array_equal(mit.view(np.uint64), wmit[pick].view(np.uint64))
        assert np.array_equal(cfd.view(np.uint64), wcfd[pick].view(np.uint64))
        got = ix.dump_hits(guides, 4, 0.0, "and")
        assert got.shape == rows.shape and np.array_equal(got, rows)
    finally:
        ix.close()


@pytest.mark.parametrize("shape", [8, 32])
def test_group_that_ends_the_stream(tmp_path, shape):
    sigs, occ, guides = check_end_world(shape)
    ix, path = _index(tmp_path, "end.issl", sigs, occ)
    oracle = ou.OracleIndex(path)
    try:
        for dist in (2, 4, 5):
            want = oracle.score(guides, dist, 0.0, "and", want_hits=True)
            for generic in (0, 1):
                ix.set_option("prune", 1).set_option("scan_generic", generic)
                st = _score_and_check(ix, None, guides, want, dist, 1)
                assert st["pruned"] == (1 if dist <= 2 else 2 if dist <= 4 else 3)
                assert st["planned_comparisons"] == pm.planned_comparisons(sigs, guides, dist, 8)
    finally:
        ix.close()
        oracle.close()
