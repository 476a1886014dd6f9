"""One centre and EVERY placement of up to four mismatches around it (and a mixed family out to six), for the scan's
distance tests: count_near / count_near12, the runtime comparators, short_unit_masks and fine_dup of issl_kernels.hip.
tests/test_neighbourhood_construction.py checks the construction on the CPU, tests/test_scan_placements.py scores it on
the GPU.  Plain numpy; nothing of crackling_amd is imported here.

Geometry: 20 positions, position p at bits 2p .. 2p + 1 of the packed signature; a slice of width w is w / 2 positions.
A mismatch is (low bit differs) | (high bit differs), so each placement comes in three kinds: code ^= 1 (low bit only),
^= 2 (high bit only), ^= 3 (both).

Sites, in text order, distinct:
  family v in {1, 2, 3}:  the centre with code ^= v at every position of P, for EVERY set P of 0..4 positions;
  mixed family:           for every P of 1..6 positions, code ^= 1 + (p + |P|) % 3 at each p of P: the three kinds inside
                          one site, and the shells at distance 5 and 6 that a threshold of 4 must reject and thresholds
                          5, 6 and 7 must accept.
The occurrence count of site id is 1 + id % 3, so the MIT and CFD sums depend on WHICH sites are hit."""
import itertools

import numpy as np

from synth import text_order_key

SEQ_LEN = 20
N_SITES = 78793
CENTRE_SEED = 40417

# the ten mutants of the centre that ride with it in batch B: (position, xor) per substitution
GUIDE_SUBS = [
    [(9, 1)],
    [(12, 2), (17, 3)],
    [(8, 3), (13, 1), (18, 2)],
    [(10, 1), (11, 2), (14, 3), (19, 1)],
    [(4, 1)],
    [(7, 2), (15, 1)],
    [(0, 3)],
    [(3, 1), (16, 2)],
    [(19, 2)],
    [(16, 1), (2, 2)],
]

# what the oracle gives for the centre alone: cumulative hits at max_dist 0, 1, ...  (a site with one mismatch in each of
# the five 8-bit slices is never met: the reference's behaviour)
CUMULATIVE = {8: [1, 61, 764, 5234, 24529, 39009, 70089], 4: [1, 61, 764, 5234, 24529, 40033, 78793],
              2: [1, 61, 764, 5234, 24529, 40033, 78793]}
BATCH_B_ROWS_WIDTH8 = {4: 96922, 6: 443900}


def _placements(k):
    """[C(20, k), k]: every set of k positions."""
    sets = list(itertools.combinations(range(SEQ_LEN), k))
    return np.array(sets, dtype=np.uint64).reshape(len(sets), k)


def _substituted(centre, positions, xors):
    """The centre with code ^= xors[i, j] at positions[i, j] (distinct inside a row: the shifted codes add up)."""
    return np.uint64(centre) ^ (xors.astype(np.uint64) << (np.uint64(2) * positions)).sum(axis=1, dtype=np.uint64)


def family(centre, v):
    """Code ^= v at every position of P, for every P of 0..4 positions."""
    parts = []
    for k in range(5):
        pos = _placements(k)
        parts.append(_substituted(centre, pos, np.full(pos.shape, v, dtype=np.uint64)))
    return np.concatenate(parts)


def mixed_family(centre):
    """Code ^= 1 + (p + |P|) % 3 at each p of P, for every P of 1..6 positions."""
    parts = []
    for k in range(1, 7):
        pos = _placements(k)
        parts.append(_substituted(centre, pos, np.uint64(1) + (pos + np.uint64(k)) % np.uint64(3)))
    return np.concatenate(parts)


class Neighbourhood:
    """centre, sigs (text order, distinct), occ, guides (the centre and its ten mutants), and the three batches."""

    def __init__(self, seed=CENTRE_SEED):
        self.centre = int(np.random.default_rng(seed).integers(0, 1 << (2 * SEQ_LEN), dtype=np.uint64))
        sigs = np.unique(np.concatenate([family(self.centre, v) for v in (1, 2, 3)] + [mixed_family(self.centre)]))
        self.sigs = sigs[np.argsort(text_order_key(sigs), kind="stable")]
        self.occ = (1 + np.arange(len(self.sigs)) % 3).astype(np.uint32)
        guides = [self.centre]
        for subs in GUIDE_SUBS:
            g = self.centre
            for p, x in subs:
                g ^= x << (2 * p)
            guides.append(g)
        self.guides = np.array(guides, dtype=np.uint64)
        self.batches = {"A": np.full(8, self.centre, dtype=np.uint64), "B": self.guides,
                        "C": np.array([self.centre], dtype=np.uint64)}
        for a in (self.sigs, self.occ, self.guides) + tuple(self.batches.values()):
            a.setflags(write=False)


_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(Neighbourhood())
    return _FIXTURE[0]


def codes(sigs):
    """[n, 20]: the 2-bit code of every position."""
    sigs = np.asarray(sigs, dtype=np.uint64)
    return np.stack([((sigs >> np.uint64(2 * p)) & np.uint64(3)).astype(np.int8) for p in range(SEQ_LEN)], axis=1)


def brute_force(sites, occ, guides, max_dist, width):
    """The hit list of the reference scorer without early exit, from the 2-bit codes alone: the distance of every (guide,
    site) pair; a pair is a hit iff the distance is at most max_dist and some slice is equal, and it is reported under the
    FIRST equal slice.  Rows (guide, slice, position in that slice's bucket, id, distance, occurrences), ordered by
    (guide, slice, id) -- the buckets of an index list their sites by ascending id."""
    sc, gc = codes(sites), codes(guides)
    per = width // 2
    n_slices = SEQ_LEN // per
    occ = np.asarray(occ)
    rows = []
    for g in range(len(gc)):
        mism = sc != gc[g]
        dist = mism.sum(axis=1)
        equal = ~mism.reshape(len(sc), n_slices, per).any(axis=2)       # [site, slice]: the slice agrees exactly
        first = np.argmax(equal, axis=1)
        near = (dist <= max_dist) & equal.any(axis=1)
        for s in range(n_slices):
            ids = np.flatnonzero(near & (first == s))
            if len(ids) == 0:
                continue
            pos = np.cumsum(equal[:, s]) - 1                           # the bucket of slice s the guide selects
            rows.append(np.stack([np.full(len(ids), g), np.full(len(ids), s), pos[ids], ids, dist[ids], occ[ids]], axis=1))
    if not rows:
        return np.empty((0, 6), dtype=np.uint32)
    return np.concatenate(rows).astype(np.uint32)


def slice_positions(s, width):
    per = width // 2
    return [s * per + j for j in range(per)]


def successor_positions(s, width):
    """The four positions that follow slice s cyclically: the successor unit."""
    per = width // 2
    return [(s * per + per + j) % SEQ_LEN for j in range(4)]


def placements_seen(sites, centre, v, s, width, positions, successor_mismatches=None):
    """The subsets of `positions` that the sites of family v realise in slice s's bucket of the centre, as sorted bit masks
    (bit i: positions[i] mismatches).  Counted are the sites that differ from the centre by code ^= v and nothing else,
    agree with it on slice s, and have ALL their other mismatches inside `positions` -- except, where
    successor_mismatches is given (the class of the pruned scan: 0 = the centre's own successor-byte group, 1 = the groups
    one mismatch away), exactly that many more in the successor unit.  Such a site is at distance |subset| + class: a hit
    iff the kernel's count over `positions` is right."""
    sc, cc = codes(sites), codes(np.array([centre], dtype=np.uint64))[0]
    x = sc ^ cc
    mism = x != 0
    pure = ((x == 0) | (x == v)).all(axis=1)
    inside = np.zeros(SEQ_LEN, dtype=bool)
    inside[list(positions)] = True
    ok = pure & ~mism[:, slice_positions(s, width)].any(axis=1)
    if successor_mismatches is None:
        ok &= ~mism[:, ~inside].any(axis=1)
    else:
        succ = np.zeros(SEQ_LEN, dtype=bool)
        succ[successor_positions(s, width)] = True
        assert not (succ & inside).any()
        ok &= ~mism[:, ~inside & ~succ].any(axis=1) & (mism[:, succ].sum(axis=1) == successor_mismatches)
    weights = np.uint64(1) << np.arange(len(positions), dtype=np.uint64)
    return np.unique((mism[ok][:, list(positions)].astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64))


def subsets_up_to(n, k):
    """Sorted bit masks of every subset of at most k of n positions."""
    out = [sum(1 << i for i in combo) for size in range(k + 1) for combo in itertools.combinations(range(n), size)]
    return np.array(sorted(out), dtype=np.uint64)


class World:
    """The index of the fixture for one slice width, its oracle, and what the oracle says (computed once, never changed).
    write_index(path, sigs, occ, width) is the caller's: the host builder of the package."""

    def __init__(self, tmp, width, write_index):
        import oracle_util as ou
        self.width, self.n = width, fixture()
        self.path = tmp / f"neighbourhood{width}.issl"
        write_index(self.path, self.n.sigs, self.n.occ, width)
        self.oracle = ou.OracleIndex(self.path)
        self._want = {}

    def want(self, batch, dist, thr):
        """-> (mit, cfd, hits) of the oracle, method `and`."""
        key = (batch, dist, float(thr))
        if key not in self._want:
            got = self.oracle.score(self.n.batches[batch], dist, thr, "and", want_hits=True)
            for a in got:
                a.setflags(write=False)
            self._want[key] = got
        return self._want[key]

    def close(self):
        self.oracle.close()
