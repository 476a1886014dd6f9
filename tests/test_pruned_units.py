"""The short last unit of a successor-byte group and the plan of the pruned scan, on CONSTRUCTED groups: hit lists row for
row and MIT / CFD as 64-bit patterns against the CPU oracle, and the four comparison counters of issl_stats against the
exact models of tests/pruned_model.py.

One index per slice width.  A case is three neighbouring non-empty groups of one bucket of slice 0 -- a lead group of L sites,
the target group of n sites, a trail group of T >= 2100 sites, their successor bytes one position apart and next to each other
in the bucket's order -- so that the target's window starts L % 32 candidates into a lane group, its span n + L % 32 leaves
the remainder the case is named after, its first and last candidate have near neighbours just outside the window, and the
bucket goes on beyond a short unit's cap.  Width 8 gives every case a bucket of its own; the 16 and 4 buckets of the narrow
widths hold several cases each, every case a multiple of 32 sites long, their target bytes at least two positions apart.
The guides of a case are copies of the window's first, last and a middle site, of the last lead and the first trail site, with
0..4 substitutions outside slice 0 and its successor positions and 0 or 1 in the successor byte (both classes in one group), and
their number walks over the pass width of a short unit and its 8-pass mask refill: 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 600."""
import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
import pruned_model as pm
from synth import random_guides, text_order_key

pytestmark = pytest.mark.gpu

# (span = n + L % 32, L, guides): every remainder with the window starting on a lane group and inside one (span 1 cannot
# start inside one: its remainder is there as 2049), every shape edge from both sides in both alignments
CASES = [
    (1, 0, 3), (8, 32, 4), (8, 1, 5), (9, 0, 31), (9, 33, 32), (511, 32, 33), (511, 31, 1), (512, 0, 15), (512, 1, 16),
    (513, 32, 17), (513, 33, 1), (1023, 0, 3), (1023, 31, 4), (1024, 32, 5), (1024, 1, 15), (1025, 0, 16), (1025, 33, 17),
    (2047, 32, 33), (2047, 31, 5), (2048, 0, 1), (2048, 1, 32), (2049, 32, 600), (2049, 33, 4), (2048 + 512, 0, 17),
    (2048 + 512, 31, 3), (2048 + 513, 32, 31), (2048 + 513, 1, 600), (2048 + 1024, 0, 32), (2048 + 1024, 33, 16),
    (2048 + 1025, 32, 15), (2048 + 1025, 31, 31),
]
N_CENTRES = 48


def _shape_of(span):
    rest = span % 2048
    return 32 if rest == 0 or rest > 1024 else 16 if rest > 512 else 8


class Constructed:
    """Sites (text order, with occurrences), guides and, per case, its guide range and the ids of its four edge sites."""

    def __init__(self, width, seed=20261):
        rng = np.random.default_rng([seed, width])
        p = width // 2                       # positions of slice 0; the successor byte is positions p .. p + 3
        nf = 16 - p                          # positions that are neither: p + 4 .. 19, the first of them leads the text order
        per_bucket = {8: 1, 4: 3, 2: 11}[width]
        centres = rng.integers(0, 1 << (2 * nf), size=N_CENTRES, dtype=np.uint64)
        # target bytes: low position 1 or 2 (lead = byte - 1, trail = byte + 1: neighbours in the order, one position away),
        # the other three a code of distance two, so that no guide of a case visits another case's target group
        uppers = [(a | (b << 2) | (((-a - b) % 4) << 4)) << 2 for a in range(4) for b in range(4)]
        self.width, self.cases, site_parts, guide_parts, n_guides = width, [], [], [], 0

        def free_part(m, c0):
            """m distinct values of the nf free positions: c0 with its leading position A, then centres with up to three
            substitutions and C or G in front, then c0 with T in front -- the group's first and last site are near c0."""
            lead_mask = np.uint64(3)
            first, last = c0 & ~lead_mask, c0 | lead_mask
            if m <= 2:
                return [first, last][:m]
            got = np.empty(0, dtype=np.uint64)
            while len(got) < m - 2:
                r = centres[rng.integers(0, N_CENTRES, size=2 * m)]
                for _ in range(3):
                    r = r ^ (rng.integers(0, 4, size=len(r), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, nf, size=len(r)).astype(np.uint64)))
                r = (r & ~lead_mask) | rng.integers(1, 3, size=len(r), dtype=np.uint64)
                got = np.unique(np.concatenate([got, r]))
            return [first] + list(rng.permutation(got)[:m - 2]) + [last]

        def sig(value, byte, free):
            return np.uint64(value) | (np.uint64(byte) << np.uint64(2 * p)) | (np.uint64(free) << np.uint64(2 * (p + 4)))

        for i, (span, lead, g) in enumerate(CASES):
            value, byte = i // per_bucket, uppers[i % per_bucket] | (1 + i % 2)
            n = span - lead % 32
            trail = 2100 + (-(lead + n + 2100)) % 32          # the case is a multiple of 32 long: the next one starts aligned
            c0 = centres[i % N_CENTRES]
            groups = {}
            for name, b, m in (("lead", byte - 1, lead), ("target", byte, n), ("trail", byte + 1, trail)):
                fp = free_part(m, c0)
                groups[name] = np.array(sorted(int(sig(value, b, f)) for f in fp), dtype=np.uint64)
                groups[name] = groups[name][np.argsort(text_order_key(groups[name]), kind="stable")]
                site_parts.append(groups[name])
            t = groups["target"]
            edges = {"target_first": t[0], "target_last": t[-1], "trail_first": groups["trail"][0]}
            anchors = [t[0], t[-1], t[len(t) // 2], groups["trail"][0]]
            if lead:
                edges["lead_last"] = groups["lead"][-1]
                anchors.append(groups["lead"][-1])
            guides = np.empty(g, dtype=np.uint64)
            for j in range(g):
                x = int(anchors[j % len(anchors)])
                # the first guides stay within two substitutions and off the leading free position: near all four edges
                subs = j % 3 if j < 5 else int(rng.integers(0, 5))
                for pos in rng.choice(np.arange(1 if j < 5 else 0, nf), size=subs, replace=False):
                    x ^= int(rng.integers(1, 4)) << (2 * (p + 4 + int(pos)))
                if (j & 1) if j < 5 else int(rng.integers(0, 2)):
                    x ^= int(rng.integers(1, 4)) << (2 * p)     # the byte's low position: still within one of the target's
                guides[j] = x
            guide_parts.append(guides)
            self.cases.append(dict(span=span, lead=lead, n=n, trail=trail, value=value, byte=byte, g0=n_guides, g1=n_guides + g,
                                   edges=edges))
            n_guides += g
        used = len(CASES) // per_bucket + 1   # slice-0 values the cases use (value < used); the random sites keep out of them
        extra = rng.integers(0, 1 << 40, size=4000, dtype=np.uint64)
        low = np.uint64((1 << width) - 1)
        clash = (extra & low) < np.uint64(used)
        extra[clash] = (extra[clash] & ~low) | rng.integers(used, 1 << width, size=int(clash.sum()), dtype=np.uint64)
        sigs = np.unique(np.concatenate(site_parts + [extra]))
        self.sigs = sigs[np.argsort(text_order_key(sigs), kind="stable")]
        assert len(self.sigs) == sum(len(x) for x in site_parts) + len(np.unique(extra)) < 250_000
        self.occ = rng.integers(1, 4, size=len(self.sigs)).astype(np.uint32)
        id_of = {int(s): k for k, s in enumerate(self.sigs)}
        for c in self.cases:
            c["edges"] = {name: id_of[int(s)] for name, s in c["edges"].items()}
        other = random_guides(self.sigs, 300, seed=seed + 1)   # ... and so do the guides that belong to no case
        clash = (other & low) < np.uint64(used)
        other[clash] = (other[clash] & ~low) | rng.integers(used, 1 << width, size=int(clash.sum()), dtype=np.uint64)
        self.guides = np.concatenate(guide_parts + [other])
        # small batches: the first three guides of every case (first, last and a middle site of the window), in chunks below the limit
        head = np.concatenate([np.arange(c["g0"], min(c["g0"] + 3, c["g1"])) for c in self.cases])
        limit = pm.small_batch_limit(width, 4)
        self.small = [head[k:k + limit] for k in range(0, len(head), limit)]

    def check_cases(self):
        """Every case is what its name says: window start, span, shape and guides in the target group -- counted from the
        signatures, slice 0's bucket ordered by the byte behind it."""
        p = self.width // 2
        value = (self.sigs & np.uint64((1 << self.width) - 1)).astype(np.int64)
        byte = ((self.sigs >> np.uint64(2 * p)) & np.uint64(255)).astype(np.int64)
        gvalue = (self.guides & np.uint64((1 << self.width) - 1)).astype(np.int64)
        gbyte = ((self.guides >> np.uint64(2 * p)) & np.uint64(255)).astype(np.int64)
        seen = set()
        for c in self.cases:
            mine = value == c["value"]
            s0 = int((mine & (byte < c["byte"])).sum())
            s1 = s0 + int((mine & (byte == c["byte"])).sum())
            blen = int(mine.sum())
            assert s1 - s0 == c["n"] and s0 % 32 == c["lead"] % 32 and s1 - (s0 & ~31) == c["span"], c
            assert (c["lead"] == 0) == (int((mine & (byte == c["byte"] - 1)).sum()) == 0), c
            assert int((mine & (byte == c["byte"] + 1)).sum()) == c["trail"] >= 2100 and blen - s1 >= 2100, c
            for tail, want in ((1, _shape_of(c["span"])), (0, 32)):
                assert int(pm.group_units(s0, s1, blen, tail)[2]) == want, c
            x = gbyte[gvalue == c["value"]] ^ c["byte"]
            landing = int((np.array([bin((v | (v >> 1)) & 0x55).count("1") for v in x]) <= 1).sum())
            assert landing == c["g1"] - c["g0"], c
            seen.add((_shape_of(c["span"]), landing))
        for shape, counts in ((8, (3, 4, 5, 31, 32, 33)), (16, (1, 3, 15, 16, 17))):
            assert all((shape, n) in seen for n in counts), (shape, seen)
        assert sum(1 for s, n in seen if n >= 600) >= 2

    def check_premises(self, hits4):
        """The oracle's max_dist 4 list (threshold 0) has a hit of the case's guides on each edge site of the case."""
        for c in self.cases:
            rows = hits4[(hits4[:, 0] >= c["g0"]) & (hits4[:, 0] < c["g1"])]
            for name, site in c["edges"].items():
                assert (rows[:, 3] == site).any(), (c["span"], c["lead"], name)
            assert set(c["edges"]) >= {"target_first", "target_last", "trail_first"} and (("lead_last" in c["edges"]) == (c["lead"] > 0))


def _subset_hits(hits, pick, n_guides):
    """The rows of a batch's hit list that a sub-batch (ascending guide indices `pick`) has, renumbered: guides are independent."""
    new = np.full(n_guides, -1, dtype=np.int64)
    new[pick] = np.arange(len(pick))
    rows = hits[new[hits[:, 0]] >= 0].copy()
    rows[:, 0] = new[rows[:, 0]]
    return rows


class _World:
    def __init__(self, tmp, width):
        self.c = Constructed(width)
        self.c.check_cases()
        self.path = tmp / f"units{width}.issl"
        host = ca.IsslIndex.build_from_sites(self.c.sigs, self.c.occ, slice_width=width)
        host.write(self.path)
        self.reference = host.count_candidates(self.c.guides)
        self.reference_small = [host.count_candidates(self.c.guides[pick]) for pick in self.c.small]
        host.close()
        self.oracle = ou.OracleIndex(self.path)
        self._want, self._model, self.tables = {}, {}, pm.site_tables(self.c.sigs, width)
        self.c.check_premises(self.want(4, 0.0)[2])

    def want(self, dist, thr):
        if (dist, thr) not in self._want:
            self._want[dist, thr] = self.oracle.score(self.c.guides, dist, thr, "and", want_hits=True, hit_cap=1 << 23)
        return self._want[dist, thr]

    def model(self, pick, dist, item_guides, tail, small):
        key = (pick, dist, item_guides, tail, small)
        if key not in self._model:
            g = self.c.guides if pick is None else self.c.guides[self.c.small[pick]]
            self._model[key] = (pm.planned_comparisons(self.tables, g, dist, self.c.width),) + \
                pm.unit_model(self.tables, g, dist, self.c.width, item_guides, tail, small)
        return self._model[key]


@pytest.fixture(scope="module", params=[8, 4, 2])
def world(request, tmp_path_factory):
    w = _World(tmp_path_factory.mktemp("units"), request.param)
    yield w
    w.oracle.close()


@pytest.fixture(scope="module", params=["sorted", "compact"])
def device_index(request, world):
    ix = ca.IsslIndex.open(world.path)
    for key, value in ({"sorted_layout": 1, "compact": 0} if request.param == "sorted" else {"compact": 1}).items():
        ix.set_option(key, value)
    ix.upload(0)
    assert ix.get_option("is_sorted") == 1 and ix.get_option("is_compact") == (request.param == "compact")
    yield ix
    ix.close()


# (max_dist, threshold, item_guides, scan_blocks, scan_threads, scan_generic, hit_slots): every value of every knob, and
# every pair of values of the knobs that decide which code a short unit runs (distance, item size, range count), at least once
SWEEP = [
    (0, 0.0, 512, 1024, 1024, 0, 1), (0, 75.0, 8, 77, 256, 1, 0),
    (1, 0.0, 8, 4096, 1024, 1, 1), (1, 75.0, 512, 77, 256, 0, 0),
    (2, 0.0, 512, 4096, 256, 1, 0), (2, 75.0, 8, 1024, 1024, 0, 1),
    (3, 0.0, 8, 77, 1024, 0, 0), (3, 75.0, 512, 1024, 256, 1, 1), (3, 0.0, 512, 4096, 1024, 0, 1),
    (4, 0.0, 512, 77, 1024, 1, 1), (4, 75.0, 8, 4096, 256, 0, 0), (4, 0.0, 8, 1024, 256, 1, 0), (4, 75.0, 512, 1024, 1024, 0, 1),
    (5, 0.0, 8, 1024, 1024, 0, 0), (5, 75.0, 512, 77, 256, 1, 1), (5, 0.0, 512, 4096, 256, 0, 1),
]
KNOBS = ("item_guides", "scan_blocks", "scan_threads", "scan_generic", "hit_slots")
DEFAULTS = (512, 1024, 1024, 0, 1)


@pytest.mark.parametrize("dist,thr,item_guides,blocks,threads,generic,slots", SWEEP)
def test_constructed_groups_against_oracle_and_models(world, device_index, dist, thr, item_guides, blocks, threads, generic, slots):
    ix, c = device_index, world.c
    omit, ocfd, ohits = world.want(dist, thr)
    batches = [(None, c.guides, omit, ocfd, ohits, world.reference)]
    for k, pick in enumerate(c.small):
        batches.append((k, c.guides[pick], omit[pick], ocfd[pick], _subset_hits(ohits, pick, len(c.guides)), world.reference_small[k]))
    ix.set_option("prune", 1)
    for knob, value in zip(KNOBS, (item_guides, blocks, threads, generic, slots)):
        ix.set_option(knob, value)
    try:
        for pick, guides, wmit, wcfd, whits, reference in batches:
            small = pick is not None and len(guides) <= pm.small_batch_limit(c.width, dist)
            counted = {}
            for tail in (1, 0):
                ix.set_option("tail_shapes", tail)
                where = (c.width, pick, dist, thr, tail)
                hits = ix.dump_hits(guides, dist, thr, "and")
                assert hits.shape == whits.shape and np.array_equal(hits, whits), where
                mit, cfd = ix.score(guides, dist, thr, "and")
                st = ix.stats()
                assert np.array_equal(mit.view(np.uint64), wmit.view(np.uint64)), ("MIT not bit-identical",) + where
                assert np.array_equal(cfd.view(np.uint64), wcfd.view(np.uint64)), ("CFD not bit-identical",) + where
                planned, tiles, cands = world.model(pick, dist, item_guides, tail, small)
                assert st["pruned"] == (1 if dist <= 2 else 2 if dist <= 4 else 3), where
                assert st["planned_comparisons"] == planned, where
                assert st["scan_tiles"] == tiles, where
                assert st["candidates"] == cands, where
                assert st["reference_comparisons"] == reference, where
                counted[tail] = st["candidates"]
            if dist <= 4:
                assert counted[1] < counted[0], (c.width, pick, dist)   # the short shapes were taken
            else:
                assert counted[1] == counted[0]                         # max_dist 5 plans full shapes only
    finally:
        ix.set_option("prune", -1).set_option("tail_shapes", 1)
        for knob, value in zip(KNOBS, DEFAULTS):
            ix.set_option(knob, value)
