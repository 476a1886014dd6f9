"""Guides with a prescribed number of hits in every slice, for the many-hit side of the scoring tail (k_replay_mid, both builds
of k_replay_big, the grouping pass): tests/test_many_hit_construction.py checks the construction with the CPU oracle alone,
tests/test_replay_many_hits.py scores it on the GPU.

Geometry: 20 positions, position j at bits 2j (synth.text_order_key), five slices of four positions (8-bit slices).  A site
within four substitutions of a guide is scored once, under the FIRST slice in which the two agree exactly; so a site with a
substitution in every slice before s and none in slice s is a slice-s hit.  Site ids are ranks in text order (position 0
first): all slice-0 hits of a guide share its first four bases and lie in one stretch of the table.

Ids are RANKS, so a substitution at position 4 does not by itself move an id far: what stretches the range a slice's ids
span is the number of OTHER sites that sort in between.  The "piled+outliers" rows therefore come with `filler_between`:
sites that share the centre's first four bases, sort between the pile and the outliers and are far from the centre."""
import pathlib
import re

import numpy as np

from synth import text_order_key

ROOT = pathlib.Path(__file__).resolve().parent.parent

# The sizes the kernels switch at, as the fixture was laid out for them; source_constants() reads the same names out of
# crackling_amd/csrc and the construction test compares: a constant that moves fails there first.
REPLAY_LDS = 512      # kReplayLds: k_replay | k_replay_mid; k_verify's `overflowed`
MID_HITS = 2048       # kMidHits: k_replay_mid | k_replay_big; terms from k_verify, copied by k_group_scatter
MID_SLICE = 1024      # kMidSlice: a longer slice is handed on to k_replay_big
MID_DIRECT = 256      # kMidDirect: rank_against_all<1> | ranking inside id groups
BIG_SMALL = 16384     # kBigSmall: 256-thread | 1024-thread build of k_replay_big
BIG_BUILDS = {256: 2048, 1024: 7680}   # THREADS -> LDS_HITS of the two builds
HEAD_RUN = 384        # the head pass takes leading id groups until they hold this many hits
PREFIX_SINGLE = 1 << 18   # launch_group_hits: k_prefix_single up to this many counts (n + 1)
SCAN_CHUNK = 2048     # kScanChunk; a k_prefix_apply thread owns 8 consecutive counts
SPECIAL_SMALL = (254, 255, 256)                    # the saturation points of the image's 8- ...
SPECIAL_BIG = (0xFFFFFE, 0xFFFFFF, 0x1000000)      # ... and 24-bit copies of the occurrence count (tests/test_replay_network.py)
N_OUTLIERS = 8


def head_max(threads):
    """kHeadMax of k_replay_big<THREADS, LDS_HITS>: what rank_sort_slice<4> takes."""
    return min(4 * threads, BIG_BUILDS[threads])


def source_constants():
    """The same numbers as the kernels' source states them."""
    src = ROOT / "crackling_amd" / "csrc"
    text = (src / "issl_kernels.hpp").read_text() + (src / "issl_replay.hip").read_text() + (src / "issl_group.hip").read_text()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    builds = {}
    for threads, lds in re.findall(r"\(k_replay_big<(\d+), (\w+)>\)", text):
        builds[int(threads)] = int(lds) if lds.isdigit() else const(lds)
    return {"REPLAY_LDS": const("kReplayLds"), "MID_HITS": const("kMidHits"), "MID_SLICE": const("kMidSlice"),
            "MID_DIRECT": const("kMidDirect"), "BIG_SMALL": const("kBigSmall"), "BIG_BUILDS": builds,
            "HEAD_RUN": int(re.search(r"run < (\d+)u\) run \+= group_cur", text).group(1)),
            "PREFIX_SINGLE": 1 << int(re.search(r"m <= \(1u << (\d+)\)", text).group(1)),
            "SCAN_CHUNK": const("kScanChunk"),
            "HEAD_MAX_IS_MIN_OF_4_THREADS_AND_LDS": "kHeadMax = 4u * THREADS < LDS_HITS ? 4u * THREADS : LDS_HITS" in text}


def mismatches(a, b):
    """Number of positions in which the 20-mers differ."""
    x = np.bitwise_xor(np.asarray(a, dtype=np.uint64), np.uint64(b))
    x = (x | (x >> np.uint64(1))) & np.uint64(0x5555555555)
    x = (x & np.uint64(0x3333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101)) >> np.uint64(32)) & np.uint64(0xFF)


def _draw(centre, m, mandatory, free, extra_min, extra_max, rng):
    """m variants of `centre` (not distinct): one substitution in every slice of `mandatory`, extra_min..extra_max more at
    distinct positions of `free`, uniform over the variants there are."""
    from math import comb
    out = np.full(m, centre, dtype=np.uint64)
    rows = np.arange(m)
    r = rng.random((m, 20))
    allowed = np.zeros(20, dtype=bool)
    allowed[np.asarray(free, dtype=np.int64)] = True
    r[:, ~allowed] = 2.0
    for s in mandatory:
        pos = 4 * s + rng.integers(0, 4, size=m)
        out ^= rng.integers(1, 4, size=m).astype(np.uint64) << (2 * pos).astype(np.uint64)
        r[rows, pos] = 2.0
    n_free = int(allowed.sum()) - sum(1 for s in mandatory if allowed[4 * s:4 * s + 4].any())
    ks = np.arange(extra_min, extra_max + 1)
    w = np.array([comb(n_free, int(k)) * 3.0 ** int(k) for k in ks])
    extra = rng.choice(ks, size=m, p=w / w.sum())
    order = np.argsort(r, axis=1)
    for k in range(extra_max):
        pos = order[:, k]
        sub = rng.integers(1, 4, size=m).astype(np.uint64) << (2 * pos).astype(np.uint64)
        out = np.where(extra > k, out ^ sub, out)
    return out


def _distinct(count, draw, rng):
    """`count` distinct values of draw(m), in random order."""
    have = np.empty(0, dtype=np.uint64)
    for _ in range(400):
        if len(have) >= count:
            return rng.permutation(have)[:count]
        have = np.unique(np.concatenate([have, draw(2 * (count - len(have)) + 256)]))
    raise AssertionError("not enough distinct variants for %d" % count)


def neighbourhood(centre, per_slice_counts, id_shape, rng):
    """Distinct site signatures within four substitutions of `centre` (the centre itself not among them), exactly
    per_slice_counts[s] of them with s as their first exactly matching slice: a substitution in every slice before s, none
    in slice s.  `id_shape` says where the substitutions of the slice-0 hits fall (positions 4..19 in any case):
      "spread"          anywhere: the ids fall in many of the 256 groups of the range they span;
      "piled"           in the last seven positions only: consecutive ids;
      "piled+outliers"  as "piled", and N_OUTLIERS hits whose position 4 is T (the centre's must be A): they sort behind
                        everything that has the centre's first four bases and C or G at position 4 (filler_between)."""
    centre = int(centre)
    parts = []
    for s, count in enumerate(per_slice_counts):
        if count == 0:
            continue
        free = [j for j in range(20) if j // 4 != s]
        if s > 0 or id_shape == "spread":
            parts.append(_distinct(count, lambda m: _draw(centre, m, range(s), free, 1 if s == 0 else 0, 4 - s, rng), rng))
            continue
        last7 = list(range(13, 20))
        n_out = N_OUTLIERS if id_shape == "piled+outliers" else 0
        assert id_shape in ("piled", "piled+outliers") and count > n_out
        parts.append(_distinct(count - n_out, lambda m: _draw(centre, m, (), last7, 1, 4, rng), rng))
        if n_out:
            assert (centre >> 8) & 3 == 0, "piled+outliers wants A at position 4 of the centre"
            parts.append(_distinct(n_out, lambda m: _draw(centre ^ (3 << 8), m, (), last7, 0, 3, rng), rng))
    out = np.concatenate(parts)
    assert len(np.unique(out)) == len(out) == sum(per_slice_counts) and centre not in out
    return out


def filler_between(centre, n, rng):
    """About n sites with the centre's first four bases, C or G at position 4 (the centre has A there) and random bases
    behind, none within four substitutions of the centre: in text order they lie between the centre's pile and its outliers,
    and they are candidates of its slice 0 that the exact test rejects."""
    centre = int(centre)
    assert (centre >> 8) & 3 == 0
    tail = rng.integers(0, 1 << 30, size=n, dtype=np.uint64) << np.uint64(10)
    pos4 = rng.integers(1, 3, size=n).astype(np.uint64) << np.uint64(8)
    out = np.unique(np.uint64(centre & 0xFF) | pos4 | tail)
    return out[mismatches(out, centre) > 4]


# name, hits per slice, id shape of slice 0, filler sites, what the row pins
_EVEN = lambda total: [total // 5 + (1 if s < total % 5 else 0) for s in range(5)]   # noqa: E731
ROWS = [
    ("t512", _EVEN(512), "spread", 0, "last guide of k_replay"),
    ("t513", _EVEN(513), "spread", 0, "first guide of k_replay_mid: one hit beyond the narrow slots"),
    ("t2047", _EVEN(2047), "spread", 0, "kMidHits - 1"),
    ("t2048", _EVEN(2048), "spread", 0, "kMidHits: last guide of k_replay_mid, the rank-2047 hit"),
    ("t2049", _EVEN(2049), "spread", 0, "kMidHits + 1: k_replay_big makes the terms"),
    ("direct256", [256, 100, 100, 100, 100], "spread", 0, "kMidDirect: rank_against_all<1>"),
    ("direct257", [257, 100, 100, 100, 100], "spread", 0, "kMidDirect + 1: ranked inside id groups"),
    ("slice1024", [1024, 120, 120, 120, 116], "spread", 0, "kMidSlice: kept by k_replay_mid"),
    ("slice1025", [1025, 120, 120, 120, 115], "spread", 0, "kMidSlice + 1: handed on to k_replay_big"),
    ("quarter", [600, 150, 150, 150, 150], "piled+outliers", 40000, "k_replay_mid: largest group holds more than a quarter"),
    ("late", [40, 3, 2, 900, 255], "spread", 0, "hits start in a late slice"),
    ("head256", [256, 700, 700, 700, 700], "spread", 0, "k_replay_big<256>: len == THREADS, no head pass in slice 0"),
    ("head257", [257, 700, 700, 700, 699], "spread", 0, "k_replay_big<256>: len == THREADS + 1, head pass"),
    ("lds2048", [2048, 1000, 1000, 1000, 952], "spread", 0, "LDS_HITS of the 256-thread build: sorted in LDS"),
    ("lds2049", [2049, 1000, 1000, 1000, 951], "spread", 0, "LDS_HITS + 1: group order, run by run"),
    ("network", [2100, 1000, 1000, 1000, 900], "piled+outliers", 530000, "one id group beyond LDS_HITS: wave_sort in HBM"),
    ("headskip", [3000, 800, 800, 800, 600], "piled+outliers", 300000, "first id group beyond kHeadMax: head counted, not walked"),
    ("big16384", [6000, 3000, 3000, 3000, 1384], "spread", 0, "kBigSmall: 256-thread build, near end of gcur_big2"),
    ("big16385", [6000, 3000, 3000, 3000, 1385], "spread", 0, "kBigSmall + 1: 1024-thread build, far end of gcur_big2"),
    ("lds7680", [7680, 4000, 4000, 3000, 1320], "spread", 0, "LDS_HITS of the 1024-thread build"),
    ("lds7681", [7681, 4000, 4000, 3000, 1319], "spread", 0, "LDS_HITS + 1 of the 1024-thread build"),
    ("twoheads", [6000, 6000, 3000, 3000, 2000], "spread", 0, "head pass in slice 0 and in slice 1: per-slice state"),
    # (not in the issue's table: behind a walked head, lds2049 and lds7681 have ONE run left -- these two have three)
    ("runs256", [5000, 1000, 1000, 500, 500], "spread", 0, "256-thread build: head, then several runs of id groups"),
    ("runs1024", [17000, 1000, 1000, 500, 500], "spread", 0, "1024-thread build: head, then several runs of id groups"),
]
ROW = {r[0]: i for i, r in enumerate(ROWS)}


def far_apart_centres(n, rng, a_at_4=()):
    """n random 20-mers, every pair at least ten substitutions apart (neighbourhoods of radius four, and those of the
    centres after one more substitution, do not meet); A at position 4 for the indexes in a_at_4."""
    out = []
    while len(out) < n:
        c = int(rng.integers(0, 1 << 40, dtype=np.uint64))
        if len(out) in a_at_4:
            c &= ~(3 << 8)
        if all(int(mismatches(np.array([c], dtype=np.uint64), o)[0]) >= 10 for o in out):
            out.append(c)
    return np.array(out, dtype=np.uint64)


def clear_of(sites, centres):
    """The sites that are no hit of any centre (a random 20-mer is one with probability 4e-7: among a million, a few are)."""
    keep = np.ones(len(sites), dtype=bool)
    for c in centres:
        keep &= mismatches(sites, c) > 4
    return sites[keep]


def _assemble(centres, rows, n_background, rng):
    """-> sites in text order, occurrence counts 1..3 with the saturation values on a few hits of every neighbourhood: the
    small ones anywhere, the large ones (one of them ends every walk it is part of, at any threshold but 0) in the later
    slices, so that the exits of the other thresholds spread over the first slices."""
    sites, occ = [], []
    for c, (name, counts, shape, n_fill, _) in zip(centres, rows):
        near = neighbourhood(c, counts, shape, rng)
        o = rng.integers(1, 4, size=len(near)).astype(np.uint32)
        o[rng.choice(len(near), size=len(SPECIAL_SMALL), replace=False)] = SPECIAL_SMALL
        late = np.flatnonzero(np.arange(len(near)) >= sum(counts[:3])) if sum(counts[3:]) >= 8 else np.arange(len(near))
        o[rng.choice(late, size=len(SPECIAL_BIG), replace=False)] = SPECIAL_BIG
        sites.append(near)
        occ.append(o)
        if n_fill:
            fill = clear_of(filler_between(c, n_fill, rng), centres)
            sites.append(fill)
            occ.append(rng.integers(1, 4, size=len(fill)).astype(np.uint32))
    background = clear_of(rng.integers(0, 1 << 40, size=n_background, dtype=np.uint64), centres)
    sites = np.concatenate(sites + [background])
    occ = np.concatenate(occ + [rng.integers(1, 4, size=len(background)).astype(np.uint32)])
    sites, first = np.unique(sites, return_index=True)
    occ = occ[first]
    order = np.argsort(text_order_key(sites), kind="stable")
    return sites[order], occ[order], background


class Case:
    """An index file, its oracle, the guides and what the oracle says about them (computed once, shared, never changed)."""

    def __init__(self, path, oracle, **kw):
        self.path, self.oracle = path, oracle
        self.__dict__.update(kw)
        self._scores, self._hits = {}, {}

    def scores(self, guides_key, method, thr):
        key = (guides_key, method, float(thr))
        if key not in self._scores:
            mit, cfd = self.oracle.score(getattr(self, guides_key), 4, thr, method)
            mit.setflags(write=False); cfd.setflags(write=False)
            self._scores[key] = (mit, cfd)
        return self._scores[key]

    def hits(self, guides_key, method, thr):
        key = (guides_key, method, float(thr))
        if key not in self._hits:
            _, _, hits = self.oracle.score(getattr(self, guides_key), 4, thr, method, want_hits=True)
            hits.setflags(write=False)
            self._hits[key] = hits
        return self._hits[key]


def _write_index(sig, occ, path):
    import crackling_amd as ca
    ix = ca.IsslIndex.build_from_sites(sig, occ)
    ix.write(path)
    ix.close()


_CASES = {}


def main_case(tmp_path_factory):
    """The index of ROWS, one centre per row, and the guide batches."""
    if "main" in _CASES:
        return _CASES["main"]
    import oracle_util as ou
    rng = np.random.default_rng(51320)
    centres = far_apart_centres(len(ROWS), rng, a_at_4=[i for i, r in enumerate(ROWS) if r[2] == "piled+outliers"])
    sig, occ, background = _assemble(centres, ROWS, 3000, rng)
    path = tmp_path_factory.mktemp("many_hits") / "rows.issl"
    _write_index(sig, occ, path)
    # the centre again after one substitution inside slice 0: its whole neighbourhood moves to later slices or out of reach
    moved = centres ^ (rng.integers(1, 4, size=len(centres)).astype(np.uint64) << (2 * rng.integers(0, 4, size=len(centres))).astype(np.uint64))
    guides = np.concatenate([centres, moved, rng.permutation(np.repeat(centres, 2))])
    few = np.concatenate([background[:48], rng.integers(0, 1 << 40, size=16, dtype=np.uint64)])   # one hit (itself) or none
    mixed = rng.permutation(np.concatenate([guides, few]))
    case = Case(path, ou.OracleIndex(path), centres=centres, guides=guides, few=few, mixed=mixed, sites=sig, occ=occ)
    _CASES["main"] = case
    return case


# ------------------------------------------------------------------------------------------------
# the kernels' grouping of a slice's ids, restated in numpy
# ------------------------------------------------------------------------------------------------

def id_groups(ids):
    """(shift, sizes of the 256 groups): group = (id - min) >> shift, the shift that brings the range below 256
    (k_replay_mid, rank_sort_slice_grouped and the head pass of k_replay_big state it alike)."""
    ids = np.asarray(ids, dtype=np.int64)
    low, top = int(ids.min()), int(ids.max() - ids.min())
    shift = 0 if top < 256 else top.bit_length() - 8   # 24 - clz(top)
    return shift, np.bincount((ids - low) >> shift, minlength=256)


def big_slice_plan(ids, threads):
    """How k_replay_big<threads> walks a slice with these ids: {"head": hits walked by the head pass (0: none), "groups":
    leading groups it counted, "first_group", "group_order": the slice is beyond the LDS and goes into group order, "runs":
    [(first hit, hits, through the HBM network)] behind the head, in scoring order}."""
    lds, n = BIG_BUILDS[threads], len(ids)
    plan = {"head": 0, "groups": 0, "counted": 0, "first_group": 0, "runs": [], "group_order": n > lds}
    done = 0
    sizes = None
    if n > threads:
        _, sizes = id_groups(ids)
        run = nb = 0
        while nb < 256 and run < HEAD_RUN:
            run += int(sizes[nb])
            nb += 1
        plan.update(groups=nb, counted=run, first_group=int(sizes[0]))
        if run <= head_max(threads) and run < n:
            plan["head"] = run
            done = nb
    if plan["head"] == n:
        return plan
    if n <= lds:
        plan["runs"].append((plan["head"], n - plan["head"], False))
        return plan
    at = np.concatenate([[0], np.cumsum(sizes)])
    g_lo = done
    while g_lo < 256:
        start = int(at[g_lo])
        g_hi = g_lo + 1
        while g_hi < 256 and int(at[g_hi + 1]) - start <= lds:
            g_hi += 1
        m = int(at[g_hi]) - start
        g_lo = g_hi
        if m:
            plan["runs"].append((start, m, m > lds))
    return plan


def replay_kernel(per_slice):
    """Which replay scores a guide with these hits per slice: "wave", "mid", "big256" or "big1024"."""
    total = int(sum(per_slice))
    if total <= REPLAY_LDS:
        return "wave"
    if total <= MID_HITS and max(per_slice) <= MID_SLICE:
        return "mid"
    return "big256" if total <= BIG_SMALL else "big1024"


def exit_situation(hits0, kept, threads):
    """Where the walk of a k_replay_big guide ends when it scores `kept` of its hits (hits0: the oracle's list at threshold
    0 for the guide, columns slice and id): "none", "head" (inside a head pass of the first slice), "first_run" (in the
    first run behind that head), "later" (a later run, or a later slice), or "other"."""
    if kept >= len(hits0):
        return "none"
    slices = hits0[:, 1]
    s = int(slices[kept - 1])
    if s != int(slices[0]):
        return "later"
    r = kept   # hits walked in the first slice
    plan = big_slice_plan(hits0[slices == s, 3], threads)
    if plan["head"] == 0:
        return "other" if not plan["runs"] or r <= plan["runs"][0][1] else "later"
    if r <= plan["head"]:
        return "head"
    return "first_run" if r <= plan["runs"][0][0] + plan["runs"][0][1] else "later"


LADDER = [0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 35.0, 50.0, 65.0, 75.0, 85.0, 90.0, 95.0, 99.0]
SITUATIONS = ("head", "first_run", "later", "none")


def choose_thresholds(case):
    """One threshold per exit situation, read off the ORACLE's kept counts (method and) of the rows that k_replay_big
    scores: for each situation the ladder's threshold that puts most rows into it.  -> ({situation: threshold},
    {(row, threshold): situation})."""
    if hasattr(case, "_thresholds"):
        return case._thresholds
    big = [i for i, r in enumerate(ROWS) if replay_kernel(r[1]).startswith("big")]
    hits0 = case.hits("centres", "and", 0.0)
    per_row = {i: hits0[hits0[:, 0] == i] for i in big}
    table = {}
    for thr in LADDER:
        kept = np.bincount(case.hits("centres", "and", thr)[:, 0], minlength=len(ROWS))
        for i in big:
            table[(ROWS[i][0], thr)] = exit_situation(per_row[i], int(kept[i]), int(replay_kernel(ROWS[i][1])[3:]))
    chosen = {"none": 0.0}
    for sit in SITUATIONS[:3]:
        votes = [sum(1 for (_, t), s in table.items() if t == thr and s == sit) for thr in LADDER]
        assert max(votes) > 0, "fixture error: no row and no threshold of the ladder ends its walk in situation '%s'" % sit
        chosen[sit] = LADDER[int(np.argmax(votes))]
    case._thresholds = (chosen, table)
    return case._thresholds


# ------------------------------------------------------------------------------------------------
# many-hit guides in batches on both sides of the one-workgroup prefix sum
# ------------------------------------------------------------------------------------------------

PREFIX_ROWS = [
    ("p600", [120, 120, 120, 120, 120], "spread", 0, "k_replay_mid"),
    ("p1500", [1100, 100, 100, 100, 100], "spread", 0, "handed on by k_replay_mid"),
    ("p2500", [500, 500, 500, 500, 500], "spread", 0, "k_replay_big"),
]
PREFIX_RANDOM_PLACES = 2100   # with the fixed places: more entries than k_replay_mid has workgroups (2048)


def prefix_case(tmp_path_factory):
    """A small index -- 10 k background sites, three neighbourhoods -- and the pool of distinct guides the large batches
    are made of: the three centres, 2048 background sites (one hit each) and 2048 random 20-mers."""
    if "prefix" in _CASES:
        return _CASES["prefix"]
    import oracle_util as ou
    rng = np.random.default_rng(77218)
    centres = far_apart_centres(len(PREFIX_ROWS), rng)
    sig, occ, background = _assemble(centres, PREFIX_ROWS, 10000, rng)
    path = tmp_path_factory.mktemp("many_hits_prefix") / "small.issl"
    _write_index(sig, occ, path)
    pool = np.concatenate([centres, background[:2048], rng.integers(0, 1 << 40, size=2048, dtype=np.uint64)])
    case = Case(path, ou.OracleIndex(path), centres=centres, pool=pool, sites=sig, occ=occ)
    _CASES["prefix"] = case
    return case


def prefix_places(n, rng):
    """Where the three centres stand in a batch of n guides (in turn): both ends of a k_prefix_apply thread's eight
    counts, both sides of kScanChunk, the last guide, eight in a row inside one thread's run, and random places."""
    fixed = [0, 7, 8, SCAN_CHUNK - 1, SCAN_CHUNK, n - 1] + list(range(5 * 8192 + 64, 5 * 8192 + 72))
    rest = np.setdiff1d(rng.choice(n, size=PREFIX_RANDOM_PLACES, replace=False), fixed)
    return np.concatenate([np.array(fixed, dtype=np.int64), rest.astype(np.int64)])


def prefix_batch(case, n, seed):
    """-> (guides[n], index into case.pool per guide)."""
    rng = np.random.default_rng(seed)
    which = rng.integers(len(PREFIX_ROWS), len(case.pool), size=n)
    places = prefix_places(n, rng)
    which[places] = np.arange(len(places)) % len(PREFIX_ROWS)
    return case.pool[which], which
