"""k_replay's ways of putting a guide's hits in scoring order: rank by counting, the sort network in registers (two and four
words per lane), the network in LDS.  Single guides with hit counts on both sides of every size the kernel switches at must
give the CPU oracle's doubles bit for bit and its hit lists in order, from the plain kernel and from the one that expands
the records (issl_dump_hits)."""
import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
from synth import text_order_key

pytestmark = pytest.mark.gpu

# 64: rank by counting; 128 / 256: two / four words per lane in registers; 512: the LDS network and the wave's last size
HIT_COUNTS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
METHODS = ["and", "or", "avg", "mit", "cfd"]
THRESHOLDS = [0.0, 75.0]


def _neighbourhoods(rng):
    """One centre per entry of HIT_COUNTS with exactly that many distinct sites within four substitutions of it (the centre
    itself not among them), far from every other centre; occurrence counts at and around the saturation points of the
    image's 8- and 24-bit copies on some of them.  A site with one or two substitutions matches the centre in three or
    four of its five slices: the scan finds it once per slice, the replay scores it once."""
    centres = rng.integers(0, 1 << 40, size=len(HIT_COUNTS), dtype=np.uint64)
    sites, occ = [], []
    for c, count in zip(centres, HIT_COUNTS):
        near = set()
        while len(near) < count:
            s = int(c)
            for p in rng.choice(20, size=int(rng.integers(1, 5)), replace=False):
                s ^= int(rng.integers(1, 4)) << (2 * int(p))
            near.add(s)
        near = sorted(near)
        o = rng.integers(1, 4, size=len(near)).astype(np.uint32)
        special = np.array([0xFFFFFF, 0x1000000, 0xFFFFFE, 255, 256, 0x1000005, 254], dtype=np.uint32)
        at = rng.choice(len(near), size=min(len(near), len(special)), replace=False)
        o[at] = special[:len(at)]
        sites += near
        occ += o.tolist()
    background = rng.integers(0, 1 << 40, size=3000, dtype=np.uint64)
    sites = np.array(sites + background.tolist(), dtype=np.uint64)
    occ = np.array(occ + rng.integers(1, 4, size=len(background)).tolist(), dtype=np.uint32)
    sites, first = np.unique(sites, return_index=True)
    occ = occ[first]
    order = np.argsort(text_order_key(sites), kind="stable")
    return centres, sites[order], occ[order]


@pytest.fixture(scope="module")
def neighbourhoods(tmp_path_factory):
    rng = np.random.default_rng(20240)
    centres, sig, occ = _neighbourhoods(rng)
    ix = ca.IsslIndex.build_from_sites(sig, occ)
    path = tmp_path_factory.mktemp("replay_net") / "sizes.issl"
    ix.write(path)
    ix.close()
    # every centre twice more behind the twelve, in another order: several guides of every size in one launch
    guides = np.concatenate([centres, rng.permutation(np.repeat(centres, 2))])
    oracle = ou.OracleIndex(path)
    yield path, guides, oracle
    oracle.close()


def _open(path):
    ix = ca.IsslIndex.open(path)
    ix.upload(0)
    return ix


def test_every_listed_hit_count_occurs(neighbourhoods):
    path, guides, oracle = neighbourhoods
    _, _, ohits = oracle.score(guides, 4, 0.0, "and", want_hits=True)
    per_guide = np.bincount(ohits[:, 0], minlength=len(guides))
    assert per_guide[:len(HIT_COUNTS)].tolist() == HIT_COUNTS
    assert sorted(set(per_guide.tolist())) == HIT_COUNTS
    ix = _open(path)
    try:
        hits = ix.dump_hits(guides, 4, 0.0, "and")
        assert np.bincount(hits[:, 0], minlength=len(guides)).tolist() == per_guide.tolist()
        assert (hits[:, 5] >= 0xFFFFFF).any() and (hits[:, 5] == 255).any()   # saturated occurrence counts among the scored hits
    finally:
        ix.close()


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("method", METHODS)
def test_sums_match_the_oracle_bit_for_bit(neighbourhoods, method, thr):
    path, guides, oracle = neighbourhoods
    omit, ocfd = oracle.score(guides, 4, thr, method)
    ix = _open(path)
    try:
        for _ in range(2):   # (the second batch of a handle runs without the grouping pass: lean_tail)
            mit, cfd = ix.score(guides, 4, thr, method)
            assert np.array_equal(mit.view(np.uint64), omit.view(np.uint64)), (method, thr)
            assert np.array_equal(cfd.view(np.uint64), ocfd.view(np.uint64)), (method, thr)
    finally:
        ix.close()


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("method", METHODS)
def test_hit_lists_match_the_oracle_in_order(neighbourhoods, method, thr):
    path, guides, oracle = neighbourhoods
    _, _, ohits = oracle.score(guides, 4, thr, method, want_hits=True)
    ix = _open(path)
    try:
        assert np.array_equal(ix.dump_hits(guides, 4, thr, method), ohits), (method, thr)
    finally:
        ix.close()


def test_signed_table_takes_the_careful_pass():
    """tests/golden/signedtable: a score table with negative, NaN and +inf entries, where the totals behind a chunk say
    nothing about the hits inside it (accumulate_chunk's second loop)."""
    from conftest import Golden
    g = Golden("signedtable")
    sigs = ca.encode_guides([s.encode() for s in g.guides])
    oracle = ou.OracleIndex(g.issl)
    ix = _open(g.issl)
    try:
        for method in METHODS:
            for thr in THRESHOLDS:
                omit, ocfd, ohits = oracle.score(sigs, 4, thr, method, want_hits=True)
                mit, cfd = ix.score(sigs, 4, thr, method)
                assert np.array_equal(mit.view(np.uint64), omit.view(np.uint64)), (method, thr)
                assert np.array_equal(cfd.view(np.uint64), ocfd.view(np.uint64)), (method, thr)
                assert np.array_equal(ix.dump_hits(sigs, 4, thr, method), ohits), (method, thr)
    finally:
        ix.close()
        oracle.close()
