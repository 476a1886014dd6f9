"""The pruned plan's binning after its split (issl_bin.hip: k_guide_scatter writes the guides' signatures in bucket order,
k_fine_count reads them there, k_fine_scatter's workgroups [0, nb) write a bucket's items and [nb, 2 nb) place its guides):
scores bit for bit against the CPU oracle, with the comparison tests/test_gpu_parity.py makes -- MIT and CFD as 64-bit
patterns, the comparison counters of the call (check_comparisons), the plan that was asked for.

  * batch sizes 1 and 102 (the one-launch binning, k_bin_small), 103 (the first batch of the seven launches), 1 000, 10 000 and
    100 000 (a bucket's guides: one trip of the 512 threads, and several),
  * prune = 0 / 1 / -1 (whole buckets, successor-byte groups, the planner's choice), max_dist 2 and 4 (1 and 13 places per guide),
  * an index of a few thousand sites: most successor-byte groups of a bucket are empty and take no guides (has_cands),
  * a batch whose guides share one bucket and one successor byte: the group holds more guides than an item takes
    (item_guides; kk > 1 chunks), at the default item size and at a small one."""
import numpy as np
import pytest
import torch

import crackling_amd as ca
import oracle_util as ou
from synth import random_sites, random_guides, random_guides_fast, check_comparisons

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

SIZES = [1, 102, 103, 1_000, 10_000, 100_000]


class _Index:
    """A synthetic index on the GPU, the oracle on the same file, and the oracle's scores of the batches asked so far."""

    def __init__(self, tmp, name, n_sites, seed):
        self.sigs, occ = random_sites(n_sites, seed=seed)
        host = ca.IsslIndex.build_from_sites(self.sigs, occ)
        path = tmp / f"{name}.issl"
        host.write(path)
        self.ix = host.upload(0)
        self.oracle = ou.OracleIndex(path)
        self.want = {}

    def guides(self, n, seed=4711):
        if n <= 1000:
            return random_guides(self.sigs, n, seed=seed + n)
        return random_guides_fast(self.sigs, n, seed=seed + n)

    def check(self, guides, key, dist, prune):
        if (key, dist) not in self.want:
            self.want[(key, dist)] = self.oracle.score(guides, dist, 75.0, "and")
        omit, ocfd = self.want[(key, dist)]
        self.ix.set_option("prune", prune)
        try:
            mit, cfd = self.ix.score(guides, dist, 75.0, "and")
            # (the exact plan where the model takes about a second: up to 10 000 guides)
            st = check_comparisons(self.ix, guides, prune, self.sigs if len(guides) <= 10_000 else None, dist)
        finally:
            self.ix.set_option("prune", -1)
        if prune == 1:
            assert st["pruned"] == (1 if dist <= 2 else 2), (key, dist)
        assert np.array_equal(mit.view(np.uint64), omit.view(np.uint64)), ("MIT not bit-identical", key, dist, prune)
        assert np.array_equal(cfd.view(np.uint64), ocfd.view(np.uint64)), ("CFD not bit-identical", key, dist, prune)

    def close(self):
        self.ix.close()
        self.oracle.close()


@pytest.fixture(scope="module")
def even(tmp_path_factory):
    """400 k sites: ~300 per bucket, one or two in a successor-byte group."""
    x = _Index(tmp_path_factory.mktemp("binsplit"), "even", 400_000, seed=3101)
    yield x
    x.close()


@pytest.fixture(scope="module")
def sparse(tmp_path_factory):
    """3 000 sites: two or three per bucket, so nearly every successor-byte group of a bucket is empty."""
    x = _Index(tmp_path_factory.mktemp("binsplit"), "sparse", 3_000, seed=3102)
    yield x
    x.close()


@pytest.mark.parametrize("dist", [2, 4])
@pytest.mark.parametrize("prune", [0, 1, -1], ids=["full", "pruned", "auto"])
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_match_oracle(even, n, prune, dist):
    even.check(even.guides(n), n, dist, prune)


@pytest.mark.parametrize("dist", [2, 4])
@pytest.mark.parametrize("prune", [0, 1, -1], ids=["full", "pruned", "auto"])
@pytest.mark.parametrize("n", SIZES)
def test_empty_groups_take_no_guides(sparse, n, prune, dist):
    assert len(sparse.sigs) < 5_000  # (a few thousand sites over 1280 buckets x 256 groups)
    sparse.check(sparse.guides(n), n, dist, prune)


@pytest.mark.parametrize("dist", [2, 4])
@pytest.mark.parametrize("item_guides", [512, 64])
def test_group_spills_over_item_guides(even, item_guides, dist):
    """3 000 guides that agree with one site in slices 0, 1 and 2: in bucket (slice 0) they all sit in the group of the
    site's own successor byte -- which has that site as a candidate --, six chunks of 512 guides or 47 of 64; the same
    holds in their bucket of slice 1.  The other slices spread them over their buckets."""
    rng = np.random.default_rng(12)
    n = 3_000
    guides = even.sigs[777:778].repeat(n) ^ (rng.integers(0, 1 << 16, size=n, dtype=np.uint64) << np.uint64(24))
    assert n > 5 * item_guides
    even.ix.set_option("item_guides", str(item_guides))
    try:
        for prune in (1, -1, 0):
            even.check(guides, "spill", dist, prune)
    finally:
        even.ix.set_option("item_guides", 512)
