"""A lean batch on the pruned plan runs the build of k_scan whose waves note their records into two buffers of their own
LDS (one chunk's slots each).  A full buffer waits there for the wave's verify tail at the next unit boundary; when both
fill inside one unit the older one is copied to a chunk of the raw buffer, and from a chunk the records go the way they
always went (the read-back tail, k_verify).  A batch that is not lean runs the build that notes into the raw buffer.

  boundaries   one wave, forced tail: growing prefixes of guides that note ONE record each behind a guide that notes a
               cluster's, so that the wave's records cross 127, 128, 254 and 255 (a buffer exactly full, the switch, both
               used); lean, and lean_tail=0 x hit_slots 0 / 1 / 2, the build without the buffers
  one unit     a cluster of 4^4 sites that differ in positions 12..15, and 120 guides one to three substitutions from its
               centre there (one or two give 66): in the buckets of slices 0 and 1 the cluster is one successor-byte group, a
               single short unit notes thousands of records and both buffers fill inside it; 16 waves and one wave
  lean to full two clean batches, then one with a guide of more than 512 hits: the batch runs again in full
  dump, lanes  issl_dump_hits, and lanes 2 and 3 with four batches in flight, on the second construction

Which way a batch's records went is read from three keys of lane 0's last finished batch: ws_scan_lds_buffers (buffers
verified from LDS), ws_scan_raw_top (one past the last chunk a buffer was copied to) and ws_raw_chunks (chunks handed out);
tests/test_scan_lds_paths.py has the shipped default, the accounting of the buffers and a record buffer that is too small.

The constructions are checked with the CPU oracle first (no guide beyond 512 hits where the lane has to stay lean)."""
import re

import numpy as np
import pytest

import oracle_util as ou
from synth import random_sites, sigs_to_text, text_order_key
from test_scan_verify import ROOT, _cluster_world, _open, _same

# (the cluster guide's 16 hits are noted in more than one slice each; with 16 .. 48 records for it, these prefixes cross the four sizes)
PREFIXES = list(range(78, 117)) + list(range(205, 244))


def _sorted_unique(sites):
    sites = np.unique(np.asarray(sites, dtype=np.uint64))
    return sites[np.argsort(text_order_key(sites), kind="stable")]


def _sub(sig, pos, d):
    """The 20-mer with the base at `pos` advanced by d (1..3)."""
    return int(sig) ^ (d << (2 * pos))


def _boundary_world(seed=21, n_single=260):
    """Noise, a cluster of 16 sites (positions 14, 15), one guide next to the cluster's centre and n_single guides that are a
    noise site with one substitution in each of slices 0..3: such a guide meets its site in slice 4 alone -- one record."""
    rng = np.random.default_rng(seed)
    noise, _ = random_sites(6000, seed=seed + 1)
    centre = int(rng.integers(0, 1 << 40))
    cluster = [centre]
    for p in (14, 15):
        cluster = [(x & ~(3 << (2 * p))) | (b << (2 * p)) for x in cluster for b in range(4)]
    sites = _sorted_unique(np.concatenate([noise, np.array(cluster, dtype=np.uint64)]))
    picks = noise[rng.permutation(len(noise))[:n_single]]
    guides = [_sub(centre, 13, 1)]
    for s in picks:
        g = int(s)
        for p in (0, 4, 8, 12):
            g = _sub(g, p, int(rng.integers(1, 4)))
        guides.append(g)
    assert len(set(guides)) == len(guides)
    return sites, np.array(guides, dtype=np.uint64)


def _unit_world(seed=31, n_guides=120):
    """test_scan_verify's cluster world (a guide of which has thousands of hits) with a second, small cluster: 4^4 sites that
    differ in positions 12..15, and guides one to three substitutions from ITS centre in those positions."""
    big_sites, big_guides = _cluster_world()
    rng = np.random.default_rng(seed)
    centre = int(rng.integers(0, 1 << 40))
    positions = (12, 13, 14, 15)
    cluster = [centre]
    for p in positions:
        cluster = [(x & ~(3 << (2 * p))) | (b << (2 * p)) for x in cluster for b in range(4)]
    sites = _sorted_unique(np.concatenate([big_sites, np.array(cluster, dtype=np.uint64)]))
    guides = [_sub(centre, p, d) for p in positions for d in (1, 2, 3)]
    guides += [_sub(_sub(centre, p, d), q, e) for p in positions for q in positions if p < q for d in (1, 2, 3) for e in (1, 2, 3)]
    guides += [_sub(_sub(_sub(centre, 12, d), 13, e), 14, f) for d in (1, 2, 3) for e in (1, 2, 3) for f in (1, 2, 3)]
    guides += [_sub(_sub(_sub(centre, 13, d), 14, e), 15, f) for d in (1, 2, 3) for e in (1, 2, 3) for f in (1, 2, 3)]
    guides = guides[:n_guides]
    assert len(set(guides)) == len(guides) == n_guides
    return sites, np.array(guides, dtype=np.uint64), np.uint64(big_guides[0])


def _case(tmp_path_factory, name, sites, guides):
    """The index file and the oracle's answers, computed once: scores (threshold 75), the hit list, hits per guide."""
    path = tmp_path_factory.mktemp("scan_lds_records") / (name + ".issl")
    path.write_bytes(ou.build_issl(sigs_to_text(sites)))
    oracle = ou.OracleIndex(path)
    want = oracle.score(guides, 4, 75.0, "and")
    hits = oracle.score(guides, 4, 0.0, "and", want_hits=True)[2]
    oracle.close()
    per_guide = np.bincount(hits[:, 0], minlength=len(guides))
    return path, guides, want, hits, per_guide


@pytest.fixture(scope="module")
def boundary_case(tmp_path_factory):
    sites, guides = _boundary_world()
    return _case(tmp_path_factory, "boundary", sites, guides)


@pytest.fixture(scope="module")
def unit_case(tmp_path_factory):
    sites, guides, big = _unit_world()
    path, all_guides, want, hits, per_guide = _case(tmp_path_factory, "unit", sites, np.append(guides, big))
    return path, all_guides, want, hits, per_guide


def _pass_records(hits):
    """The most records one pass can note in the boundary world: the cluster guide's largest hit count in one slice (a single
    guide notes one record).  A buffer closes early only when a pass's records do not fit, so with this p a closed buffer
    holds at least 127 - (p - 1) records."""
    return int(np.bincount(hits[hits[:, 0] == 0][:, 1]).max())


def test_the_constructions(boundary_case, unit_case):
    """The CPU oracle alone: the lane stays lean on both constructions (no guide beyond 512 hits), every single guide of the
    first has exactly one hit, and the added guide of the second has more than 512."""
    _, guides, _, _, per_guide = boundary_case
    assert per_guide.max() <= 512 and per_guide[0] == 16 and np.all(per_guide[1:] == 1), (per_guide[0], per_guide[1:].min(), per_guide[1:].max())
    assert len(guides) > max(PREFIXES)
    assert _pass_records(boundary_case[3]) <= 16
    _, guides, _, _, per_guide = unit_case
    assert len(guides) == 121 and 256 <= per_guide[:-1].min() and per_guide[:-1].max() <= 512, (per_guide[:-1].min(), per_guide[:-1].max())
    assert per_guide[-1] > 512


def _prefix(want, k):
    return want[0][:k], want[1][:k]


def _list_chunks():
    """kListChunks of issl_kernels.hip (a wave's budget is one less), read as test_scan_verify._constant reads the header's."""
    m = re.search(r"constexpr\s+uint32_t\s+kListChunks\s*=\s*(\d+)", (ROOT / "crackling_amd" / "csrc" / "issl_kernels.hip").read_text())
    assert m
    return int(m.group(1))


def _paths(ix):
    """Which way the last batch's records went: (buffers verified from LDS, one past the last chunk a buffer was copied to, chunks handed out)."""
    return ix.get_option("ws_scan_lds_buffers"), ix.get_option("ws_scan_raw_top"), ix.get_option("ws_raw_chunks")


def _first_batch_is_not_lean(ix):
    """A handle's first batch runs k_scan<THR, true, false>: no buffer in LDS, and nothing writes raw_top."""
    assert _paths(ix)[:2] == (0, 0), _paths(ix)


@pytest.fixture(scope="module")
def quiet_guide(boundary_case):
    """A guide without a site within 4 mismatches in the boundary world: a batch of it notes nothing."""
    path = boundary_case[0]
    rng = np.random.default_rng(77)
    oracle = ou.OracleIndex(path)
    try:
        for _ in range(64):
            g = np.array([rng.integers(0, 1 << 40)], dtype=np.uint64)
            if len(oracle.score(g, 4, 0.0, "and", want_hits=True)[2]) == 0:
                return g, oracle.score(g, 4, 75.0, "and")
    finally:
        oracle.close()
    raise AssertionError("no guide without hits")


@pytest.mark.gpu
def test_buffer_boundaries_one_wave_lean(boundary_case, quiet_guide):
    path, guides, want, hits, per_guide = boundary_case
    p = _pass_records(hits)
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("scan_threads", 64).set_option("prune", 1)
    ix.upload(0)
    try:
        assert _same(ix.score(guides[:8], 4, 75.0, "and"), _prefix(want, 8))   # (a clean batch: the lane's next ones are lean)
        _first_batch_is_not_lean(ix)
        # a batch that notes nothing: the chunks a launch hands out by itself (the waves' own)
        assert _same(ix.score(quiet_guide[0], 4, 75.0, "and"), quiet_guide[1])
        assert ix.stats()["hits"] == 0 and ix.get_option("ws_scan_verified") == 0 and _paths(ix)[:2] == (0, 0)
        quiet_chunks = ix.get_option("ws_raw_chunks")
        assert quiet_chunks > 0
        counts = []
        for k in PREFIXES:
            got = ix.score(guides[:k], 4, 75.0, "and")
            st = ix.stats()
            verified = ix.get_option("ws_scan_verified")
            buffers, raw_top, raw_chunks = _paths(ix)
            print("prefix", k, "hits", st["hits"], "ws_scan_verified", verified, "raw_records", st["raw_records"])
            if verified in (127, 128, 254, 255):
                print("  ws_scan_verified", verified, "ws_scan_lds_buffers", buffers, "ws_scan_raw_top", raw_top, "ws_raw_chunks", raw_chunks)
            assert _same(got, _prefix(want, k)), k
            assert st["pruned"] == 2 and st["hits"] == per_guide[:k].sum(), k
            assert st["hits"] <= verified <= st["raw_records"], k
            # fewer than 63 buffers: no record leaves the wave -- no chunk receives a buffer, none is handed out, and every
            # verified record came from a buffer of at most 127; a buffer closes early only by what a pass notes (p records)
            assert raw_top == 0 and raw_chunks == quiet_chunks, k
            assert buffers >= -(-verified // 127), (k, buffers, verified)
            assert (buffers - 1) * (127 - (p - 1)) < verified, (k, buffers, verified)
            counts.append(verified)
        # one wave with a forced tail verifies every record it notes: the prefixes take the wave across a buffer exactly full
        # (127 records), the first record of the second buffer, both full, and the first record behind them
        assert {127, 128, 254, 255} <= set(counts), counts
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [0, 1, 2])
def test_buffer_boundaries_one_wave_not_lean(boundary_case, slots):
    path, guides, want, _, per_guide = boundary_case
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("scan_threads", 64).set_option("prune", 1)
    ix.set_option("lean_tail", 0).set_option("hit_slots", slots)
    ix.upload(0)
    try:
        for k in PREFIXES:
            got = ix.score(guides[:k], 4, 75.0, "and")
            st = ix.stats()
            verified = ix.get_option("ws_scan_verified")
            assert _same(got, _prefix(want, k)), k
            assert st["hits"] == per_guide[:k].sum(), k
            assert st["hits"] <= verified <= st["raw_records"], k
            # lean_tail 0: the launch takes k_scan<THR, true, false>, the first batch as every other
            assert _paths(ix)[:2] == (0, 0), (k, _paths(ix))
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1024, 64])
def test_both_buffers_inside_one_unit(unit_case, threads):
    path, guides, want, _, per_guide = unit_case
    n = len(guides) - 1
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("scan_threads", threads).set_option("prune", 1)
    ix.upload(0)
    try:
        for call in range(3):   # (the first batch is not lean: a lane is lean once it has finished a clean one)
            got = ix.score(guides[:n], 4, 75.0, "and")
            st = ix.stats()
            verified = ix.get_option("ws_scan_verified")
            print("call", call, "hits", st["hits"], "ws_scan_verified", verified, "raw_records", st["raw_records"])
            assert _same(got, _prefix(want, n))
            assert st["pruned"] == 2 and st["hits"] == per_guide[:n].sum()
            assert 0 < verified <= st["raw_records"]
            buffers, raw_top, raw_chunks = _paths(ix)
            print("  ws_scan_lds_buffers", buffers, "ws_scan_raw_top", raw_top, "ws_raw_chunks", raw_chunks)
            if call == 0:
                _first_batch_is_not_lean(ix)
            else:   # both buffers fill inside the cluster's unit: buffers verified from LDS AND buffers copied to chunks
                assert buffers > 0 and 0 < raw_top <= raw_chunks, (call, buffers, raw_top, raw_chunks)
                if threads == 64:   # (one wave's budget)
                    assert buffers <= _list_chunks() - 1, (call, buffers)
    finally:
        ix.close()


@pytest.mark.gpu
def test_lean_to_full_and_back(unit_case):
    path, guides, want, _, per_guide = unit_case
    n = len(guides) - 1
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("prune", 1)
    ix.upload(0)
    try:
        for call in range(2):
            assert _same(ix.score(guides[:n], 4, 75.0, "and"), _prefix(want, n))
            if call == 0:
                _first_batch_is_not_lean(ix)
        # the lane is lean and the last guide outgrows its hit slots: the batch is run again with the whole tail
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st = ix.stats()
        assert st["hits"] == per_guide.sum() and st["scan_launches"] >= 2
        for _ in range(3):      # (not lean, then lean again)
            assert _same(ix.score(guides[:n], 4, 75.0, "and"), _prefix(want, n))
            assert 0 < ix.get_option("ws_scan_verified") <= ix.stats()["raw_records"]
    finally:
        ix.close()


@pytest.fixture(scope="module")
def unit_forced(unit_case):
    path, guides, want, hits, _ = unit_case
    n = len(guides) - 1
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("prune", 1)
    ix.upload(0)
    assert _same(ix.score(guides[:n], 4, 75.0, "and"), _prefix(want, n))
    _first_batch_is_not_lean(ix)
    yield ix, guides[:n], _prefix(want, n), hits[hits[:, 0] < n]
    ix.close()


@pytest.mark.gpu
def test_dump_hits(unit_forced):
    ix, guides, _, hits = unit_forced
    got = ix.dump_hits(guides, 4, 0.0, "and")
    assert got.shape == hits.shape and np.array_equal(got, hits)
    assert ix.get_option("ws_scan_verified") > 0
    assert ix.get_option("ws_scan_lds_buffers") == 0   # (a dump has no hit slots: the batch is not lean)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 3])
def test_four_batches_in_flight(unit_forced, lanes):
    import torch
    ix, guides, want, _ = unit_forced
    ix.set_option("lanes", lanes)
    try:
        d_g = torch.from_numpy(guides.view(np.int64)).cuda()
        d_m = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]
        d_c = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]
        for _ in range(4):   # (a finish may ask for the batches again: a grown buffer)
            for m, c in zip(d_m, d_c):
                ix.score_device_async(d_g, m, c, 4, 75.0, "and")
            if ix.finish():
                break
        else:
            raise AssertionError("the batches were asked for a fifth time")
        for m, c in zip(d_m, d_c):
            assert _same((m.cpu().numpy(), c.cpu().numpy()), want)
        assert ix.get_option("ws_scan_verified") > 0
    finally:
        ix.set_option("lanes", 1)
