"""Which way the records of a lean batch went, where tests/test_scan_lds_records.py could not tell: the build of k_scan whose
waves note into two buffers of their LDS (k_scan<THR, true, true>) verifies a full buffer from LDS (scan_tail_lds) or copies
it to a chunk (lds_spill), and three read-only keys say which -- of lane 0's last finished batch ws_scan_lds_buffers
(Counters::lds_chunks: buffers verified from LDS), ws_scan_raw_top (Counters::raw_top: one past the last chunk a buffer
was copied to) and ws_raw_chunks (Counters::raw_chunks: chunks handed out, the waves' own included).

  C1  the shipped default: ISSL_SCAN_VERIFY unset, the tail armed by the batch's plan (PlanInfo::scan_tail), a lean batch --
      what the flagship's steady state runs.  test_scan_verify's cluster sites; 162 guides two or three substitutions from
      the cluster's centre in positions 8..11, 25 .. 277 hits each; one workgroup, 16 waves and one wave, both threshold
      builds, hit_slots 1 and 2, lanes 2 and 3 with four batches in flight, issl_dump_hits, lean_tail=0 on the same handle
  C2  the accounting of Counters::lds_chunks: one wave keeps every buffer of a batch in LDS and meets a guide beyond its hit
      slots; the batch is run again in full exactly ONCE, because sticky[1] = raw_chunks + lds_chunks made the host grow the
      record buffer first.  The buffer starts at the 16 chunks the counter starts from (one per wave of a workgroup,
      whatever scan_threads says): below that raw_chunks alone exceeds the capacity and the host grows the buffer whatever
      lds_chunks says; at 16 the lean launch asks for nothing beyond, and only lds_chunks can say that the repeat will
  C3  a lean batch outgrows the record buffer under the LDS build: lds_spill's raw_acquire<true> runs out of chunks (spare
      chunk, raw_overflow, no listing), the batch is run again in a grown buffer, and the lane is lean afterwards

Not covered: waves WITHOUT a chunk of their own under the LDS build (raw_chunks below the wave count on a lean lane).  Any
record such a wave notes overflows, the first overflow grows the buffer by at least 1 024 chunks, and a lane is lean only
after a clean batch: no sequence of calls keeps the lane lean and the buffer that small at once.

The constructions are checked on the CPU first (test_the_constructions_*: the oracle's hit counts, pruned_model's planned
comparisons, the header's constants)."""
import math
import re

import numpy as np
import pytest

import oracle_util as ou
import pruned_model as pm
from synth import random_sites
from test_scan_lds_records import _case, _sorted_unique, _sub, _unit_world
from test_scan_verify import ROOT, _cluster_world, _constant, _open, _same

LDS_KEYS = ("ws_scan_verified", "ws_scan_lds_buffers", "ws_scan_raw_top", "ws_raw_chunks", "ws_cap_chunks", "ws_lean")
RECS = 127   # records of a chunk or a buffer (kChunkRecs - 1; test_the_constructions_constants)


def _keys(ix):
    return {k: ix.get_option(k) for k in LDS_KEYS}


def _kernel_constant(name):
    """A constexpr uint32_t of issl_kernels.hip, as test_scan_verify._constant reads the header's."""
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)u?\s*;" % name, (ROOT / "crackling_amd" / "csrc" / "issl_kernels.hip").read_text())
    assert m, name
    return int(m.group(1))


def _scan_tail_cands():
    m = re.search(r"kScanTailCands\s*=\s*([0-9ul* ]+);", (ROOT / "crackling_amd" / "csrc" / "issl_device.hpp").read_text())
    assert m
    return math.prod(int(f.strip().rstrip("ul")) for f in m.group(1).split("*"))


def _prefix(want, k):
    return want[0][:k], want[1][:k]


def _singles(noise, rng, n):
    """n guides that are a noise site with one substitution in each of slices 0..3 (test_scan_lds_records._boundary_world's): such a
    guide meets its site in slice 4 alone -- one record."""
    out = []
    for s in noise[rng.permutation(len(noise))[:n]]:
        g = int(s)
        for p in (0, 4, 8, 12):
            g = _sub(g, p, int(rng.integers(1, 4)))
        out.append(g)
    return out


# ---- the constructions ----------------------------------------------------------------------------------------------------

def _lean_cluster_world():
    """test_scan_verify._cluster_world's sites, and the cluster's centre with two or three substitutions in positions 8..11
    (slice 2): 6 pairs of positions x 9 + 4 triples x 27 = 162 guides.  The cluster's sites differ from the centre in positions
    12..19 alone, so a guide has the centre, 24 sites at one and (two substitutions) 252 at two further mismatches within 4."""
    sites, big_guides = _cluster_world()
    centre = int(big_guides[0]) ^ (1 << 24)   # (its first guide: the centre with position 12 advanced by 1)
    pos = (8, 9, 10, 11)
    guides = [_sub(_sub(centre, p, d), q, e) for p in pos for q in pos if p < q for d in (1, 2, 3) for e in (1, 2, 3)]
    guides += [_sub(_sub(_sub(centre, p, d), q, e), r, f) for p in pos for q in pos for r in pos if p < q < r
               for d in (1, 2, 3) for e in (1, 2, 3) for f in (1, 2, 3)]
    assert len(set(guides)) == len(guides) == 162
    return sites, np.array(guides, dtype=np.uint64)


def _spread_world(seed=41, n_added=600):
    """Noise, eight single-record guides, and a guide G with n_added sites that are G with one substitution in each of slices
    0..3: within 4 of G, and found through slice 4's bucket alone.  The successor byte there is the site's slice 0, which has
    ONE substitution: 12 groups, n_added / 12 sites each.  -> sites, guides (G last), the added sites"""
    rng = np.random.default_rng(seed)
    noise, _ = random_sites(6000, seed=seed + 1)
    big = int(rng.integers(0, 1 << 40))
    added = set()
    for way in range(12):                       # slice 0: position way // 3 advanced by 1 + way % 3
        mine = set()
        while len(mine) < n_added // 12:
            s = _sub(big, way // 3, 1 + way % 3)
            for sl in (1, 2, 3):
                s = _sub(s, 4 * sl + int(rng.integers(0, 4)), int(rng.integers(1, 4)))
            mine.add(s)
        added |= mine
    added = np.array(sorted(added), dtype=np.uint64)
    assert len(added) == n_added
    sites = _sorted_unique(np.concatenate([noise, added]))
    guides = _singles(noise, rng, 8) + [big]
    assert len(set(guides)) == len(guides)
    return sites, np.array(guides, dtype=np.uint64), added


def _small_cluster_world(seed=51):
    """Noise, test_scan_lds_records._unit_world's small cluster (4^4 sites that differ in positions 12..15) with its 120 guides,
    and eight single-record guides in front of them."""
    _, guides, _ = _unit_world()
    centre = int(guides[0]) ^ (1 << 24)         # (its first guide: the centre with position 12 advanced by 1)
    cluster = [centre]
    for p in (12, 13, 14, 15):
        cluster = [(x & ~(3 << (2 * p))) | (b << (2 * p)) for x in cluster for b in range(4)]
    rng = np.random.default_rng(seed)
    noise, _ = random_sites(6000, seed=seed + 1)
    sites = _sorted_unique(np.concatenate([noise, np.array(cluster, dtype=np.uint64)]))
    all_guides = _singles(noise, rng, 8) + [int(g) for g in guides]
    assert len(set(all_guides)) == len(all_guides) == 128
    return sites, np.array(all_guides, dtype=np.uint64)


@pytest.fixture(scope="module")
def lean_cluster_case(tmp_path_factory):
    sites, guides = _lean_cluster_world()
    return _case(tmp_path_factory, "lean_cluster", sites, guides) + (sites,)


@pytest.fixture(scope="module")
def spread_case(tmp_path_factory):
    sites, guides, added = _spread_world()
    return _case(tmp_path_factory, "spread", sites, guides) + (added,)


@pytest.fixture(scope="module")
def small_cluster_case(tmp_path_factory):
    sites, guides = _small_cluster_world()
    return _case(tmp_path_factory, "small_cluster", sites, guides)


def test_the_constructions_constants():
    """What the file's arithmetic takes from the sources: 127 records per chunk, a wave's budget of 63 buffers, 512 hit slots."""
    assert _constant("kChunkRecs") - 1 == RECS
    assert _kernel_constant("kListChunks") == 64
    assert _constant("kSlotHits") == 512
    assert _scan_tail_cands() == 2 * 127 * 2048


def test_the_constructions_c1(lean_cluster_case):
    """C1 on the CPU: every guide stays within its hit slots (the lane is lean), the batch is too large for k_bin_small, and its
    plan arms the tail by itself for one workgroup of 16 waves -- kScanTailCands planned comparisons per wave."""
    _, guides, _, hits, per_guide, sites = lean_cluster_case
    print("hits per guide", per_guide.min(), "..", per_guide.max(), "in all", len(hits))
    assert len(guides) == 162 > pm.small_batch_limit(8, 4) == 102
    assert per_guide.min() == 25 and per_guide.max() == 277 <= _constant("kSlotHits")
    assert len(hits) == per_guide.sum() == 17659    # (54 x 277 + 108 x 25 of the cluster, one noise site)
    planned = pm.planned_comparisons(sites, guides, 4, 8)
    need = _scan_tail_cands() * 16
    print("planned comparisons", planned, "needed to arm the tail", need, "ratio %.2f" % (planned / need))
    assert planned == 10664586 and need == 8323072
    assert planned >= need


def test_the_constructions_c2(spread_case):
    """C2 on the CPU: the eight singles have one hit each, G between 513 and 1 024 (beyond its hit slots, within the wide
    ones), the batch's records take at least five buffers, and no (slice, slice value, successor byte) group holds more than a
    buffer's worth of the added sites -- no unit notes two buffers' worth, every buffer of the lean launch stays in LDS."""
    _, guides, _, hits, per_guide, added = spread_case
    assert len(guides) == 9 and np.all(per_guide[:8] == 1), per_guide[:8]
    print("hits of G", per_guide[8])
    assert 513 <= per_guide[8] <= 1024
    assert np.all(hits[hits[:, 0] == 8][:, 1] == 4)         # (found through slice 4 alone)
    assert math.ceil(len(hits) / RECS) >= 5
    codes = pm._codes(added)
    most = 0
    for s in range(5):
        value, succ = pm._slice_and_successor(codes, s, 8)
        most = max(most, int(np.bincount(value * 256 + succ).max()))
    print("largest group of added sites", most)
    assert most <= RECS
    value, succ = pm._slice_and_successor(codes, 4, 8)
    assert len(set(value.tolist())) == 1 and len(set(succ.tolist())) == 12    # one bucket of slice 4, 12 successor-byte groups


def test_the_constructions_c3(small_cluster_case):
    """C3 on the CPU: singles of one hit, cluster guides of 256 .. 512 (the lane stays lean), and more hits than the 63 buffers
    of a wave's budget hold: a single wave has to copy buffers to chunks."""
    _, guides, _, hits, per_guide = small_cluster_case
    assert len(guides) == 128 and np.all(per_guide[:8] == 1), per_guide[:8]
    print("hits per cluster guide", per_guide[8:].min(), "..", per_guide[8:].max(), "in all", len(hits))
    assert 256 <= per_guide[8:].min() and per_guide[8:].max() <= _constant("kSlotHits")
    assert per_guide[8:].sum() > (_kernel_constant("kListChunks") - 1) * RECS


# ---- C1: the default knob, a plan-armed tail, a lean batch ------------------------------------------------------------------

def _open_default(path, threads=1024, generic=0, slots=1):
    ix = _open(path, "auto")
    ix.set_option("prune", 1).set_option("scan_blocks", 1).set_option("scan_threads", threads)
    ix.set_option("scan_generic", generic).set_option("hit_slots", slots)
    ix.upload(0)
    return ix


def _first_default_batch(ix, guides, want):
    """The handle's first batch: by the index's mean group length no plan could arm a tail, so it runs the builds without one
    (test_scan_verify.cluster_auto); the batch is clean, so the lane is lean afterwards."""
    assert _same(ix.score(guides, 4, 75.0, "and"), want)
    keys = _keys(ix)
    print("first batch", keys, "scan_launches", ix.stats()["scan_launches"])
    assert keys["ws_scan_verified"] == 0 and keys["ws_scan_lds_buffers"] == 0 and keys["ws_scan_raw_top"] == 0
    assert keys["ws_lean"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("threads", [1024, 64])
def test_default_knob_plan_armed_tail_lean_batch(lean_cluster_case, threads, generic, slots):
    """Closes hole 2 (the shipped default never ran k_scan<THR, true, true> in a test) and, through the keys, hole 1: with the
    knob unset kTailLast is not set at first -- a wave's first full buffer sets it -- and a part-filled buffer at the end of the
    range goes to a chunk that k_verify finds through raw_top alone.  About 550 records fall into each of the cluster group's
    32 units, so both buffers of a wave fill inside a unit and buffers are copied to chunks: ws_scan_raw_top > 0 beside
    ws_scan_lds_buffers > 0 (seen on an MI355X: 16 waves verify ~22 100 records, 40 .. 43 buffers from LDS, raw_top 190 / 191;
    one wave 7 800 records -- its list's worth --, 16 buffers, raw_top 202).  Then issl_dump_hits (no hit slots: not lean) and lean_tail=0 on the same handle: no buffers."""
    path, guides, want, hits, per_guide, _ = lean_cluster_case
    ix = _open_default(path, threads, generic, slots)
    try:
        _first_default_batch(ix, guides, want)
        for call in (1, 2):
            got = ix.score(guides, 4, 75.0, "and")
            st, keys = ix.stats(), _keys(ix)
            print("threads", threads, "generic", generic, "slots", slots, "call", call, keys, "hits", st["hits"])
            assert _same(got, want)
            assert st["scan_launches"] == 1 and st["pruned"] == 2 and st["hits"] == per_guide.sum() == len(hits)
            assert keys["ws_lean"] == 1
            assert keys["ws_scan_verified"] > 0 and keys["ws_scan_lds_buffers"] > 0
            assert 0 < keys["ws_scan_raw_top"] <= keys["ws_raw_chunks"] <= keys["ws_cap_chunks"]
            if threads == 64:
                assert keys["ws_scan_lds_buffers"] <= _kernel_constant("kListChunks") - 1
        got = ix.dump_hits(guides, 4, 0.0, "and")
        assert got.shape == hits.shape and np.array_equal(got, hits)
        assert ix.get_option("ws_scan_lds_buffers") == 0 and ix.get_option("ws_scan_raw_top") == 0
        assert _same(ix.score(guides, 4, 75.0, "and"), want) and ix.get_option("ws_lean") == 1   # (the dump left the lane not lean)
        ix.set_option("lean_tail", 0)
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        keys = _keys(ix)
        assert keys["ws_scan_lds_buffers"] == 0 and keys["ws_scan_raw_top"] == 0 and keys["ws_scan_verified"] > 0
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 3])
def test_default_knob_four_batches_in_flight(lean_cluster_case, lanes):
    """Closes hole 2 for two workspaces: four batches in flight on lanes 2 and 3, the knob unset.  The first round may be asked
    for again (the second workspace's first record buffer is too small, and no lane is lean for a repeat); after a round that
    finished clean both lanes are lean, and the next four batches run the LDS build: finished at once, the first lane's last
    batch with buffers verified from LDS."""
    import torch
    path, guides, want, _, _, _ = lean_cluster_case
    ix = _open_default(path)
    try:
        _first_default_batch(ix, guides, want)
        ix.set_option("lanes", lanes)
        d_g = torch.from_numpy(guides.view(np.int64)).cuda()
        d_m = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]
        d_c = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]

        def four_batches():
            for m, c in zip(d_m, d_c):
                m.zero_()
                c.zero_()
                ix.score_device_async(d_g, m, c, 4, 75.0, "and")
            return ix.finish()

        def check():
            for m, c in zip(d_m, d_c):
                assert _same((m.cpu().numpy(), c.cpu().numpy()), want)

        for _ in range(4):
            if four_batches():
                break
        else:
            raise AssertionError("the batches were asked for a fifth time")
        check()
        print("lanes", lanes, "first round", _keys(ix))
        assert four_batches()
        check()
        keys = _keys(ix)
        print("lanes", lanes, "lean round", keys)
        assert keys["ws_lean"] == 1 and keys["ws_scan_verified"] > 0
        assert keys["ws_scan_lds_buffers"] > 0 and 0 < keys["ws_scan_raw_top"] <= keys["ws_raw_chunks"] <= keys["ws_cap_chunks"]
    finally:
        ix.close()


# ---- C2: the repeat in full finds its chunks ------------------------------------------------------------------------------

def _open_one_wave(path, raw_chunks, threads=64):
    ix = _open(path, "forced")
    ix.set_option("scan_blocks", 1).set_option("scan_threads", threads).set_option("prune", 1).set_option("raw_chunks", raw_chunks)
    ix.upload(0)
    return ix


def _clean_first_batch(ix, guides, want, raw_chunks):
    """Eight guides of one record each: the first batch is not lean, fits the wave's own chunk, and leaves the lane lean.
    -> ws_raw_chunks of a launch that hands out no chunk"""
    assert _same(ix.score(guides[:8], 4, 75.0, "and"), _prefix(want, 8))
    keys = _keys(ix)
    print("first batch", keys)
    assert ix.stats()["scan_launches"] == 1 and keys["ws_cap_chunks"] == raw_chunks and keys["ws_lean"] == 1
    assert keys["ws_scan_lds_buffers"] == 0 and keys["ws_scan_raw_top"] == 0 and keys["ws_scan_verified"] == 8
    return keys["ws_raw_chunks"]


@pytest.mark.gpu
def test_repeat_in_full_finds_its_chunks(spread_case):
    """Closes hole 3 (lds_chunks was asserted only as scan_launches >= 2): the lean launch keeps all its buffers in LDS and asks
    for no chunk, so sticky[1] exceeds the buffer's 16 chunks only by lds_chunks; without that the host would not grow the
    buffer, the repeat in full would overflow and the batch would take a THIRD launch -- with the right scores."""
    path, guides, want, hits, _, _ = spread_case
    ix = _open_one_wave(path, 16)
    try:
        _clean_first_batch(ix, guides, want, 16)
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st, keys = ix.stats(), _keys(ix)
        print("many-hit batch: scan_launches", st["scan_launches"], keys)
        assert st["scan_launches"] == 2
        assert st["hits"] == len(hits)
        assert keys["ws_cap_chunks"] >= math.ceil(len(hits) / RECS) and keys["ws_cap_chunks"] > 16
        assert keys["ws_scan_lds_buffers"] == 0     # (the repeat is not lean)
    finally:
        ix.close()


@pytest.mark.gpu
def test_repeat_in_full_finds_its_chunks_async(spread_case):
    """Closes holes 3 and 1: the same sequence through score_device_async; finish() says "again" exactly once, and between the
    two the keys are the LEAN launch's: at least five buffers verified from LDS, no buffer copied to a chunk, no chunk handed
    out -- so the grown buffer can only have come from lds_chunks."""
    import torch
    path, guides, want, hits, _, _ = spread_case
    ix = _open_one_wave(path, 16)
    try:
        quiet_chunks = _clean_first_batch(ix, guides, want, 16)
        d_g = torch.from_numpy(guides.view(np.int64)).cuda()
        d_m = torch.empty(len(guides), dtype=torch.float64, device="cuda")
        d_c = torch.empty_like(d_m)
        tries = 0
        for _ in range(4):
            ix.score_device_async(d_g, d_m, d_c, 4, 75.0, "and")
            tries += 1
            done = ix.finish()
            keys = _keys(ix)
            print("try", tries, "finished" if done else "again", keys)
            if done:
                break
            assert tries == 1
            assert keys["ws_scan_lds_buffers"] >= 5 and keys["ws_scan_raw_top"] == 0 and keys["ws_raw_chunks"] == quiet_chunks
            assert keys["ws_scan_verified"] >= len(hits)     # (one wave with a forced tail verifies every record it notes)
            assert keys["ws_cap_chunks"] >= quiet_chunks + keys["ws_scan_lds_buffers"] > 16
        assert tries == 2
        assert _same((d_m.cpu().numpy(), d_c.cpu().numpy()), want)
        assert keys["ws_scan_lds_buffers"] == 0 and keys["ws_cap_chunks"] >= math.ceil(len(hits) / RECS)
    finally:
        ix.close()


# ---- C3: a lean batch outgrows the record buffer ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_lean_batch_outgrows_the_record_buffer_one_wave(small_cluster_case):
    """Closes hole 4 (a lean batch never met a record buffer that is too small): one wave notes more than its budget of 63
    buffers, lds_spill's raw_acquire<true> finds no chunk in a buffer of four, the batch is run again in a grown buffer -- once --
    and the same batch is then lean, within the budget, with buffers in chunks that k_verify finds below raw_top."""
    path, guides, want, hits, _ = small_cluster_case
    budget = _kernel_constant("kListChunks") - 1
    ix = _open_one_wave(path, 4)
    try:
        _clean_first_batch(ix, guides, want, 4)
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st, keys = ix.stats(), _keys(ix)
        print("lean batch in a buffer of 4: scan_launches", st["scan_launches"], keys)
        assert st["scan_launches"] == 2 and st["hits"] == len(hits)
        assert keys["ws_cap_chunks"] > 4 and keys["ws_scan_lds_buffers"] == 0 and keys["ws_lean"] == 1
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st, keys = ix.stats(), _keys(ix)
        print("the same batch, lean: scan_launches", st["scan_launches"], keys)
        assert st["scan_launches"] == 1 and st["hits"] == len(hits)
        assert 1 <= keys["ws_scan_lds_buffers"] <= budget
        assert 0 < keys["ws_scan_raw_top"] <= keys["ws_raw_chunks"] <= keys["ws_cap_chunks"]
    finally:
        ix.close()


@pytest.mark.gpu
def test_lean_batch_outgrows_the_record_buffer_16_waves(small_cluster_case):
    """Closes hole 4 with 16 waves and 16 chunks: every wave has its own chunk and nothing beyond."""
    path, guides, want, hits, _ = small_cluster_case
    ix = _open_one_wave(path, 16, threads=1024)
    try:
        _clean_first_batch(ix, guides, want, 16)
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st, keys = ix.stats(), _keys(ix)
        print("lean batch, 16 waves in a buffer of 16: scan_launches", st["scan_launches"], keys)
        assert st["scan_launches"] <= 2 and st["hits"] == len(hits)
        if st["scan_launches"] == 1:
            assert keys["ws_scan_raw_top"] <= 16
        else:
            assert keys["ws_cap_chunks"] > 16
    finally:
        ix.close()
