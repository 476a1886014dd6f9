"""k_scan's verify tail: a scan wave applies the exact test to the records it noted itself (between two units and when
its range is done), marks the chunks it has been through, and k_verify takes what is left.  The knob is the environment
variable ISSL_SCAN_VERIFY, read when a handle is made: 0, the scan verifies nothing; unset, the tail runs in a batch whose
plan expects its waves to fill chunks (PlanInfo::scan_tail: kScanTailCands planned comparisons per wave), and there a wave
takes the chunks it has filled and, once it has filled one, its last one -- small batches lose time when the launch is
armed for a tail that has a handful of records per wave to verify --; 1, every batch and every wave's last chunk too: the
setting that brings the tail to the few records of a golden set.  The read-only key ws_scan_verified says how many records of the last batch
the scan's own waves verified.

  goldens    every golden scoring set, ISSL_SCAN_VERIFY unset, 1 and 0 (one child process per setting), lean_tail 0/1 x
             hit_slots 0/1/2: the reference's stdout, MIT / CFD as 64-bit patterns equal between the settings; with 1 the
             key is positive exactly where the tail can run (sorted layout, pruned plan), with 0 it is 0, unset it is at
             most what 1 gives
  one wave   scan_blocks=1, scan_threads=64: one wave notes more records than its list of reservations covers (sized from
             kScanVerifyRuns in the header): the rest is k_verify's, 0 < ws_scan_verified < hits
  exhausted  a raw-record buffer below what the batch needs: spare chunk, grow and re-run
  default    the unset knob on a batch whose plan arms the tail (a cluster of 65 536 sites, 110 guides, one workgroup): both
             builds of the kernel, lanes 2 and 3 with four batches in flight, issl_dump_hits
  edges      (ISSL_SCAN_VERIFY=1) batches of 1, 64 and 103 guides, max_dist 0..5, the runtime-threshold build, lanes 2 and 3 with four batches in
             flight, issl_dump_hits"""
import json
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
from synth import random_guides, random_sites, sigs_to_text, text_order_key

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
SETS = sorted(p.parent.name for p in (ROOT / "tests" / "golden").glob("*/guides.txt") if list(p.parent.glob("hits_*.tsv")))
COMBOS = [(lean, slots) for lean in (0, 1) for slots in (0, 1, 2)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---- goldens: one child process per environment --------------------------------------------------------------------

_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import crackling_amd as ca
from conftest import Golden
out = {}
for name in sys.argv[2].split(","):
    g = Golden(name)
    sigs = ca.encode_guides([s.encode() for s in g.guides])
    for lean in (0, 1):
        for slots in (0, 1, 2):
            ix = ca.IsslIndex.open(g.issl)
            ix.set_option("lean_tail", lean).set_option("hit_slots", slots).set_option("prune", 1)
            ix.upload(0)
            rows = {}
            for key, want in g.expected.items():
                method, thr, dist = key.split("|")
                mit, cfd = ix.score(sigs, int(dist), float(thr), method)
                st = ix.stats()
                rows[key] = [hashlib.sha256(mit.tobytes() + cfd.tobytes()).hexdigest(), ca.format_scores(sigs, mit, cfd, method) == want,
                             ix.get_option("ws_scan_verified"), st["pruned"], st["hits"], ix.get_option("is_sorted")]
            out["%s|%d|%d" % (name, lean, slots)] = rows
            ix.close()
# where the tail must not run: whole buckets, a list-order layout
g = Golden("uniform")
sigs = ca.encode_guides([s.encode() for s in g.guides])
for label, option in (("prune0", ("prune", 0)), ("list_order", ("sorted_layout", 0))):
    ix = ca.IsslIndex.open(g.issl)
    ix.set_option(*option)
    ix.upload(0)
    mit, cfd = ix.score(sigs, 4, 75.0, "and")
    out[label] = [ca.format_scores(sigs, mit, cfd, "and") == g.expected["and|75|4"], ix.get_option("ws_scan_verified"), ix.stats()["hits"]]
    ix.close()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def golden_runs():
    """{"auto": ..., "on": ..., "off": ...}: the child's report with ISSL_SCAN_VERIFY unset, 1 and 0."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("ISSL_")}
    runs = {}
    for label, extra in (("auto", {}), ("on", {"ISSL_SCAN_VERIFY": "1"}), ("off", {"ISSL_SCAN_VERIFY": "0"})):
        run = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), ",".join(SETS)], env={**base, **extra}, capture_output=True,
                             text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        runs[label] = json.loads(run.stdout.strip().splitlines()[-1])
    return runs


def test_the_sets_are_all_there():
    assert "signedtable" in SETS and len(SETS) >= 9


@pytest.mark.parametrize("name", SETS)
def test_goldens_with_and_without_the_tail(golden_runs, name):
    auto, on, off = golden_runs["auto"], golden_runs["on"], golden_runs["off"]
    ran = 0
    for lean, slots in COMBOS:
        a, b, c = on["%s|%d|%d" % (name, lean, slots)], off["%s|%d|%d" % (name, lean, slots)], auto["%s|%d|%d" % (name, lean, slots)]
        assert a.keys() == b.keys() == c.keys() and a
        for key in a:
            where = (name, lean, slots, key)
            bits_on, text_on, verified_on, pruned_on, hits_on, sorted_on = a[key]
            bits_off, text_off, verified_off, pruned_off, hits_off, _ = b[key]
            bits_auto, text_auto, verified_auto, pruned_auto, hits_auto, _ = c[key]
            assert text_on and text_off and text_auto, where   # the reference's stdout
            assert bits_on == bits_off == bits_auto, where     # MIT and CFD bit for bit, tail or none
            assert (pruned_on, hits_on) == (pruned_off, hits_off) == (pruned_auto, hits_auto), where
            assert verified_off == 0, where
            assert 0 <= verified_auto <= verified_on, where
            assert sorted_on == (0 if name == "mixedocc" else 1), where   # (counts that differ between a site's lists: list order)
            assert not pruned_on or sorted_on, where
            if pruned_on and hits_on:                    # (a hit is a record that survived: the batch noted some)
                assert verified_on > 0, where
                ran += 1
            if not pruned_on:                            # (max_dist 6, a list-order layout: whole buckets)
                assert verified_on == 0, where
    assert ran or name == "mixedocc", name


def test_no_tail_without_the_pruned_plan_or_the_sorted_layout(golden_runs):
    for label in ("prune0", "list_order"):
        for run in ("auto", "on", "off"):
            text_ok, verified, hits = golden_runs[run][label]
            assert text_ok and hits > 0 and verified == 0, (label, run)


# ---- one wave, many chunks ------------------------------------------------------------------------------------------

def _open(path, mode):
    """A handle made with ISSL_SCAN_VERIFY unset ("auto") or 1 ("forced"): the variable is read when the handle is made."""
    old = os.environ.pop("ISSL_SCAN_VERIFY", None)
    try:
        if mode == "forced":
            os.environ["ISSL_SCAN_VERIFY"] = "1"
        return ca.IsslIndex.open(path)
    finally:
        os.environ.pop("ISSL_SCAN_VERIFY", None)
        if old is not None:
            os.environ["ISSL_SCAN_VERIFY"] = old


def _constant(name):
    header = (ROOT / "crackling_amd" / "csrc" / "issl_device.hpp").read_text()
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)" % name, header)
    assert m, name
    return int(m.group(1))


def _listed_records():
    """Records the chunks of a full list hold: the wave's own chunk and its reservations of 1, 2, 4, 8, 16, 16 ... chunks."""
    runs, recs = _constant("kScanVerifyRuns"), _constant("kChunkRecs")
    chunks = 1 + sum(min(1 << (k - 1), 16) for k in range(1, runs))
    return chunks * (recs - 1)


def _cluster_world(n_guides=110, seed=5):
    """A site list with a cluster of 4^8 sites that differ in positions 12..19 only (slices 3 and 4 of five), among random
    ones, and guides one or two substitutions away from the cluster's centre in those positions.  In the buckets of slices
    0 and 1 the whole cluster is ONE successor-byte group, so a guide plans ~135 000 comparisons and has 7 459 - a few
    sites within 4 mismatches: a batch of more than 102 guides (no k_bin_small) that plans kScanTailCands comparisons per
    wave of one 16-wave workgroup -- the plan arms the tail by itself -- and whose waves fill hundreds of chunks."""
    rng = np.random.default_rng(seed)
    centre = int(rng.integers(0, 1 << 40))
    positions = list(range(12, 20))
    cluster = [centre]
    for p in positions:
        cluster = [(x & ~(3 << (2 * p))) | (b << (2 * p)) for x in cluster for b in range(4)]
    noise, _ = random_sites(20000, seed=seed + 1)
    sites = np.unique(np.concatenate([np.array(cluster, dtype=np.uint64), noise]))
    sites = sites[np.argsort(text_order_key(sites), kind="stable")]
    guides = [centre ^ (d << (2 * p)) for p in positions for d in (1, 2, 3)]
    guides += [centre ^ (d << (2 * p)) ^ (e << (2 * q)) for p in positions for q in positions if p < q for d in (1, 2, 3) for e in (1, 2)]
    guides = guides[:n_guides]
    assert len(set(guides)) == len(guides) == n_guides > 102
    return sites, np.array(guides, dtype=np.uint64)


@pytest.fixture(scope="module")
def cluster_case(tmp_path_factory):
    listed = _listed_records()
    sites, guides = _cluster_world()
    path = tmp_path_factory.mktemp("scan_verify") / "cluster.issl"
    ix = ca.IsslIndex.build_from_text(sigs_to_text(sites))
    ix.write(path)
    ix.close()
    oracle = ou.OracleIndex(path)
    want = oracle.score(guides, 4, 75.0, "and")
    hits = oracle.score(guides, 4, 0.0, "and", want_hits=True)[2]
    oracle.close()
    return path, guides, want, listed, hits


def test_the_cluster_batch_arms_the_tail_by_its_plan(cluster_case):
    """What k_fine_plan will see, from the header's constants: the planned comparisons of the batch against one workgroup's
    16 waves."""
    path, guides, _, _, _ = cluster_case
    m = re.search(r"kScanTailCands\s*=\s*2ull \* 127ull \* 2048ull", (ROOT / "crackling_amd" / "csrc" / "issl_device.hpp").read_text())
    assert m
    assert len(guides) * 2 * 65536 >= 2 * 127 * 2048 * 16     # (the cluster alone, in the buckets of slices 0 and 1)


@pytest.mark.parametrize("mode", ["auto", "forced"])
def test_one_wave_outgrows_its_list(cluster_case, mode):
    path, guides, want, listed, _ = cluster_case
    ix = _open(path, mode)
    ix.set_option("scan_blocks", 1).set_option("scan_threads", 64).set_option("prune", 1)
    ix.upload(0)
    try:
        # (the second call: the lane has learnt that its guides outgrow their hit slots -- and, with the knob unset, the handle
        # what a guide of this index plans: the host takes the builds with a tail for a batch only when the index's mean group
        # length or the handle's last finished plan says that the batch's plan can arm one)
        for call in range(2):
            got = ix.score(guides, 4, 75.0, "and")
            st = ix.stats()
            verified = ix.get_option("ws_scan_verified")
            print("hits", st["hits"], "listed records", listed, "ws_scan_verified", verified)
            assert _same(got, want)
            assert st["pruned"] == 2 and st["hits"] > 2 * listed
            assert verified <= listed < st["hits"]
            assert verified > 0 or (mode == "auto" and call == 0)
    finally:
        ix.close()


# ---- exhausted buffer -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["auto", "forced"])
@pytest.mark.parametrize("raw_chunks", [4, 24, 200])
def test_exhausted_record_buffer(cluster_case, raw_chunks, mode):
    """Fewer chunks than scan waves (the waves beyond start in the spare chunk), than the batch's records need: issl_score
    grows the buffer and runs the batch again."""
    path, guides, want, _, _ = cluster_case
    ix = _open(path, mode)
    ix.set_option("raw_chunks", raw_chunks).set_option("prune", 1).set_option("scan_blocks", 1)
    ix.upload(0)
    try:
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        assert ix.get_option("ws_cap_chunks") > raw_chunks
        if mode == "auto":   # (the handle has now finished a batch of this index: the next one gets the builds with a tail)
            assert _same(ix.score(guides, 4, 75.0, "and"), want)
        assert ix.get_option("ws_scan_verified") > 0
    finally:
        ix.close()


# ---- the shipped default where waves fill chunks -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def cluster_auto(cluster_case):
    path, guides, want, _, hits = cluster_case
    ix = _open(path, "auto")
    ix.set_option("prune", 1).set_option("scan_blocks", 1)
    ix.upload(0)
    # the handle's first batch: by the index's mean group length (85 000 sites) no plan could arm a tail, so it runs the
    # builds without one; from its plan the handle learns what a guide of this index plans
    assert _same(ix.score(guides, 4, 75.0, "and"), want) and ix.get_option("ws_scan_verified") == 0
    yield ix, guides, want, hits
    ix.close()


@pytest.mark.parametrize("generic", [0, 1])
def test_default_setting_on_a_batch_that_fills_chunks(cluster_auto, generic):
    ix, guides, want, _ = cluster_auto
    listed = _listed_records()
    ix.set_option("scan_generic", generic)
    try:
        assert _same(ix.score(guides, 4, 75.0, "and"), want)
        st = ix.stats()
        verified = ix.get_option("ws_scan_verified")
        print("hits", st["hits"], "raw records", st["raw_records"], "ws_scan_verified", verified)
        # 16 waves share the units through tickets and note ~50 000 records each, six times what a list covers: no wave
        # verifies more than its list holds, and a retired chunk is at least half full (a pass notes at most 64 records), so
        # half of the waves filling their lists already give 8 x listed / 2
        assert st["pruned"] == 2 and st["hits"] > 16 * listed
        assert 8 * listed // 2 < verified <= 16 * listed
    finally:
        ix.set_option("scan_generic", 0)


@pytest.mark.parametrize("lanes", [2, 3])
def test_default_setting_four_batches_in_flight(cluster_auto, lanes):
    import torch
    ix, guides, want, _ = cluster_auto
    ix.set_option("lanes", lanes)
    try:
        d_g = torch.from_numpy(guides.view(np.int64)).cuda()
        d_m = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]
        d_c = [torch.empty(len(guides), dtype=torch.float64, device="cuda") for _ in range(4)]
        for _ in range(4):   # (a finish may ask for the batches again: a lean lane that met a guide beyond its slots, a grown buffer)
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


def test_default_setting_dump_hits(cluster_auto):
    ix, guides, _, hits = cluster_auto
    got = ix.dump_hits(guides, 4, 0.0, "and")
    assert got.shape == hits.shape and np.array_equal(got, hits)
    assert ix.get_option("ws_scan_verified") > 0


# ---- edges of the gate ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    sites, occ = random_sites(60000, seed=11)
    guides = random_guides(sites, 103, seed=12)
    path = tmp_path_factory.mktemp("scan_verify") / "random.issl"
    ix = ca.IsslIndex.build_from_text(sigs_to_text(sites, occ))
    ix.write(path)
    ix.close()
    oracle = ou.OracleIndex(path)
    want = {d: oracle.score(guides, d, 75.0, "and") for d in range(6)}
    hits = oracle.score(guides, 4, 0.0, "and", want_hits=True)[2]
    oracle.close()
    ix = _open(path, "forced")   # (a few records per wave: the tail's last chunk has to be asked for)
    ix.set_option("prune", 1)
    ix.upload(0)
    yield ix, guides, want, hits
    ix.close()


@pytest.mark.parametrize("n", [1, 64, 103])
def test_small_batches(random_case, n):
    """1 and 64 guides are binned by k_bin_small; all three leave scan workgroups without a range."""
    ix, guides, want, _ = random_case
    got = ix.score(guides[:n], 4, 75.0, "and")
    assert _same(got, (want[4][0][:n], want[4][1][:n]))
    st = ix.stats()
    assert st["pruned"] == 2
    assert (ix.get_option("ws_scan_verified") > 0) == (st["hits"] > 0)


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("max_dist", range(6))
def test_every_distance_and_the_runtime_threshold_build(random_case, max_dist, generic):
    ix, guides, want, _ = random_case
    ix.set_option("scan_generic", generic)
    try:
        assert _same(ix.score(guides, max_dist, 75.0, "and"), want[max_dist])
        st = ix.stats()
        assert st["pruned"] == (1 if max_dist <= 2 else 3 if max_dist == 5 else 2)
        assert (ix.get_option("ws_scan_verified") > 0) == (st["hits"] > 0)
    finally:
        ix.set_option("scan_generic", 0)


@pytest.mark.parametrize("lanes", [2, 3])
def test_four_batches_in_flight(random_case, lanes):
    import torch
    ix, guides, want, _ = random_case
    ix.set_option("lanes", lanes)
    try:
        parts = [guides[:40], guides[40:64], guides[64:], guides]
        d_g = [torch.from_numpy(p.view(np.int64)).cuda() for p in parts]
        d_m = [torch.empty(len(p), dtype=torch.float64, device="cuda") for p in parts]
        d_c = [torch.empty(len(p), dtype=torch.float64, device="cuda") for p in parts]
        for _ in range(3):   # (a finish may ask for the batches again: a lean lane that met a guide beyond its slots, a grown buffer)
            for g, m, c in zip(d_g, d_m, d_c):
                ix.score_device_async(g, m, c, 4, 75.0, "and")
            if ix.finish():
                break
        else:
            raise AssertionError("the batches were asked for a fourth time")
        got_mit = torch.cat(d_m[:3]).cpu().numpy(), d_m[3].cpu().numpy()
        got_cfd = torch.cat(d_c[:3]).cpu().numpy(), d_c[3].cpu().numpy()
        for k in range(2):
            assert _same((got_mit[k], got_cfd[k]), want[4])
        assert ix.get_option("ws_scan_verified") > 0
    finally:
        ix.set_option("lanes", 1)


def test_dump_hits(random_case):
    """issl_dump_hits runs without hit slots: every hit of a chunk the scan verified is grouped from the keys, ranks and
    terms its wave left."""
    ix, guides, _, hits = random_case
    got = ix.dump_hits(guides, 4, 0.0, "and")
    assert got.shape == hits.shape and np.array_equal(got, hits)
    assert ix.get_option("ws_scan_verified") > 0
