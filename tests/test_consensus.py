"""GPU: crackling_amd.Consensus / issl_consensus_* against the reference's own rows (tests/golden/consensus) and, bit for
bit, against the numpy model of tests/consensus_util.py, which tests/test_consensus_model.py pins to those rows."""
import ctypes as C
import itertools

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import consensus_util as cu

pytestmark = pytest.mark.gpu
CONFIGS = cu.golden_configs()
WORKGROUP = 256  # kThreads of issl_consensus.hip: guides per workgroup of every kernel
COUNTS = [0, 1, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 5003]
ENERGIES = [-35.0, -30.0, -29.9, -18.0, -17.9, -10.0, -5.3]


# ---- inputs -----------------------------------------------------------------------------------------------------------

def synthetic_set(n, seed):
    """A FASTA whose guide set is exactly n known guides in a known order: one record of 23 characters per occurrence,
    [AGT][ACGT]{20}GG -- one window, the forward pattern only -- and every seventh guide a second time at the end.
    -> (blob, guides, seen)"""
    rng = np.random.default_rng(seed)
    guides, have = [], set()
    while len(guides) < n:
        g = "AGT"[rng.integers(3)] + "".join("ACGT"[c] for c in rng.integers(0, 4, 20)) + "GG"
        if g not in have:
            have.add(g)
            guides.append(g)
    again = guides[::7]
    blob = "".join(f">r{i}\n{g}\n" for i, g in enumerate(guides + again)).encode() or b">none\nATATAT\n"
    seen = [2 if i % 7 == 0 else 1 for i in range(n)]
    return blob, guides, seen


_sets = {}


def guide_set(n, seed=1):
    """The set of synthetic_set(n, seed), extracted once and kept for the module."""
    if (n, seed) not in _sets:
        blob, guides, seen = synthetic_set(n, seed)
        gs = ca.GuideSet.extract([blob])
        assert gs.strings() == guides and gs.guides["seen"].tolist() == seen
        _sets[(n, seed)] = (gs, guides, seen)
    return _sets[(n, seed)]


def synthetic_model(n_sv, seed):
    """Random 0/1 rows -- nothing makes them one-hot per position -- and coefficients of both signs from 1e-3 to 1e3: a
    sum in another order, or a fused multiply-add, rounds differently."""
    rng = np.random.default_rng(seed)
    sv = rng.integers(0, 2, (n_sv, 80)).astype(np.uint8)
    coef = rng.choice([-1.0, 1.0], n_sv) * 10.0 ** rng.uniform(-3, 3, n_sv)
    return sv, coef, float(rng.normal())


def synthetic_folds(n, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros(n, dtype=ca.FOLD_DTYPE)
    f["energy"] = rng.choice(ENERGIES, n)
    f["scaffold"] = rng.integers(0, 2, n)
    f["present"] = rng.random(n) < 0.9
    return f


def same_rows(got, want):
    """Bit for bit: the three doubles as 64-bit words (NaN where the model has NaN), the eight codes as bytes."""
    assert got.dtype == ca.CONSENSUS_DTYPE and len(got) == len(want)
    for f in ("sgrna_score", "at", "ss_energy"):
        nan = np.isnan(want[f])
        assert np.array_equal(np.isnan(got[f]), nan), f
        assert np.array_equal(got[f][~nan].view(np.uint64), want[f][~nan].view(np.uint64)), f
    for f in cu.CODE_FIELDS + ("count",):
        assert np.array_equal(got[f], want[f]), f


def run_both(gs, guides, seen, kw, fold_seed=5):
    """Consensus on the device and the model with the same folds; compares everything.  -> the finished Consensus"""
    m = cu.Model(guides, seen, **kw)
    c = gs.consensus(kw)
    assert c.n_fold == len(m.fold_rows) and np.array_equal(c.fold_rows, m.fold_rows)
    folds = synthetic_folds(c.n_fold, fold_seed)
    m.finish(folds)
    c.finish(folds)
    same_rows(c.rows, m.rows)
    assert c.n_selected == len(m.selected) and np.array_equal(c.selected, m.selected)
    assert c.selected.dtype == np.uint32 and c.fold_rows.dtype == np.uint32
    return c


# ---- the reference's own rows -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_set():
    gs = ca.GuideSet.extract([(cu.GOLDEN / "guides.fa").read_bytes()])
    yield gs
    gs.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c["name"] for c in CONFIGS])
def test_golden_parity(cfg, golden_set):
    gs = golden_set
    want = cu.golden_rows(cfg["name"])
    guides, seen = gs.strings(), gs.guides["seen"].tolist()
    kw = cu.golden_keywords(cfg)
    with gs.consensus(kw) as c:
        folded = [j for j, w in enumerate(want) if w["ssEnergy"] != "?"]  # the reference fills ssEnergy for every line it folded
        assert c.fold_rows.tolist() == folded
        assert c.fold_input() == "".join("G" + guides[j][1:20] + ca.SCAFFOLD + "\n" for j in folded)
        if cfg["name"] == "ultralow":
            assert c.fold_input() == "".join(cu.fold_text().splitlines(True)[0::2])
        assert c.fold_guides() == [guides[j] for j in c.fold_rows]
        text = cu.fold_text()
        folds = ca.read_rnafold_output(text, c.fold_guides())
        c.finish(folds if cfg["mm10db"] else None)
        cu.compare_with_reference(c.rows, guides, seen, want, cu.fold_energies(text))
        m = cu.Model(guides, seen, **kw).finish(ca.read_rnafold_output(text, [guides[j] for j in c.fold_rows]))
        same_rows(c.rows, m.rows)  # the scores: the same bits as the model's, whose digits are the reference's
        assert np.array_equal(c.selected, m.selected) and c.selected_tensor().dtype.is_floating_point is False


# ---- synthetic models, bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_sv", [1, 215, 257])
@pytest.mark.parametrize("n", COUNTS)
def test_synthetic_models(n, n_sv):
    gs, guides, seen = guide_set(n)
    model = synthetic_model(n_sv, seed=n_sv)
    level = ("ultralow", "low", "medium", "high")[(n + n_sv) % 4]
    with run_both(gs, guides, seen, dict(optimisation=level, n=2, model=model, sgrna_threshold=0.5)) as c:
        if level == "ultralow":  # every guide is scored
            assert not np.isnan(c.rows["sgrna_score"]).any() and c.n_selected == n
    # sgRNAScorer2 alone at ultralow: one score per guide whatever the other tools say
    with run_both(gs, guides, seen, dict(optimisation=0, n=1, mm10db=False, chopchop=False, model=model)) as c:
        want = cu.sgrna_scores(guides, *model)
        assert np.array_equal(c.rows["sgrna_score"].view(np.uint64), want.view(np.uint64))
        assert c.n_fold == 0


def test_fused_or_reordered_sums_would_show():
    """The coefficients of synthetic_model do what they are there for: on these guides the sum in reverse order differs
    from the specified one in some bits (so a kernel that reordered it could not pass test_synthetic_models)."""
    _, guides, _ = guide_set(257)
    sv, coef, b = synthetic_model(215, seed=215)
    a = cu.sgrna_scores(guides, sv, coef, b)
    r = cu.sgrna_scores(guides, sv[::-1], coef[::-1], b)
    assert (a.view(np.uint64) != r.view(np.uint64)).any()


# ---- every configuration ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", ["ultralow", "low", "medium", "high"])
def test_configurations(level):
    gs, guides, seen = guide_set(301, seed=3)
    model = synthetic_model(33, seed=9)
    for (mm, ch, sg), n in itertools.product(itertools.product([False, True], repeat=3), range(4)):
        kw = dict(optimisation=level, n=n, mm10db=mm, chopchop=ch, sgrnascorer2=sg, model=model, sgrna_threshold=-1.0)
        with run_both(gs, guides, seen, kw, fold_seed=n) as c:
            if not mm:
                assert c.n_fold == 0 and (c.rows["mm10db"] == cu.UNTESTED).all()


# ---- scoring with a selection -----------------------------------------------------------------------------------------

def test_score_with_a_selection(golden_set):
    gs = golden_set
    blob = (cu.GOLDEN / "guides.fa").read_bytes()
    cfg = next(c for c in CONFIGS if c["name"] == "high")
    with ca.IsslIndex.build_from_fasta([blob]) as index, gs.consensus(cu.golden_keywords(cfg)) as c:
        c.finish(ca.read_rnafold_output(cu.fold_text(), c.fold_guides()))
        assert 0 < c.n_selected < gs.n_unique
        idx, mit, cfd = gs.score(index, consensus=c)
        assert np.array_equal(idx, c.selected)
        all_idx, all_mit, all_cfd = gs.score(index, only_unique=False)
        assert np.array_equal(all_idx, np.arange(len(gs)))
        assert np.array_equal(mit.view(np.uint64), all_mit[idx].view(np.uint64))
        assert np.array_equal(cfd.view(np.uint64), all_cfd[idx].view(np.uint64))
        uniq_idx, _, _ = gs.score(index)  # without the keyword: the rows seen once, as before
        assert np.array_equal(uniq_idx, np.flatnonzero(gs.guides["seen"] == 1))
        other, _, _ = guide_set(64)
        with pytest.raises(ValueError):
            other.score(index, consensus=c)


# ---- states and errors ------------------------------------------------------------------------------------------------

def test_states_and_errors():
    gs, guides, seen = guide_set(65)
    model = synthetic_model(3, seed=1)
    lib = _lib.lib
    with gs.consensus(optimisation="low", model=model) as c:
        assert c.n_fold > 0
        rows = np.empty(len(gs), dtype=ca.CONSENSUS_DTYPE)
        p, q, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert lib.issl_consensus_copy(c._h, rows.ctypes.data, len(rows)) == -7      # ahead of finish
        assert lib.issl_consensus_device(c._h, C.byref(p), C.byref(q), C.byref(n)) == -7
        folds = synthetic_folds(c.n_fold, 1)
        assert lib.issl_consensus_finish(c._h, folds.ctypes.data, c.n_fold - 1) == -1  # not the fold list's length
        assert lib.issl_consensus_finish(c._h, folds.ctypes.data, c.n_fold + 1) == -1
        assert lib.issl_consensus_finish(c._h, None, c.n_fold) == -1
        assert lib.issl_consensus_fold_copy(c._h, rows.ctypes.data, c.n_fold - 1) == -1
        with pytest.raises(ca.IsslError) as e:
            c.finish(None)
        assert e.value.code == -1
        c.finish(folds)
        with pytest.raises(ca.IsslError) as e:
            c.finish(folds)
        assert e.value.code == -7                                                       # a second time
        assert lib.issl_consensus_copy(c._h, rows.ctypes.data, len(rows) - 1) == -1
        assert lib.issl_consensus_copy(c._h, None, len(rows)) == -1
        same_rows(c.rows, cu.Model(guides, seen, optimisation="low", model=model).finish(folds).rows)
    h = C.c_void_p()
    cfg = _lib.ConsensusConfig(optimisation=4)
    assert lib.issl_consensus_begin(gs._h, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    cfg = _lib.ConsensusConfig(optimisation=3, sgrnascorer2=1, n_sv=0)
    assert lib.issl_consensus_begin(gs._h, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    cfg = _lib.ConsensusConfig(optimisation=3, sgrnascorer2=1, n_sv=2)                 # no arrays
    assert lib.issl_consensus_begin(gs._h, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    sv, coef, b = model
    with pytest.raises(ca.IsslError) as e:
        gs.consensus(model=(sv * 2, coef, b))
    assert e.value.code == -4                                                           # an entry other than 0 / 1
    with gs.consensus(mm10db=False, model=model) as c:                                 # nothing to fold
        assert c.n_fold == 0 and len(c.fold_rows) == 0 and c.fold_input() == ""
        assert lib.issl_consensus_finish(c._h, None, 0) == 0
        assert lib.issl_consensus_finish(c._h, None, 0) == -7


def test_empty_set():
    gs, guides, seen = guide_set(0)
    assert len(gs) == 0
    with gs.consensus(model=synthetic_model(5, seed=2)) as c:
        assert c.n_fold == 0 and len(c.fold_rows) == 0
        c.finish(None)
        assert len(c.rows) == 0 and c.n_selected == 0 and c.selected_tensor().numel() == 0


def test_two_runs_give_the_same_bytes():
    gs, guides, seen = guide_set(5003)
    model = synthetic_model(215, seed=4)
    out = []
    for _ in range(2):
        with gs.consensus(optimisation="medium", model=model) as c:
            folds = synthetic_folds(c.n_fold, 8)
            c.finish(folds)
            out.append((c.fold_rows.tobytes(), c.rows.tobytes(), c.selected.tobytes()))
    assert out[0] == out[1]
