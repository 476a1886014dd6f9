"""GPU: the figures of the run's log made on the device (crackling_amd.BatchCounts / issl_runlog_batches, the Bowtie step's
events per page, the log a pipeline run feeds) against the host model of tests/runlog_model.py, which
tests/test_runlog_model.py pins to the reference's own logs (tests/golden/runlog).

The counting kernels take three paths -- a workgroup of 2048 rows inside one batch sums in LDS, a wave inside one batch adds
its ballot, a wave across batches adds lane by lane -- so the sizes are placed around them: batches of 1, 17, 64, 255, 256,
257, around 2048 and 4096, one batch, a batch above the set, on a set of about 300 rows (one workgroup, not full) and one of
several thousand (several workgroups, the last not full)."""
import ctypes as C

import numpy as np
import pytest

import crackling_amd as ca
import batches_util as bt
import bowtie_util as bu
import consensus_util as cu
import results_util as ru
import runlog_model as rm
import runlog_util as rl

pytestmark = pytest.mark.gpu
RUNS = rl.golden_runs()
IDS = [r["name"] for r in RUNS]
_models = {}


def model_of(run):
    key = (run["base"], run["batch_size"], run["rnafold_page_length"], run["rnafold_answers"])
    if key not in _models:
        _models[key] = rm.Run(run, rl.golden_fold_text(run))
    m = _models[key]
    m.run = run
    return m


@pytest.fixture(scope="module")
def golden():
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    index = ca.IsslIndex.open(bu.GOLDEN / "index.issl").upload(0)
    yield genome, index
    index.close()
    genome.close()


def same_counts(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in rm.FIELDS:
        bad = np.flatnonzero(np.asarray(got[f]) != np.asarray(want[f]))
        assert len(bad) == 0, (what, f, bad[:5].tolist(), np.asarray(got[f])[bad[:5]].tolist(), np.asarray(want[f])[bad[:5]].tolist())


class Spy(ca.RunLog):
    """A RunLog that keeps what the stages feed it."""

    def __init__(self, config):
        super().__init__(config)
        self.fed = []

    def batch(self, index, n_batches, counts, page_failed=(), not_found=(), bowtie_failed=0, seconds=0.0):
        self.fed.append((index, n_batches, np.array(counts), [int(x) for x in page_failed], list(not_found), int(bowtie_failed)))
        super().batch(index, n_batches, counts, page_failed, not_found, bowtie_failed, seconds)


# ---- 1. the reference's own logs, through the pipeline ------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_golden_log_and_counts_through_the_pipeline(golden, run, monkeypatch):
    genome, index = golden
    if run.get("genome"):
        genome = ca.Genome.open([rl.golden_genome(run)])
    whole = rl.golden_fold_text(run)
    monkeypatch.chdir(rl.golden_source(run))  # (the log names the input as it was configured: the golden keeps the file's name)
    kw = rl.golden_keywords(run)
    log = Spy(kw)
    got = ca.pipeline.run([run["input"]], genome, index, kw, lambda text: bt.answer_page(whole, text), log=log)
    assert got == rl.golden_bytes(run)
    assert got == ca.pipeline.run([run["input"]], genome, index, kw, lambda text: bt.answer_page(whole, text))
    rl.same_log(log.text(), rl.golden_log(run["name"]))
    m = model_of(run)
    batches, page_failed, not_found = m.counts()
    events = m.batch_events(batches)
    assert [f[0] for f in log.fed] == list(range(len(batches))) and all(f[1] == len(batches) for f in log.fed)
    same_counts(np.array([f[2] for f in log.fed], dtype=rm.DTYPE) if log.fed else np.zeros(0, dtype=rm.DTYPE), batches, run["name"])
    assert [x for f in log.fed for x in f[3]] == page_failed.tolist()
    if run["rnafold_page_length"] == 0:  # every row is not found and the log prints none of them: none is gathered
        assert len(not_found) == len(m.fold_rows) > 0 and not any(f[4] for f in log.fed)
    else:
        assert [p for f in log.fed for p, _ in f[4]] == not_found.tolist()
        assert [g for f in log.fed for _, g in f[4]] == [m.seqs[int(m.fold_rows[p])][:20] for p in not_found]
    assert [f[5] for f in log.fed] == events
    if run.get("genome"):
        genome.close()


# ---- 2. seeded inputs around the edges of waves and workgroups -----------------------------------------------------------

def seeded_stages(n_guides, seed):
    """GuideSet, finished Consensus with Folds (every seventh answer left out), BowtieStep on a genome that is the input and
    its first third once more (the guides of that third are rejected), and scores of its own making for every second
    selected row -> the objects and the same arrays on the host."""
    import torch
    rng = np.random.default_rng(seed)
    if n_guides <= 400:
        blob = ru.crafted_fasta(n_guides, seed)
    else:
        blob = (">big\n" + "".join(rng.choice(list("ACGT"), 12 * n_guides)) + "\n").encode()
    genome = ca.Genome.open([blob + blob[:blob.rindex(b"\n>", 0, len(blob) // 3) + 1]] if n_guides <= 400 else
                            [blob + b">again\n" + blob[5:4 * n_guides] + b"\n"])
    gs = ca.GuideSet.extract([blob])
    c = ca.Consensus(gs, optimisation="low", n=1, **{k: v for k, v in cu.golden_keywords(cu.golden_configs()[0]).items()
                                                     if k in ("model", "sgrna_threshold", "low_energy", "high_energy")})
    folds = c.folds()
    lines = folds.input().decode().splitlines()
    text = "".join(f"{line}\n{'.' * 100} ({-10.0 - (k % 25):.2f})\n" for k, line in enumerate(lines) if k % 7 != 3)
    folds.read(text)
    c.finish(folds)
    bowtie = c.bowtie(genome, 7, 0)
    sel = c.selected_tensor()
    rows = sel[::2].contiguous()
    k = rows.numel()
    mit, cfd = rng.uniform(0, 100, k), rng.uniform(0, 100, k)
    e = min(k, len(ru.SCORES))
    mit[:e], cfd[:e] = ru.SCORES[:e], ru.SCORES[:e][::-1]
    scores = (rows, torch.from_numpy(mit).cuda(), torch.from_numpy(cfd).cuda())
    host = dict(rows=c.rows, fold_rows=c.fold_rows, present=fold_present(c, folds), selection=c.selected, codes=bowtie.rows["code"],
                scored=rows.cpu().numpy(), mit=mit, cfd=cfd)
    genome.close()
    return gs, c, folds, bowtie, scores, host


def check_sizes(stages, cases):
    """cases: (batch size, [offtargetscore] page-length, method, threshold)."""
    gs, c, folds, bowtie, scores, host = stages
    for batch_size, page_length, method, threshold in cases:
        got = ca.BatchCounts(c, folds, bowtie, scores, threshold, method, batch_size, page_length)
        want = rm.batch_counts(host["rows"], 1, host["fold_rows"], host["present"], host["selection"], host["codes"], host["scored"],
                               host["mit"], host["cfd"], method, threshold, batch_size, page_length)
        what = (batch_size, page_length, method)
        same_counts(got.batches, want[0], what)
        assert got.page_failed.tolist() == want[1].tolist(), what
        assert got.not_found.tolist() == want[2].tolist(), what
    # without the folds the rows the consensus left untested are the ones not found: the same figures
    got = ca.BatchCounts(c, None, bowtie, scores, 75.0, "and", 17, 5)
    want = ca.BatchCounts(c, folds, bowtie, scores, 75.0, "and", 17, 5)
    assert got.batches.tobytes() == want.batches.tobytes() and got.not_found.tolist() == want.not_found.tolist()
    # no Bowtie step and no scores: the positions of an empty list, one empty page per batch under page length 0
    bare = ca.BatchCounts(c, folds, None, None, 75.0, "and", 64, 0)
    assert not bare.batches["bowtie_rejected"].any() and not bare.batches["scored_end"].any()
    assert bare.page_failed.tolist() == [0] * len(bare.batches)
    assert len(ca.BatchCounts(c, folds, None, None, 75.0, "and", 64, 9).page_failed) == 0


def test_seeded_300_guides_at_the_wave_and_workgroup_edges():
    stages = seeded_stages(300, 5)
    gs, c, folds, bowtie, scores, host = stages
    try:
        assert gs.n_guides == 300 and 0 < (host["present"] == 0).sum() < len(host["present"]) and len(host["scored"]) > 40
        assert (host["rows"]["ss"] == 3).any() and (host["codes"] == 0).any()
        sizes = (1, 17, 64, 255, 256, 257, 299, 300, 301, 5000000, 0)
        rules = [(0, "and", 75.0), (1, "or", 75.0), (7, "mit", 50.0), (5000000, "cfd", 99.99995), (3, "avg", 60.0), (2, "AND", 75.0),
                 (0, " Or ", 75.0), (7, "nothing", 75.0), (1, "and", 1e-6), (4, "mit", 100.0), (5, "avg", 0.0)]
        # every size under two rules, every rule under two sizes
        check_sizes(stages, [(b,) + rules[(k + d) % len(rules)] for k, b in enumerate(sizes) for d in (0, 4)])
    finally:
        folds.close()
        c.close()
        gs.close()


def test_seeded_several_workgroups():
    stages = seeded_stages(5000, 11)
    gs, c, folds, bowtie, scores, host = stages
    try:
        n = gs.n_guides
        assert n > 3 * 2048 and n % 2048 and c.n_fold > 2048 and len(host["scored"]) > 2048 and (host["codes"] == 0).sum() > 500
        check_sizes(stages, [(64, 0, "and", 75.0), (257, 1, "or", 75.0), (2047, 7, "mit", 50.0), (2048, 5000000, "cfd", 30.0),
                             (2049, 300, "avg", 60.0), (4096, 2048, "and", 75.0), (n - 1, 0, "or", 20.0), (n, 7, "mit", 75.0),
                             (0, 1, "cfd", 75.0), (1000, 4, "and", 99.0)])
    finally:
        folds.close()
        c.close()
        gs.close()


def fold_present(c, folds):
    out = np.zeros(c.n_fold, dtype=ca.FOLD_DTYPE)
    if c.n_fold:
        ca._lib.check(ca.lib.issl_folds_copy(folds._h, out.ctypes.data, None, len(out)))
    return out["present"]


# ---- 3. the Bowtie step's events -------------------------------------------------------------------------------------------

def device_events(genome, sigs, starts):
    import torch
    d_sigs = torch.from_numpy(np.ascontiguousarray(sigs).view(np.int64)).cuda()
    d_starts = torch.from_numpy(np.asarray(starts, dtype=np.uint64).view(np.int64)).cuda()
    rows, plain = (torch.zeros((len(sigs), 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    events = torch.full((len(starts) - 1,), 77, dtype=torch.int32, device="cuda")
    genome.occurrences_device(d_sigs, rows, page_starts=d_starts, page_events=events)
    genome.occurrences_device(d_sigs, plain, page_starts=d_starts)
    assert torch.equal(rows, plain), "the rows change with the events"
    return events.cpu().numpy().tolist(), rows.cpu().numpy().view(bu.DTYPE).reshape(-1)


def test_constructed_page_reject_accept_reject_counts_twice():
    blob, guides, a = rm.constructed_page()
    genome = ca.Genome.open([blob])
    try:
        sigs = np.array([bu.sig(g[:20]) for g in guides], dtype=np.uint64)
        events, rows = device_events(genome, sigs, [0, 3])
        assert events == [2] and rows["code"].tolist() == [2, 0, 2] and rows["source"][a] == 2
        events, rows = device_events(genome, sigs[:2], [0, 2])
        assert events == [1] and rows["code"].tolist() == [2, 1]
        events, rows = device_events(genome, sigs, [0, 1, 2, 3])
        assert events == [1, 0, 1] and rows["code"].tolist() == [0, 1, 0]
        events, rows = device_events(genome, sigs, [0, 0, 3, 3])
        assert events == [0, 2, 0]
    finally:
        genome.close()


def test_events_of_irregular_pages_against_the_loop():
    blob, model, planted, sigs = bu.adversarial()
    sigs = sigs[:3000]
    n = len(sigs)
    guides20 = [bu.unsig(s) for s in sigs]
    genome = ca.Genome.open([blob])
    try:
        rng = np.random.default_rng(9)
        cuts = np.sort(rng.choice(np.arange(1, n), 40, replace=False)).tolist()
        for starts in ([0, n], list(range(0, n, 7)) + [n], [0, 0] + cuts + [n, n], list(range(n + 1))):
            want, codes = rm.bowtie_events(model, guides20, starts)
            got, rows = device_events(genome, sigs, starts)
            assert got == want, (len(starts), [k for k, (x, y) in enumerate(zip(got, want)) if x != y][:5])
            assert rows["code"].tolist() == codes.tolist()
        assert sum(want) > 0
    finally:
        genome.close()


# ---- 4. the entry points' errors that need a consensus ---------------------------------------------------------------------

def test_state_and_argument_errors(golden):
    lib = ca.lib
    gs = ca.GuideSet.extract([ru.crafted_fasta(40, 2)])
    c = ca.Consensus(gs, optimisation="ultralow", n=1, mm10db=False, sgrnascorer2=False)
    other = ca.Consensus(gs, optimisation="ultralow", n=1, mm10db=True, sgrnascorer2=False)
    h = C.c_void_p()
    try:
        assert lib.issl_runlog_batches(c._h, None, None, 0, None, None, None, 0, 75.0, b"and", 0, 0, C.byref(h)) == -7 and h.value is None
        c.finish()
        folds = other.folds()
        assert lib.issl_runlog_batches(c._h, folds._h, None, 0, None, None, None, 0, 75.0, b"and", 0, 0, C.byref(h)) == -1
        folds.close()
        assert lib.issl_runlog_batches(c._h, None, None, 3, None, None, None, 0, 75.0, b"and", 0, 0, C.byref(h)) == -1
        assert lib.issl_runlog_batches(c._h, None, None, 0, None, None, None, 2, 75.0, b"and", 0, 0, C.byref(h)) == -1
        assert lib.issl_runlog_batches(c._h, None, None, 0, None, None, None, 0, 75.0, b"and", 7, 0, C.byref(h)) == 0
        n_batches, n_pages = C.c_uint64(), C.c_uint64()
        assert lib.issl_runlog_info(h, C.byref(n_batches), C.byref(n_pages), None, None) == 0
        assert n_batches.value == (gs.n_guides + 6) // 7 == n_pages.value
        out = np.zeros(n_batches.value, dtype=ca.BATCH_DTYPE)
        assert lib.issl_runlog_copy(h, out.ctypes.data, len(out) - 1, None, 0, None, 0) == -1
        assert lib.issl_runlog_copy(h, out.ctypes.data, len(out), None, 0, None, 0) == 0
        assert out["loaded"].sum() == gs.n_guides and out["consensus_tested"].tolist() == out["loaded"].tolist()
        assert lib.issl_runlog_close(h) == 0
    finally:
        other.close()
        c.close()
        gs.close()
