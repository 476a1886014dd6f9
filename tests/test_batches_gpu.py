"""GPU: a run in batches (pipeline.run with batch_size / rnafold_page_length, Genome.occurrences with page_starts,
Consensus.selection_pages, ResultTable with rows / header) against the reference's own output files for several
[input] batch-size and [rnafold] page-length (tests/golden/batches) and against the host model of tests/batches_util.py,
which tests/test_batches_model.py pins to those files."""
import numpy as np
import pytest

import crackling_amd as ca
import batches_util as bt
import bowtie_util as bu
import consensus_util as cu
import results_util as ru

pytestmark = pytest.mark.gpu
RUNS = bt.golden_runs()
IDS = [r["name"] for r in RUNS]
PIECE = 1 << 22  # sites per piece of the Bowtie step (include/issl_hip.h)


@pytest.fixture(scope="module")
def golden():
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    index = ca.IsslIndex.open(bu.GOLDEN / "index.issl").upload(0)
    yield genome, index
    index.close()
    genome.close()


@pytest.fixture(scope="module")
def adversarial():
    blob, model, planted, sigs = bu.adversarial()
    genome = ca.Genome.open([blob])
    yield genome, model, sigs, planted
    genome.close()


def golden_sigs():
    """The 20-mers of every guide of the golden input, in the order of the guide set: the selection at ultralow."""
    import guides_util as gu
    guides = gu.brute_force(gu.parse([(bu.GOLDEN / "input.fa").read_bytes()]))
    return np.array([bu.sig(s[:20]) for s in ru.guide_strings(guides)], dtype=np.uint64)


def device_rows(genome, sigs, page_length=0, page_starts=None, fill=None):
    """Genome.occurrences_device on tensors -> (rows as a structured array, the return of the call or its error)."""
    import torch
    d_sigs = torch.from_numpy(np.ascontiguousarray(sigs).view(np.int64)).cuda()
    d_rows = torch.full((len(sigs), 32), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
    d_starts = None if page_starts is None else torch.from_numpy(np.asarray(page_starts, dtype=np.uint64).view(np.int64)).cuda()
    error = None
    try:
        genome.occurrences_device(d_sigs, d_rows, page_length, page_starts=d_starts)
    except ca.IsslError as e:
        error = e
    return d_rows.cpu().numpy().view(bu.DTYPE).reshape(-1), error


# ---- 1. the reference's own files ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_golden_parity_through_the_pipeline(golden, run):
    """On a pipeline that ignores batch_size the files of medium_page0 with batches of 64, 50 and 17 differ from what it
    writes in 3 to 4 rows (the CCT-window pair lands in two batches), and [rnafold] page-length 0 in every folded row."""
    genome, index = golden
    whole = bt.golden_fold_text(run)
    asked = []

    def rnafold(fold_input):
        asked.append(fold_input)
        return bt.answer_page(whole, fold_input)

    got = ca.pipeline.run([ru.golden_input(run)], genome, index, bt.golden_keywords(run), rnafold)
    want = bt.golden_bytes(run["name"])
    if got != want:
        bad = [k for k, (a, b) in enumerate(zip(got.splitlines(), want.splitlines())) if a != b]
        raise AssertionError(f"{len(got)} bytes for {len(want)}; lines {bad[:8]} differ: {got.splitlines()[bad[0]]!r} != "
                             f"{want.splitlines()[bad[0]]!r}" if bad else f"{len(got)} bytes for {len(want)}")
    assert len(asked) == bt.rnafold_runs(run)
    if run["rnafold_page_length"]:
        assert all(0 < text.count("\n") <= run["rnafold_page_length"] for text in asked)


# ---- 2. explicit pages of one length are page_length ---------------------------------------------------------------------

def test_uniform_boundaries_give_the_bytes_of_page_length(adversarial, golden):
    genome, _, sigs, _ = adversarial
    for g, s in ((genome, sigs), (golden[0], golden_sigs())):
        n = len(s)
        assert n > 200
        for page_length in (0, 1, 7, n):
            want = g.occurrences(s, page_length)
            starts = bt.uniform_starts(n, page_length)
            assert g.occurrences(s, page_starts=starts).tobytes() == want.tobytes(), page_length
            got, error = device_rows(g, s, page_starts=starts)
            assert error is None and got.tobytes() == want.tobytes(), page_length
    assert genome.occurrences(np.zeros(0, dtype=np.uint64), page_starts=[0]).shape == (0,)
    assert genome.occurrences(np.zeros(0, dtype=np.uint64), page_starts=[0, 0, 0]).shape == (0,)


# ---- 3. pages of any length against the model -----------------------------------------------------------------------------

def test_irregular_pages_against_the_model(adversarial, golden):
    genome, model, sigs, _ = adversarial
    sigs = sigs[:3000]
    n = len(sigs)
    rng = np.random.default_rng(9)
    cuts = np.sort(rng.choice(np.arange(1, n), 40, replace=False)).tolist()
    cases = {"one page": [0, n],
             "pages of one": list(range(n + 1)),
             "mixed, pages of one among them": [0, 1, 2, 3] + [c for c in cuts if c > 3] + [n - 2, n - 1, n],
             "empty pages in front, in the middle and at the end": [0, 0, 0] + cuts[:20] + [cuts[20]] * 3 + cuts[21:] + [n, n, n]}
    for name, starts in cases.items():
        starts = sorted(starts)
        want = bt.paged_rows(model, sigs, starts)
        bu.same_rows(genome.occurrences(sigs, page_starts=starts), want)
        got, error = device_rows(genome, sigs, page_starts=starts)
        assert error is None, name
        bu.same_rows(got, want)
    # the CCT-window pair of the golden input: the strand-1 guide's group sets the verdict of the strand-0 guide
    g, gm, s = golden[0], bu.golden_model(), golden_sigs()
    one = gm.rows(s, 0)
    named = [(t, int(src)) for t, src in enumerate(one["source"]) if src != bu.NONE and s[int(src)] != s[t]]
    assert named, "no guide of the golden input is named by the group of a guide with another 20-mer"
    t, src = named[0]
    together = [0, len(s)]
    apart = [0, max(t, src), len(s)]
    for starts in (together, apart):
        want = bt.paged_rows(gm, s, starts)
        bu.same_rows(g.occurrences(s, page_starts=starts), want)
    assert bt.paged_rows(gm, s, together)["source"][t] == src and bt.paged_rows(gm, s, apart)["source"][t] != src


# ---- 4. a page across a piece edge ----------------------------------------------------------------------------------------

def large_queries(model, text_sigs, planted):
    """2^22 + 300 queries: random signatures; the text's own 20-mers around site 10 and on both sides of the piece edge, one
    of them at the last index of the first piece and the first of the second; the two guides of the CCT ... AGG window,
    the one on strand 0 for the last time five sites ahead of the edge, the one on strand 1 three behind it."""
    rng = np.random.default_rng(6)
    n = PIECE + 300
    q = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    own = text_sigs[np.nonzero(model.counts(text_sigs)["nb"])[0]]
    assert len(own) > 600
    q[:40] = np.resize(own[:13], 40)                         # the same 20-mers ahead of site 10 and behind it
    q[100:100 + len(own)] = own
    q[PIECE - 300:PIECE + 300] = np.resize(own, 600)
    q[PIECE - 1] = q[PIECE] = own[0]
    fwd, rev = bu.sig(planted["both"][:20]), bu.sig(bu.rc(planted["both"])[:20])
    behind = np.nonzero(q[PIECE - 4:] == fwd)[0] + PIECE - 4
    q[behind] = rng.integers(0, 1 << 40, len(behind), dtype=np.uint64)
    q[PIECE - 4], q[PIECE + 3] = fwd, rev
    return q


@pytest.mark.parametrize("starts", [[0, PIECE - 5, PIECE + 5, PIECE + 300], [0, 10, PIECE + 300]], ids=["ten sites around the edge", "from site 10 to the end"])
def test_pages_across_a_piece_edge(adversarial, starts):
    """2^22 + 300 sites: a page of ten sites around the edge between two pieces, and one from site 10 to the end -- where
    the look-up of a page's last site with a key walks over the pieces from a lower end that is no multiple of anything."""
    genome, model, sigs, planted = adversarial
    q = large_queries(model, sigs, planted)
    want = bt.paged_rows(model, q, starts)
    assert want["owner"][PIECE - 4] == 1 and want["source"][PIECE - 4] == PIECE + 3  # a verdict the second piece's group sets
    assert want["owner"][PIECE - 1] == 0 and want["source"][PIECE] == PIECE          # the pair lies in one page
    if starts[1] == 10:  # the ten sites ahead of the page name themselves, not their copies behind the boundary
        assert want["source"][:10].tolist() == list(range(10)) and want["owner"][10] == 0
    else:
        assert (want["owner"][:10] == 0).all()
    bu.same_rows(genome.occurrences(q, page_starts=starts), want)


# ---- 5. the pages of a batched run, made on the device ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["medium_page0", "ultralow_page0", "high_page0"])
def test_selection_pages_against_the_host_boundaries(name):
    run = next(r for r in ru.golden_runs() if r["name"] == name)
    with ca.GuideSet.extract([ru.golden_input(run)]) as gs, ca.Consensus(gs, **cu.golden_keywords(run)) as c:
        with pytest.raises(ca.IsslError) as e:
            c.selection_pages(0, 0)
        assert e.value.code == -7
        c.finish(ca.read_rnafold_output(bu.golden_folds(), c.fold_guides()) if c.n_fold else None)
        n, sel = gs.n_guides, c.selected
        assert n > 100 and (len(sel) == n if name.startswith("ultralow") else 0 < len(sel) < n)
        for batch_size in (0, 1, 17, n - 1, n, n + 1):
            for page_length in (0, 1, 7, 5000000):
                got = c.selection_pages(batch_size, page_length).cpu().numpy().astype(np.uint64).tolist()
                assert got == bt.page_starts(sel, n, batch_size, page_length).tolist(), (batch_size, page_length)
        if len(sel) < n:  # batches of one row: most hold no selected row and get no page
            assert len(c.selection_pages(1, 0)) == len(sel) + 1 < n
        step = c.bowtie(ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()]), 7, 17)
        assert step.batch_size == 17 and step.page_starts.cpu().tolist() == bt.page_starts(sel, n, 17, 7).tolist()
        sigs = gs.sigs_tensor().cpu().numpy().view(np.uint64)[sel.astype(np.int64)]
        bu.same_rows(step.rows, bt.paged_rows(bu.golden_model(), sigs, bt.page_starts(sel, n, 17, 7)))
        step.genome.close()


def test_selection_pages_of_an_empty_set_and_an_empty_selection():
    with ca.GuideSet.extract([b">none\nATATATATATATATATATATATATATATATAT\n"]) as gs, ca.Consensus(gs, model=cu.golden_model()) as c:
        c.finish()
        assert gs.n_guides == 0 and c.selection_pages(0, 0).cpu().tolist() == [0] and c.selection_pages(3, 2).cpu().tolist() == [0]
    blob = b">a\nACGTACGTTGCATGCAAGCTAGGTT\n>b\nACGTACGTTGCATGCAAGCTAGGTT\n"  # one guide, seen twice: nothing is selected
    with ca.GuideSet.extract([blob]) as gs, ca.Consensus(gs, optimisation="low", model=cu.golden_model()) as c:
        c.finish(np.zeros(c.n_fold, dtype=ca.FOLD_DTYPE) if c.n_fold else None)
        assert gs.n_guides == 1 and c.n_selected == 0
        for batch_size, page_length in ((0, 0), (1, 1), (5, 0)):
            assert c.selection_pages(batch_size, page_length).cpu().tolist() == [0]


# ---- 6. boundaries that do not tile the sites ---------------------------------------------------------------------------

def test_bad_boundaries_are_refused_before_any_row_is_written(adversarial):
    genome, _, sigs, _ = adversarial
    sigs = sigs[:1000]
    n = len(sigs)
    for name, starts in {"the first is not 0": [1, 500, n], "the last is not n": [0, 500, n - 1], "the last is beyond n": [0, 500, n + 1],
                         "a decrease": [0, 600, 500, n], "no page for the sites": [0]}.items():
        with pytest.raises(ca.IsslError) as e:
            genome.occurrences(sigs, page_starts=starts)
        assert e.value.code == -1, name
        got, error = device_rows(genome, sigs, page_starts=starts, fill=0xAB)
        assert error is not None and error.code == -1, name
        assert (got.view(np.uint8) == 0xAB).all(), name  # the rows are as they were
    with pytest.raises(ca.IsslError) as e:
        genome.occurrences(np.zeros(0, dtype=np.uint64), page_starts=[0, 1])
    assert e.value.code == -1
    got, error = device_rows(genome, sigs, page_starts=[0, 500, n])  # and the handle is as good as before
    assert error is None
    bu.same_rows(got, bt.paged_rows(adversarial[1], sigs, [0, 500, n]))


# ---- 7. the table by row range ----------------------------------------------------------------------------------------------

class Crafted:
    """Guide set, consensus, Bowtie step and scores of one crafted FASTA (as tests/test_results_gpu.py builds its own)."""

    def __init__(self, n_guides, seed, long_header=0):
        import torch
        self.blob = ru.crafted_fasta(n_guides, seed, long_header)
        self.gs = ca.GuideSet.extract([self.blob])
        assert self.gs.n_guides == n_guides
        self.genome = ca.Genome.open([self.blob])
        self.c = ca.Consensus(self.gs, optimisation="ultralow", n=2, model=cu.golden_model())
        rng = np.random.default_rng(seed)
        folds = np.zeros(self.c.n_fold, dtype=ca.FOLD_DTYPE)
        folds["energy"] = rng.choice([-35.0, -30.0, -29.9, -18.0, -17.9, -5.3], self.c.n_fold)
        folds["scaffold"] = rng.integers(0, 2, self.c.n_fold)
        folds["present"] = rng.integers(0, 5, self.c.n_fold) > 0
        self.c.finish(folds if self.c.n_fold else None)
        self.bowtie = self.c.bowtie(self.genome, 7, 64)
        scores = ru.crafted_scores(self.c.selected, seed)
        self.d_scores = tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int64 if k == 0 else np.float64)).cuda()
                              for k, x in enumerate(scores))
        self.texts = ru.crafted_fold_texts(self.c.n_fold, seed, ",")

    def table(self, texts="list", **kw):
        texts = self.texts if texts == "list" else texts
        return ca.ResultTable(self.c, texts, self.bowtie, self.d_scores, ",", "and", 75.0, **kw)

    def close(self):
        self.c.close()
        self.genome.close()
        self.gs.close()


@pytest.fixture(scope="module")
def big():
    c = Crafted(700, 5, long_header=100000)
    yield c
    c.close()


@pytest.mark.parametrize("flags", [0, ca.results.DIRECT], ids=["staged", "direct"])
def test_row_ranges_join_to_the_whole_table(big, flags):
    n = big.gs.n_guides
    with big.table(flags=flags) as whole:
        want, offsets, per_group = whole.to_bytes(), whole.row_offsets_tensor().cpu().numpy().astype(np.int64), whole.rows_per_group
    lengths = np.diff(offsets)
    long_row = int(np.argmax(lengths))
    assert lengths[long_row] > 100000 and n > 2 * per_group + 1
    cuts = sorted({0, 1, per_group - 1, per_group, per_group + 1, long_row, long_row + 1, n})
    with big.table(rows=(0, 0), flags=flags) as t:
        header = t.to_bytes()
        assert t.n_rows == 0 and t.n_bytes == offsets[0] and t.row_offsets_tensor().cpu().tolist() == [offsets[0]]
    assert header == want[:offsets[0]] == (",".join(ru.ORDER) + "\n").encode()
    pieces = [header]
    packed = ca.PackedFolds(big.texts)
    for k, (a, b) in enumerate(zip([0] + cuts, cuts)):  # (the first range is empty)
        lo, hi = np.searchsorted(big.c.fold_rows, (a, b))
        texts = big.texts if k % 2 else packed.piece(int(lo), int(hi))  # the whole list, or the range's own texts alone
        with big.table(texts, rows=(a, b - a), header=False, flags=flags) as t:
            assert t.n_rows == b - a and t.first_row == a and t.n_bytes == offsets[b] - offsets[a]
            piece = t.to_bytes()
            assert piece == want[offsets[a]:offsets[b]], (a, b)
            assert (t.row_offsets_tensor().cpu().numpy() + offsets[a]).tolist() == offsets[a:b + 1].tolist()
            assert t.text_tensor().cpu().numpy().tobytes() == piece
        pieces.append(piece)
    assert b"".join(pieces) == want
    with big.table(rows=(per_group - 1, 3), flags=flags) as t:  # with the header row: the offsets start behind it
        assert t.to_bytes() == header + want[offsets[per_group - 1]:offsets[per_group + 2]]
        assert t.row_offsets_tensor().cpu().tolist()[0] == len(header)


def test_row_ranges_outside_the_set(big):
    n = big.gs.n_guides
    for rows in ((n + 1, 0), (n, 1), (0, n + 1), (5, n), (1 << 40, 1), (1, (1 << 64) - 1)):
        with pytest.raises(ca.IsslError) as e:
            big.table(rows=rows, header=False)
        assert e.value.code == -1, rows
    with big.table(rows=(n, 0), header=False) as t:
        assert t.n_bytes == 0 and t.to_bytes() == b"" and t.row_offsets_tensor().cpu().tolist() == [0]


# ---- 8. the pipeline's ways out -----------------------------------------------------------------------------------------------

def test_pieces_join_to_run_and_append_to_a_file(golden, tmp_path, monkeypatch):
    genome, index = golden
    run = next(r for r in RUNS if r["name"] == "medium_page7_batch17_fold5")
    whole = bt.golden_fold_text(run)
    args = ([ru.golden_input(run)], genome, index, bt.golden_keywords(run), lambda asked: bt.answer_page(whole, asked))
    want = bt.golden_bytes(run["name"])
    alive = {"now": 0, "peak": 0, "sizes": []}

    class Watched(ca.ResultTable):  # how many bytes of text are alive on the device at once
        def __init__(self, *a, **kw):
            self.counted = 0
            super().__init__(*a, **kw)
            self.counted = self.n_bytes
            alive["now"] += self.counted
            alive["peak"] = max(alive["peak"], alive["now"])
            alive["sizes"].append(self.n_bytes)

        def close(self):
            alive["now"] -= self.counted
            self.counted = 0
            super().close()

    monkeypatch.setattr(ca.pipeline, "ResultTable", Watched)
    pieces = list(ca.pipeline.batches(*args))
    n = want.count(b"\n") - 1
    assert b"".join(pieces) == want == ca.pipeline.run(*args)
    assert len(pieces) == 1 + -(-n // 17) and pieces[0] == (",".join(ru.ORDER) + "\n").encode()
    assert all(p.count(b"\n") == 17 for p in pieces[1:-1]) and 0 < pieces[-1].count(b"\n") <= 17
    assert alive["now"] == 0 and alive["peak"] == max(alive["sizes"]) == max(len(p) for p in pieces) < len(want) // 4
    out = tmp_path / "guides.txt"
    out.write_bytes(b"what was there\n")
    assert ca.pipeline.run_to_file(out, *args) == len(want)
    assert out.read_bytes() == b"what was there\n" + want
    # one batch: pieces of at most SCORE_CHUNK rows
    monkeypatch.setattr(ca.pipeline, "SCORE_CHUNK", 50)
    one = dict(bt.golden_keywords(run), batch_size=0)
    one.pop("rnafold_page_length")
    pieces = list(ca.pipeline.batches(args[0], genome, index, one, lambda asked: whole))
    assert [p.count(b"\n") for p in pieces] == [1] + [50] * (n // 50) + ([n % 50] if n % 50 else [])
    assert b"".join(pieces) == ru.golden_bytes("medium_page7")
