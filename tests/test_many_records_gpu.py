"""GPU: locate, the Bowtie step and what reads a record number behind them, on genomes with more records than the table of
record starts that k_locate_finish and k_occur_verdict keep in LDS (kLdsRecords; tests/many_records_util.py).  The sizes
stand on both sides of the switch -- K - 1 and K records run the <true> builds, K + 1 and 2K + 808 the <false> ones, by the
host's `n_records <= kLdsRecords` -- and every comparison is exact, against the brute force of locate_util and the model of
bowtie_util, which tests/test_many_records_model.py pins to these inputs on the CPU.  The consumers of a record number --
transcript counts from the rows, the result table, a whole run in batches -- run on the largest size alone."""
import csv
import io

import numpy as np
import pytest

import crackling_amd as ca
import batches_util as bt
import bowtie_util as bu
import consensus_util as cu
import guides_util as gu
import locate_util as lu
import many_records_util as mr
import oracle_util as ou
import results_util as ru
import runlog_model as rm
import transcripts_util as tu
from test_runlog_gpu import device_events

pytestmark = pytest.mark.gpu
K = mr.switch()
SIZES = mr.sizes()
LARGE = SIZES[-1]


@pytest.fixture(scope="module")
def opened():
    """n_records -> (many_records_util.case, Genome), one Genome per size for the module."""
    genomes = {}

    def get(n_records):
        if n_records not in genomes:
            genomes[n_records] = ca.Genome.open([mr.case(n_records)["blob"]])
        return mr.case(n_records), genomes[n_records]

    yield get
    for g in genomes.values():
        g.close()


def places(locs):
    return sorted(zip(locs["record"].tolist(), locs["pos"].tolist(), locs["strand"].tolist()))


def irregular_starts(n, seed):
    """Seeded cuts of [0, n) with empty pages in front, in the middle and at the end, and a page of one query."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(3, n), 40, replace=False)).tolist()
    return [0, 0, 1] + cuts[:20] + [cuts[20]] * 3 + cuts[21:] + [n, n]


# ---- locate ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_records", SIZES)
def test_locate_on_both_sides_of_the_switch(opened, n_records):
    c, g = opened(n_records)
    records, truth, q, last = c["records"], c["truth"], c["queries"], n_records - 1
    assert g.records == [(name, len(seq)) for name, seq in records] and len(g.records) == n_records
    assert g.n_bases == sum(len(seq) for _, seq in records)
    offsets, locs = g.locate(q)
    lu.check_locate(g.records, offsets, locs, q, truth)
    got = set(places(locs))
    assert {(last, 0, 0), (last, len(records[last][1]) - 23, 0), (last - 1, 0, 0), (last - 1, 0, 1)} <= got
    assert bu.sig(c["planted"]["past"][:20]) in set(q.tolist())  # asked, and check_locate found its range empty
    if n_records > K:
        assert (locs["record"] >= K).any() and (locs["record"] == K).any()
    if n_records > K + 3:
        size = len(records[K - 1][1])
        assert {(K - 1, size - 23, 0), (K, 0, 0), (K + 2, 0, 1)} <= got
    if n_records == LARGE:
        assert int((locs["record"] >= K).sum()) > 1000


def test_low_record_reads_are_located_alike_around_the_switch(opened):
    """The reads planted below record 10 are the same in the three sizes around the switch: so are their locations there."""
    seen = []
    for n_records in SIZES[:3]:
        c, g = opened(n_records)
        p = c["planted"]
        sites = np.array([bu.sig(p["dup"]), bu.sig(p["strands"][:20]), bu.sig(p["strands"][3:])], dtype=np.uint64)
        offsets, locs = g.locate(sites)
        lu.check_locate(g.records, offsets, locs, sites, c["truth"])
        low = [places(locs[int(a):int(b)][locs["record"][int(a):int(b)] < 10]) for a, b in zip(offsets, offsets[1:])]
        assert low == [[(mr.LOW_DUP, 2, 0), (mr.LOW_DUP, 31, 0)], [(mr.LOW_STRANDS, 7, 0)], [(mr.LOW_STRANDS, 10, 0)]]
        assert places(locs[int(offsets[0]):int(offsets[1])])[2:] == [(n_records - 6, 5, 0), (n_records - 6, 31, 0)]
        seen.append(low)
    assert seen[0] == seen[1] == seen[2]


def test_locate_device_entry_gives_the_host_bytes(opened):
    import torch
    c, g = opened(LARGE)
    q = c["queries"]
    want_off, want = g.locate(q)
    d_sites = torch.from_numpy(q.view(np.int64)).cuda()
    d_offs = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    assert g.locate_device(d_sites, d_offs, None) == len(want)
    d_locs = torch.full((16 * len(want),), 0xAB, dtype=torch.uint8, device="cuda")
    assert g.locate_device(d_sites, d_offs, d_locs) == len(want)
    torch.cuda.synchronize()
    assert d_locs.cpu().numpy().tobytes() == want.tobytes()
    assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()


# ---- occurrences ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page_length", [0, 7])
@pytest.mark.parametrize("n_records", SIZES)
def test_occurrences_on_both_sides_of_the_switch(opened, n_records, page_length):
    c, g = opened(n_records)
    q = c["queries"]
    want = c["model"].rows(q, page_length)
    got = g.occurrences(q, page_length)
    bu.same_rows(got, want)
    assert not got["reserved"].any() and not got["reserved2"].any()
    placed = got[got["record"] != bu.NONE]
    assert int(placed["record"].max()) == n_records - 1 and {0, 1, 2} <= set(got["code"].tolist())
    if n_records > K:
        assert (placed["record"] >= K).any()
    if n_records == LARGE:
        assert int((placed["record"] >= K).sum()) > 1000 and (placed["record"] == K).any()
        assert ((placed["record"] >= K) & (placed["strand"] == 1)).any() and ((placed["record"] >= K) & (placed["owner"] == 1)).any()


@pytest.mark.parametrize("n_records", SIZES)
def test_occurrences_with_irregular_pages(opened, n_records):
    c, g = opened(n_records)
    q = c["queries"]
    starts = irregular_starts(len(q), n_records)
    want = bt.paged_rows(c["model"], q, starts)
    assert want["code"][0] == 0 and {0, 1, 2} <= set(want["code"].tolist())  # (`dup` alone in its page: named, and rejected)
    got = g.occurrences(q, page_starts=starts)
    bu.same_rows(got, want)
    if n_records > K:
        assert ((got["record"] != bu.NONE) & (got["record"] >= K)).any()


def test_events_leave_the_rows_alone(opened):
    c, g = opened(LARGE)
    q = c["queries"][:3000]
    starts = irregular_starts(len(q), 3)
    want, codes = rm.bowtie_events(c["model"], [bu.unsig(s) for s in q], starts)
    got, rows = device_events(g, q, starts)  # (asserts that the rows equal the rows without events)
    assert got == want and sum(want) > 0
    assert rows["code"].tolist() == codes.tolist()
    bu.same_rows(rows, bt.paged_rows(c["model"], q, starts))
    assert ((rows["record"] != bu.NONE) & (rows["record"] >= K)).any()


def test_two_calls_give_the_same_bytes(opened):
    c, g = opened(LARGE)
    q = c["queries"]
    assert g.occurrences(q, 7).tobytes() == g.occurrences(q, 7).tobytes()
    offsets, locs = g.locate(q)
    again_off, again = g.locate(q)
    assert locs.tobytes() == again.tobytes() and offsets.tobytes() == again_off.tobytes()


# ---- what reads the record number afterwards --------------------------------------------------------------------------------

def chrom(name):
    """bowtieChr: the record's name up to the first blank."""
    return (name.split() or [b""])[0]


def annotation_gff(records):
    """Two transcripts of one gene on each of five sequences -- a low record, K - 1, K, K + 1 (which is empty) and the last
    -- and one transcript on '*', where the reference looks a guide up that does not occur."""
    lines = []
    for r in (mr.LOW_DUP, K - 1, K, K + 1, len(records) - 1):
        seq = chrom(records[r][0]).decode()
        lines += [tu.gff_line(seq, "mRNA", 1, 60, f"ID=a{r};Parent=g{r}"), tu.gff_line(seq, "mRNA", 1, 60, f"ID=b{r};Parent=g{r}"),
                  tu.gff_line(seq, "exon", 1, 12, f"ID=ea{r};Parent=a{r}"), tu.gff_line(seq, "exon", 30, 45, f"ID=fa{r};Parent=a{r}"),
                  tu.gff_line(seq, "exon", 1, 60, f"ID=eb{r};Parent=b{r}")]
    lines += [tu.gff_line("*", "mRNA", 0, 0, "ID=s;Parent=gs"), tu.gff_line("*", "exon", 0, 0, "ID=es;Parent=s")]
    return b"".join(lines)


def test_transcript_counts_from_rows_beyond_the_switch(opened):
    import torch
    c, g = opened(LARGE)
    records = c["records"]
    rows = g.occurrences(c["queries"], 7)
    gff = annotation_gff(records)
    with ca.Annotation.open(gff) as a:
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1, 32).copy()).cuda()
        d_out = torch.full((len(rows), 16), 0xAB, dtype=torch.uint8, device="cuda")
        a.hits_occurrences_device(g, d_rows, d_out)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(ca.TRANSCRIPT_HITS_DTYPE).reshape(-1)
        tested = np.flatnonzero(rows["code"] != 2)
        none = rows["record"][tested] == bu.NONE
        names = [b"*" if x else chrom(records[int(r)][0]) for x, r in zip(none, rows["record"][tested])]
        starts = np.where(none, 0, rows["pos"][tested].astype(np.int64) + 1)
        again = a.hits(names, starts)
        assert got[tested].tobytes() == again.tobytes()
        assert (got["status"][rows["code"] == 2] == 1).all() and (rows["code"] == 2).any()
    want = tu.Model(gff).rows(names, starts.tolist())
    for f in ("hit", "total", "status", "first"):
        assert np.array_equal(again[f], want[f]), f
    hit = got[tested]["hit"] > 0
    assert none.any() and (got[tested]["hit"][none] == 1).all()
    assert (hit & ~none & (rows["record"][tested] >= K)).any() and (hit & (rows["record"][tested] == K)).any()
    assert (hit & (rows["record"][tested] == LARGE - 1)).any() and {1, 2} <= set(got[tested]["hit"].tolist())


class Stages:
    """Guide set, consensus, Bowtie step and scores over the FASTA that is also the genome, as tests/test_results_gpu.py
    builds them for its crafted input -- with whatever number of guides the extraction finds."""

    def __init__(self, blob, genome, seed=5):
        import torch
        self.gs = ca.GuideSet.extract([blob])
        self.genome = genome
        self.c = ca.Consensus(self.gs, optimisation="ultralow", n=2, model=cu.golden_model())
        rng = np.random.default_rng(seed)
        folds = np.zeros(self.c.n_fold, dtype=ca.FOLD_DTYPE)
        folds["energy"] = rng.choice([-35.0, -30.0, -29.9, -18.0, -17.9, -5.3], self.c.n_fold)
        folds["scaffold"] = rng.integers(0, 2, self.c.n_fold)
        folds["present"] = rng.integers(0, 5, self.c.n_fold) > 0
        self.c.finish(folds if self.c.n_fold else None)
        self.bowtie = self.c.bowtie(genome, 7)
        self.scores = ru.crafted_scores(self.c.selected, seed)
        self.d_scores = tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int64 if k == 0 else np.float64)).cuda()
                              for k, x in enumerate(self.scores))
        self.seed = seed

    def table(self, delimiter):
        ft = ru.crafted_fold_texts(self.c.n_fold, self.seed, delimiter)
        t = ca.ResultTable(self.c, ft, self.bowtie, self.d_scores, delimiter, "and", 75.0)
        return t, ru.model_table(guides=self.gs.guides, record_names=[n for n, _ in self.gs.records], rows=self.c.rows,
                                 fold_rows=self.c.fold_rows, folds_text=ft, selection=self.c.selected, bowtie_rows=self.bowtie.rows,
                                 genome_names=[n for n, _ in self.genome.records], scores=self.scores, delimiter=delimiter,
                                 method="and", threshold=75.0)

    def close(self):
        self.c.close()
        self.gs.close()


def test_result_table_names_records_beyond_the_switch(opened):
    c, g = opened(LARGE)
    last = LARGE - 1
    s = Stages(c["blob"], g)
    try:
        want = gu.brute_force(gu.parse([c["blob"]]))
        gu.check_set(s.gs, gu.parse([c["blob"]]), want)
        assert int(s.gs.guides["record"].max()) == last and int((s.gs.guides["record"] >= K).sum()) > 1000
        sigs = np.array([bu.sig(x[:20]) for x in ru.guide_strings(s.gs.guides)], dtype=np.uint64)
        bu.same_rows(s.bowtie.rows, c["model"].rows(sigs[s.c.selected.astype(np.int64)], 7))
        for delimiter in (",", "\t"):
            t, (text, offsets) = s.table(delimiter)
            with t:
                got = t.to_bytes()
                assert got == text, next((a, b) for a, b in zip(got.splitlines(), text.splitlines()) if a != b)
                assert t.row_offsets_tensor().cpu().numpy().astype(np.uint64).tolist() == offsets.tolist()
            rows = list(csv.reader(io.StringIO(text.decode("latin-1"), newline=""), delimiter=delimiter, quotechar='"'))
            name = c["records"][last][0].decode()
            assert " " in name and rows[0] == ru.ORDER and len(rows) == s.gs.n_guides + 1
            header, chromosome = ru.ORDER.index("header"), ru.ORDER.index("bowtieChr")
            assert any(r[header] == name for r in rows[1:]) and any(r[chromosome] == name.split()[0] for r in rows[1:])
            assert not any(r[chromosome] == name for r in rows[1:])
            assert any(r[chromosome] == chrom(c["records"][K][0]).decode() for r in rows[1:])
    finally:
        s.close()


def test_a_run_in_batches_on_the_many_record_genome(opened, tmp_path):
    """pipeline.run over the FASTA as input and as genome, in batches of 257 with Bowtie pages of 7, against the host models
    of the stages put together as batches_util.host_stages does for the goldens: guides_util, consensus_util.Model (medium,
    no mm10db: nothing is folded), the Bowtie model per page of every batch, the C oracle over the index built from the
    same FASTA on the device."""
    c, g = opened(LARGE)
    blob, last = c["blob"], LARGE - 1
    sv, coef, intercept = cu.golden_model()
    consensus = dict(optimisation="medium", n=1, mm10db=False, chopchop=True, sgrnascorer2=True, model=(sv, coef, intercept),
                     sgrna_threshold=0.0, low_energy=-30.0, high_energy=-18.0)
    config = dict(consensus, offtargetscore=True, batch_size=257, page_length=7, max_distance=4, score_threshold=75.0, method="and",
                  delimiter=",")
    ix = ca.IsslIndex.build_from_fasta([blob])
    try:
        path = tmp_path / "many.issl"
        ix.write(path)

        def rnafold(text):
            raise AssertionError("nothing is to be folded")

        got = ca.pipeline.run([blob], g, ix, config, rnafold)
    finally:
        ix.close()
    records = gu.parse([blob])
    guides = gu.brute_force(records)
    seqs = ru.guide_strings(guides)
    n = len(seqs)
    m = cu.Model(seqs, guides["seen"], **consensus)
    assert len(m.fold_rows) == 0
    m.finish(None)
    sel = m.selected
    sigs = np.array([bu.sig(seqs[j][:20]) for j in sel], dtype=np.uint64)
    brows = bt.paged_rows(c["model"], sigs, bt.page_starts(sel, n, 257, 7))
    scored = sel[brows["code"] != 0]
    assert m.level == 2 and 1000 < len(scored) < len(sel) < n
    oracle = ou.OracleIndex(path)
    mit, cfd = oracle.score(np.array([bu.sig(seqs[j][:20]) for j in scored], dtype=np.uint64), 4, 75.0, "and")
    oracle.close()
    want, _ = ru.model_table(guides=guides, record_names=[name for name, _ in records], rows=m.rows, fold_rows=m.fold_rows, folds_text=[],
                             selection=sel, bowtie_rows=brows, genome_names=[name for name, _ in c["records"]], scores=(scored, mit, cfd),
                             delimiter=",", method="and", threshold=75.0)
    if got != want:
        bad = [k for k, (a, b) in enumerate(zip(got.splitlines(), want.splitlines())) if a != b]
        raise AssertionError(f"{len(got)} bytes for {len(want)}; lines {bad[:8]} differ: {got.splitlines()[bad[0]]!r} != "
                             f"{want.splitlines()[bad[0]]!r}" if bad else f"{len(got)} bytes for {len(want)}")
    rows = list(csv.reader(io.StringIO(want.decode("latin-1"), newline="")))
    chromosome = ru.ORDER.index("bowtieChr")
    assert sum(r[chromosome] not in ("?", "*") and int(r[chromosome][1:]) >= K for r in rows[1:]) > 500
