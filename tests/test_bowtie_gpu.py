"""GPU: the Bowtie step (crackling_amd.Genome.occurrences*, Consensus.bowtie, GuideSet.score(bowtie=), bin/cracklingBowtie)
against the reference's own run (tests/golden/bowtie) and, field by field, against the model of tests/bowtie_util.py,
which tests/test_bowtie_host.py pins to that run."""
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
import bowtie_util as bu
import consensus_util as cu

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CONFIGS = bu.golden_configs()
IDS = [c["name"] for c in CONFIGS]
PIECE = 1 << 22  # kPieceSites of issl_genome.hpp: queries per scan of the text
EXE = str(ROOT / "bin" / "cracklingBowtie")
COLUMNS = ("passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd")


@pytest.fixture(scope="module")
def golden():
    """(guide set of input.fa, genome of genome.fa, uploaded index.issl), once for the module."""
    gs = ca.GuideSet.extract([(bu.GOLDEN / "input.fa").read_bytes()])
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    index = ca.IsslIndex.open(bu.GOLDEN / "index.issl").upload(0)
    yield gs, genome, index
    index.close()
    genome.close()
    gs.close()


@pytest.fixture(scope="module")
def adversarial():
    blob, model, planted, sigs = bu.adversarial()
    genome = ca.Genome.open([blob])
    yield genome, model, sigs, planted
    genome.close()


# ---- the reference's own run -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_golden_parity(golden, cfg):
    gs, genome, index = golden
    want = bu.golden_rows(cfg["name"])
    guides = gs.strings()
    assert guides == [w["seq"] for w in want]
    sel = bu.golden_selection(cfg, want)
    with gs.consensus(cu.golden_keywords(cfg)) as c:
        c.finish(ca.read_rnafold_output(bu.golden_folds(), c.fold_guides()))
        assert c.selected.tolist() == sel
        b = c.bowtie(genome, cfg["page_length"])
        assert b.rows.dtype == ca.OCCURRENCE_DTYPE and len(b.rows) == len(sel)
        assert b.columns() == bu.golden_columns(want, sel)
        rest = sorted(set(range(len(want))) - set(sel))
        assert all(want[k][col] == "?" for k in rest for col in COLUMNS)
        bu.same_rows(b.rows, bu.golden_model().rows(ca.encode_guides([guides[k][:20] for k in sel]), cfg["page_length"]))
        assert not b.rows["reserved"].any() and not b.rows["reserved2"].any()
        # what goes on to scoring, and what comes back
        scored = [k for k, w in enumerate(want) if w["mitOfftargetscore"] != "?"]
        assert b.selected_tensor().cpu().numpy().tolist() == scored
        assert (len(scored) < len(sel)) == (cfg["optimisation"] != "ultralow")
        idx, mit, cfd = gs.score(index, cfg["max_distance"], float(cfg["score_threshold"]), cfg["method"], consensus=c, bowtie=b)
        assert idx.tolist() == scored
        lines = ca.format_scores(ca.encode_guides([guides[k][:20] for k in idx]), mit, cfd, cfg["method"]).splitlines()
        assert [ln.split("\t")[0] for ln in lines] == [guides[k][:20] for k in scored]
        assert [repr(float(ln.split("\t")[1])) for ln in lines] == [want[k]["mitOfftargetscore"] for k in scored]
        assert [repr(float(ln.split("\t")[2])) for ln in lines] == [want[k]["cfdOfftargetscore"] for k in scored]
        verdict = ca.verdicts([float(ln.split("\t")[1]) for ln in lines], [float(ln.split("\t")[2]) for ln in lines],
                              float(cfg["score_threshold"]), cfg["method"])
        assert [str(v) for v in verdict] == [want[k]["passedOffTargetScore"] for k in scored]
        assert all(want[k]["passedOffTargetScore"] == "?" for k in set(range(len(want))) - set(scored))
        # without the keyword: today's behaviour, the whole selection
        idx_all, _, _ = gs.score(index, cfg["max_distance"], float(cfg["score_threshold"]), cfg["method"], consensus=c)
        assert idx_all.tolist() == sel
        with gs.consensus(cu.golden_keywords(cfg)) as other:
            with pytest.raises(ValueError):
                gs.score(index, consensus=other, bowtie=b)
        with pytest.raises(ValueError):
            gs.score(index, bowtie=b)


# ---- the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page_length", [0, 1, 5, "n"])
def test_model_parity_on_adversarial_text(adversarial, page_length):
    genome, model, sigs, _ = adversarial
    page_length = len(sigs) if page_length == "n" else page_length
    got = genome.occurrences(sigs, page_length)
    bu.same_rows(got, model.rows(sigs, page_length))
    assert not got["reserved"].any() and not got["reserved2"].any()
    assert {0, 1, 2} <= set(got["code"].tolist()) or page_length == 1
    # strings are taken as well as signatures
    few = [bu.unsig(x) for x in sigs[:50]]
    assert genome.occurrences(few, page_length).tobytes() == genome.occurrences(sigs[:50], page_length).tobytes()


def test_two_runs_give_the_same_bytes(adversarial):
    genome, _, sigs, _ = adversarial
    assert genome.occurrences(sigs, 5).tobytes() == genome.occurrences(sigs, 5).tobytes()
    assert genome.occurrences(sigs).tobytes() == genome.occurrences(sigs).tobytes()


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_small_query_counts(adversarial, n):
    genome, model, sigs, _ = adversarial
    hot = sigs[np.nonzero(model.counts(sigs)["nb"])[0]]          # queries that occur, first: a single one is not a miss
    q = np.concatenate([hot, sigs])[:n]
    got = genome.occurrences(q)
    assert got.dtype == ca.OCCURRENCE_DTYPE and len(got) == n
    bu.same_rows(got, model.rows(q))
    if n:
        assert got["nb"][0] > 0


_large = []


def large_queries(model, text_sigs, planted):
    """2^22 + 5 queries: random signatures; the text's own 20-mers twice, once on both sides of the piece boundary; one
    20-mer of the text at the last index of the first piece and the first of the second; and the two guides of the
    CCT ... AGG window, the one on strand 0 for the last time ahead of the boundary, the one on strand 1 behind it."""
    if not _large:
        rng = np.random.default_rng(5)
        q = rng.integers(0, 1 << 40, PIECE + 5, dtype=np.uint64)
        own = text_sigs[np.nonzero(model.counts(text_sigs)["nb"])[0]]
        assert len(own) > 600
        q[100:100 + len(own)] = own
        q[PIECE - 300:] = own[:305]                              # runs over the boundary
        q[PIECE - 1] = q[PIECE] = own[0]
        fwd, rev = bu.sig(planted["both"][:20]), bu.sig(bu.rc(planted["both"])[:20])
        behind = np.nonzero(q[PIECE:] == fwd)[0] + PIECE
        q[behind] = rng.integers(0, 1 << 40, len(behind), dtype=np.uint64)
        q[PIECE - 5], q[PIECE + 3] = fwd, rev
        _large.append(q)
    return _large[0]


@pytest.mark.parametrize("page_length", [0, 1000003])
def test_more_queries_than_a_piece(adversarial, page_length):
    """Rows across the boundary of 2^22 queries: a page that runs over it names its last query of a 20-mer wherever it lies."""
    genome, model, sigs, planted = adversarial
    q = large_queries(model, sigs, planted)
    want = model.rows(q, page_length)
    assert PIECE % 1000003 and want["owner"][PIECE - 1] == 0 and want["owner"][PIECE] == 1  # the pair lies in one page
    assert (want["nb"] > 0).sum() > 900 and {0, 1, 2} <= set(want["code"].tolist())
    assert want["owner"][PIECE - 5] == 1 and want["source"][PIECE - 5] == PIECE + 3  # a verdict the second piece's group sets
    got = genome.occurrences(q, page_length)
    bu.same_rows(got, want)


def test_device_entry_on_another_stream(adversarial):
    import torch
    genome, model, sigs, _ = adversarial
    d_sites = torch.from_numpy(sigs.view(np.int64)).cuda()
    before = d_sites.clone()
    d_rows = torch.full((len(sigs), 32), 0xAB, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        genome.occurrences_device(d_sites, d_rows, 5, stream=stream.cuda_stream)
    stream.synchronize()
    assert d_rows.cpu().numpy().tobytes() == genome.occurrences(sigs, 5).tobytes()
    assert torch.equal(d_sites, before)
    genome.occurrences_device(d_sites[:0], d_rows[:0])           # nothing to do, nothing written
    with pytest.raises(ValueError):
        genome.occurrences_device(d_sites, d_rows[:10])


def test_bits_above_the_twenty_bases_are_refused(adversarial):
    genome, _, sigs, _ = adversarial
    bad = sigs[:100].copy()
    bad[77] |= np.uint64(1) << np.uint64(40)
    with pytest.raises(ca.IsslError) as e:
        genome.occurrences(bad)
    assert e.value.code == -1 and "20 bases" in e.value.message
    assert genome.occurrences(sigs[:100]).tobytes() == genome.occurrences(sigs[:100]).tobytes()  # the handle goes on


# ---- the executable -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,width", [("ultralow_page0", 23), ("ultralow_page7", 20), ("high_page0", 23)])
def test_executable_prints_the_reference_columns(tmp_path, name, width):
    cfg = next(c for c in CONFIGS if c["name"] == name)
    want = bu.golden_rows(name)
    sel = bu.golden_selection(cfg, want)
    guides = [want[k]["seq"][:width] for k in sel]
    path = tmp_path / "guides.txt"
    path.write_text("".join(g + "\n" for g in guides))
    r = subprocess.run([EXE, "--page-length", str(cfg["page_length"]), str(path), str(bu.GOLDEN / "genome.fa")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    nb = bu.golden_model().rows(ca.encode_guides([g[:20] for g in guides]), cfg["page_length"])["nb"]
    assert r.stdout == "".join("\t".join([g, want[k]["passedBowtie"], str(n), want[k]["bowtieChr"], want[k]["bowtieStart"],
                                          want[k]["bowtieEnd"]]) + "\n" for g, k, n in zip(guides, sel, nb))


def test_executable_refuses_a_malformed_guides_file(tmp_path):
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGTACGTACGTACGTACGT\nACGT\n")
    r = subprocess.run([EXE, str(bad), str(bu.GOLDEN / "genome.fa")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and "query file is not a multiple" in r.stderr
    scorer = subprocess.run([str(ROOT / "bin" / "isslScoreOfftargets"), str(bu.GOLDEN / "index.issl"), str(bad), "4", "75", "and"],
                            capture_output=True, text=True)
    assert scorer.returncode == r.returncode
    r = subprocess.run([EXE, "--page-length", "x", str(bad), str(bu.GOLDEN / "genome.fa")], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr
