"""GPU: transcript hit counts (crackling_amd.Annotation, BowtieStep.transcripts, bin/countHitTranscripts) against the
reference's own answers (tests/golden/transcripts) and, field by field, against the model of tests/transcripts_util.py,
which tests/test_transcripts_model.py pins to those answers."""
import csv
import io
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
import bowtie_util as bu
import consensus_util as cu
import transcripts_util as tu

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "countHitTranscripts")
CASES = tu.cases()
IDS = [c["name"] for c in CASES]
ANNOTATIONS = sorted({c["annotation"] for c in CASES})
WAVE = 64        # kWaveSpan of issl_transcripts.hip: ranges and lists from this length on are walked by the wave
GROUP = 256      # rows of a query workgroup
E_FORMAT, E_UNSUPPORTED = -3, -4


def same_rows(got, want):
    assert got.dtype == ca.TRANSCRIPT_HITS_DTYPE and len(got) == len(want)
    for f in ("hit", "total", "status", "first"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), f"{f} differs at {bad[:5].tolist()}: got {got[f][bad[:5]].tolist()}, want {want[f][bad[:5]].tolist()}"


def around_breakpoints(model):
    """Every breakpoint of every sequence at -1, 0 and +1."""
    names, starts = [], []
    for seq in model.seqs:
        for p in model.breakpoints(seq):
            for d in (-1, 0, 1):
                names.append(seq)
                starts.append(p + d)
    return names, starts


def parsed(path):
    text = path.read_bytes().decode().replace("\r\n", "\n").replace("\r", "\n")
    return list(csv.reader(io.StringIO(text, newline=""), delimiter=",", quotechar='"'))


def opens(blob):
    try:
        tu.Model(blob)
    except tu.FormatError:
        return False
    return True


# ---- the reference's own answers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_through_hits(case):
    blob = case["annotation"].read_bytes()
    if not opens(blob):
        with pytest.raises(ca.IsslError) as e:
            ca.Annotation.open(blob)
        assert e.value.code == E_FORMAT
        return
    if case.get("error"):
        return                                        # the Crackling file is at fault: the executable's business
    rows, want = parsed(case["crackling"]), parsed(case["expected"])
    if not rows:
        assert not want
        return
    chrom, start = rows[0].index("bowtieChr"), rows[0].index("bowtieStart")
    asked = [k for k in range(1, len(rows)) if rows[k][chrom] != "?"]
    with ca.Annotation.open(blob) as a:
        got = a.hits([rows[k][chrom] for k in asked], [int(rows[k][start]) for k in asked])
        by_path = ca.Annotation.open(case["annotation"])
        assert by_path.info == a.info and by_path.seqs == a.seqs
        by_path.close()
    assert ca.format_hits(got) == [want[k][-1] for k in asked]
    assert all(want[k][-1] == "?/?" for k in range(1, len(rows)) if k not in asked) and want[0][-1] == "hits"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_through_the_executable(tmp_path, case):
    out = tmp_path / "out.csv"
    r = subprocess.run([EXE, "--annotation", str(case["annotation"]), "--crackling", str(case["crackling"]), "--output", str(out)],
                       capture_output=True, text=True)
    if case.get("error"):
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("countHitTranscripts: ") and not out.exists()
    else:
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stderr
        assert out.read_bytes() == case["expected"].read_bytes()
        assert not pathlib.Path(str(case["annotation"]) + ".p").exists()


def test_executable_short_options_and_usage(tmp_path):
    case = next(c for c in CASES if c["name"] == "sample")
    out = tmp_path / "o.csv"
    r = subprocess.run([EXE, "-a", str(case["annotation"]), "-c", str(case["crackling"]), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and out.read_bytes() == case["expected"].read_bytes()
    r = subprocess.run([EXE, "-a", str(case["annotation"]), "-c", str(tmp_path / "absent.csv"), "-o", str(tmp_path / "p.csv")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stderr and not (tmp_path / "p.csv").exists()
    r = subprocess.run([EXE, "--sample"], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr


# ---- the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ANNOTATIONS, ids=[p.parent.name for p in ANNOTATIONS])
def test_every_breakpoint_of_the_golden_annotations(path):
    blob = path.read_bytes()
    if not opens(blob):
        return
    model = tu.Model(blob)
    names, starts = around_breakpoints(model)
    names += [b"*", b"?", b"", b"absent"] + [s.replace(b"_", b".") for s in model.seqs]
    starts += [0, 0, 5, 5] + [1] * len(model.seqs)
    with ca.Annotation.open(blob) as a:
        assert a.info == model.info and a.seqs == model.seqs
        assert [a.lookup(s) for s in model.seqs] == list(range(len(model.seqs))) and a.lookup("no such sequence") == 0xFFFFFFFF
        same_rows(a.hits(names, starts), model.rows(names, starts))


_random = {}


def random_case(n_seqs):
    """(blob, model, names, starts, want) for an annotation of about 3000 exons over n_seqs sequences, made once."""
    if n_seqs not in _random:
        rng = np.random.default_rng(100 + n_seqs)
        blob = tu.random_annotation(rng, n_seqs, 3000, span=max(20_000, 200_000 // n_seqs))  # genes overlap at every n_seqs
        model = tu.Model(blob)
        names, starts = tu.random_queries(rng, model, 20000)
        _random[n_seqs] = (blob, model, names, starts, model.rows(names, starts))
    return _random[n_seqs]


@pytest.mark.parametrize("n_seqs", [1, 3, 40])
def test_random_annotations(n_seqs):
    blob, model, names, starts, want = random_case(n_seqs)
    assert min(starts) < 0 and max(starts) > 1 << 40 and b"absent" in names
    assert {0, 2, 3} <= set(want["status"].tolist()) and (want["hit"] > want["total"])[want["status"] == 0].any()
    with ca.Annotation.open(blob) as a:
        assert a.info == model.info
        same_rows(a.hits(names, starts), want)
        b_names, b_starts = around_breakpoints(model)
        same_rows(a.hits(b_names, b_starts), model.rows(b_names, b_starts))


def test_two_opens_give_the_same_bytes():
    blob, model, names, starts, _ = random_case(3)
    b_names, b_starts = around_breakpoints(model)
    with ca.Annotation.open(blob) as a, ca.Annotation.open(blob) as b:
        assert a.hits(b_names, b_starts).tobytes() == b.hits(b_names, b_starts).tobytes()
        assert a.hits(names, starts).tobytes() == b.hits(names, starts).tobytes() == a.hits(names, starts).tobytes()


# ---- the sizes at which the kernels change shape ------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, WAVE - 1, WAVE, WAVE + 1, 5001])
def test_an_exon_over_k_segments(k):
    blob = tu.long_exon_annotation(k)
    model = tu.Model(blob)
    (s, e), = model.exons[(b"chrL", b"long")]
    assert sum(1 for p in model.breakpoints(b"chrL") if s <= p <= e) == k
    names, starts = around_breakpoints(model)
    want = model.rows(names, starts)
    assert want["hit"].max() == min(k, 2) and (want["first"][want["hit"] > 0] == 0).all()
    with ca.Annotation.open(blob) as a:
        assert a.info == model.info
        same_rows(a.hits(names, starts), want)


@pytest.mark.parametrize("twice", [False, True], ids=["once", "twice"])
@pytest.mark.parametrize("k", [1, WAVE - 1, WAVE, WAVE + 1, 3000])
def test_a_segment_under_k_transcripts(k, twice):
    blob = tu.deep_segment_annotation(k, twice)
    model = tu.Model(blob)
    names, starts = around_breakpoints(model)
    want = model.rows(names, starts)
    assert want["hit"].max() == k and (want["total"][want["hit"] > 0] == k).all()
    with ca.Annotation.open(blob) as a:
        assert a.info == model.info
        same_rows(a.hits(names, starts), want)


def test_long_lists_decide_genes_like_short_ones():
    """A list of more than 64 transcripts whose one stranger -- another gene, or no mRNA line -- sits anywhere in it."""
    for stranger, attributes, status in ((0, "ID=x;Parent=other", 2), (70, "ID=x;Parent=other", 2), (0, None, 3), (70, None, 0)):
        lines = []
        for i in range(100):
            if i == stranger:
                if attributes:
                    lines.append(tu.gff_line("c", "mRNA", 1, 2, attributes))
                lines.append(tu.gff_line("c", "exon", 10, 20, "ID=ex;Parent=x"))
            lines.append(tu.gff_line("c", "mRNA", 1, 2, f"ID=t{i};Parent=g"))
            lines.append(tu.gff_line("c", "exon", 10, 20, f"ID=e{i};Parent=t{i}"))
        blob = b"".join(lines)
        model = tu.Model(blob)
        want = model.rows([b"c"] * 3, [9, 10, 21])
        assert want[1]["hit"] == 101 and want[1]["status"] == status and want[1]["first"] == 0
        with ca.Annotation.open(blob) as a:
            same_rows(a.hits([b"c"] * 3, [9, 10, 21]), want)


@pytest.mark.parametrize("n", [0, 1, GROUP - 1, GROUP, GROUP + 1])
def test_row_counts_around_a_workgroup(n):
    import torch
    blob, model, names, starts, want = random_case(3)
    with ca.Annotation.open(blob) as a:
        same_rows(a.hits(names[:n], starts[:n]), want[:n])
        seq = np.array([a.lookup(x) for x in names[:n]], dtype=np.uint32)
        same_rows(a.hits(seq, starts[:n]), want[:n])
        d_seq = torch.from_numpy(seq.view(np.int32)).cuda()
        d_start = torch.tensor(starts[:n], dtype=torch.int64).cuda()
        d_out = torch.full((n + 1, 16), 0xAB, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            a.hits_device(d_seq, d_start, d_out, stream=stream.cuda_stream)
        stream.synchronize()
        host = d_out.cpu().numpy()
        same_rows(host[:n].reshape(-1).view(ca.TRANSCRIPT_HITS_DTYPE), want[:n])
        assert (host[n] == 0xAB).all()                # nothing behind the last row
        if n:
            with pytest.raises(ValueError):
                a.hits_device(d_seq, d_start, d_out[:n - 1])


# ---- bounds -------------------------------------------------------------------------------------------------------------

def test_coordinates_at_the_bound():
    top = tu.MAX_COORD
    blob = (tu.gff_line("c", "mRNA", 1, 2, "ID=t;Parent=g") + tu.gff_line("c", "exon", top - 1, top, "ID=e;Parent=t")
            + tu.gff_line("c", "exon", -7, 2, "ID=f;Parent=t") + tu.gff_line("c", "exon", -9, -3, "ID=h;Parent=t")
            + tu.gff_line("c", "exon", top + 5, top + 4, "ID=i;Parent=t"))
    model = tu.Model(blob)
    names = [b"c"] * 10
    starts = [top - 2, top - 1, top, top + 1, top + 2, (1 << 63) - 1, 0, 2, 3, -(1 << 63)]
    want = model.rows(names, starts)
    assert want["hit"].tolist() == [0, 1, 1, 0, 0, 0, 1, 1, 0, 0]
    with ca.Annotation.open(blob) as a:
        assert a.info == model.info
        same_rows(a.hits(names, starts), want)
    for beyond in (tu.gff_line("c", "exon", top, top + 1, "ID=z;Parent=t"), tu.gff_line("c", "exon", -1, 1 << 62, "ID=z;Parent=t")):
        with pytest.raises(ca.IsslError) as e:
            ca.Annotation.open(blob + beyond)
        assert e.value.code == E_UNSUPPORTED and "2^40 - 2" in e.value.message


def test_an_annotation_without_a_counted_line():
    with ca.Annotation.open(b"##gff-version 3\nc\tx\tgene\t1\t9\t.\t+\t.\tID=g\n") as a, ca.Annotation.open(b"") as b:
        for x in (a, b):
            assert x.info == {"n_seqs": 0, "n_transcripts": 0, "n_genes": 0, "n_exons": 0, "n_segments": 0} and x.seqs == []
            assert ca.format_hits(x.hits(["c", "*", ""], [5, 0, -1])) == ["0/0"] * 3
    with ca.Annotation.open(tu.gff_line("c", "gene", 1, 9, "ID=g;Parent=p") + tu.gff_line("d", "mRNA", 1, 9, "ID=t;Parent=g")) as a:
        assert a.info == {"n_seqs": 2, "n_transcripts": 1, "n_genes": 1, "n_exons": 0, "n_segments": 0} and a.seqs == [b"c", b"d"]
        assert ca.format_hits(a.hits(["c", "d"], [5, 5])) == ["0/0"] * 2


# ---- the rows of the Bowtie step ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bowtie_golden():
    gs = ca.GuideSet.extract([(bu.GOLDEN / "input.fa").read_bytes()])
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    annotation = ca.Annotation.open(tu.GOLDEN / "bowtie" / "annotation.gff")
    yield gs, genome, annotation
    annotation.close()
    genome.close()
    gs.close()


@pytest.mark.parametrize("cfg", bu.golden_configs(), ids=[c["name"] for c in bu.golden_configs()])
def test_bowtie_step_transcripts(bowtie_golden, cfg):
    gs, genome, annotation = bowtie_golden
    want = bu.golden_rows(cfg["name"])
    sel = bu.golden_selection(cfg, want)
    expected = parsed(tu.GOLDEN / "bowtie" / f"{cfg['name']}.expected.csv")
    assert expected[0][-1] == "hits" and [r[0] for r in expected[1:]] == [w["seq"] for w in want]
    hits = [r[-1] for r in expected[1:]]
    with gs.consensus(cu.golden_keywords(cfg)) as c:
        c.finish(ca.read_rnafold_output(bu.golden_folds(), c.fold_guides()))
        step = c.bowtie(genome, cfg["page_length"])
        t = step.transcripts(annotation)
        assert t.rows_tensor().is_cuda and tuple(t.rows_tensor().shape) == (len(sel), 16)
        assert t.rows.dtype == ca.TRANSCRIPT_HITS_DTYPE and t.column() == [hits[k] for k in sel]
        assert all(hits[k] == "?/?" for k in set(range(len(want))) - set(sel))
        # the same answers from the columns the reference prints
        cols = step.columns()
        asked = [k for k, ch in enumerate(cols["bowtieChr"]) if ch != "?"]
        again = annotation.hits([cols["bowtieChr"][k] for k in asked], [int(cols["bowtieStart"][k]) for k in asked])
        assert t.rows[asked].tobytes() == again.tobytes()
        assert (t.rows["status"][[k for k in range(len(sel)) if k not in asked]] == 1).all()
        # a guide that does not occur is asked as the reference prints it, ('*', 0): the annotation's '*' has one transcript
        # at 0 and another gene's at 1..30
        star = [k for k in range(len(sel)) if cols["bowtieChr"][k] == "*"]
        assert star and {cols["bowtieStart"][k] for k in star} == {"0"} and {t.column()[k] for k in star} == {"1/1"}
        assert ca.format_hits(annotation.hits(["*", "*", "*"], [0, 1, 31])) == ["1/1", "1/2", "0/0"]
    assert len({h for h in hits if h not in ("?/?", "0/0")}) >= 2
