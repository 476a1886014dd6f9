"""CPU: the model of tests/transcripts_util.py against the reference's own answers (tests/golden/transcripts, recorded by
tools/make_golden_transcripts.py), format_hits, and the executable's refusal to answer without a device."""
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
import transcripts_util as tu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "countHitTranscripts")
CASES = tu.cases()
IDS = [c["name"] for c in CASES]


def test_the_cases_the_issue_names_are_there():
    names = set(IDS)
    assert len(CASES) >= 40 and sum(1 for c in CASES if c.get("error")) >= 10
    assert {"sample", "dotted_names", "gene_lines", "two_genes", "crlf", "cr_only", "csv_quoting", "nothing_counted"} <= names
    assert sum(1 for n in names if n.startswith("bowtie_")) == 6
    assert (tu.GOLDEN / "sample" / "expected.csv").read_text().splitlines()[1:] == [
        "AAAA,Chr1,60,83,2/4", "AAAT,Chr1,200,223,2/4", "AATA,Chr1,320,343,4/4", "ATAA,Chr1,460,483,0/0"]
    assert not list(tu.GOLDEN.rglob("*.p"))           # the reference's pickle stays out of the tree


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_reproduces_the_reference(case):
    gff, crackling = case["annotation"].read_bytes(), case["crackling"].read_bytes()
    if case.get("error"):
        assert not case.get("expected")
        with pytest.raises(tu.FormatError):
            tu.process(gff, crackling)
    else:
        assert tu.process(gff, crackling) == case["expected"].read_bytes()


def test_golden_answers_cover_the_quirks():
    """The fixtures show what the issue calls easy to get wrong: 2/1, '?/?' for two genes and for a first transcript
    without an mRNA line, 0/0 for '*' and for dotted query names."""
    def hits(name):
        return [ln.rsplit(",", 1)[1] for ln in (tu.GOLDEN / name / "expected.csv").read_text().splitlines()[1:]]
    assert hits("exon_without_mrna_later") == ["1/1", "2/1", "?/?", "0/0"]
    assert "?/?" in hits("exon_without_mrna_first") and "?/?" in hits("two_genes")
    assert hits("dotted_names") == ["0/0", "1/1", "1/1", "0/0", "0/0"]
    assert set(hits("nothing_counted")) == {"0/0"}
    assert hits("only_unmapped") == ["?/?", "?/?", "0/0"]


def test_format_hits():
    rows = np.array([(0, 0, 0, tu.NONE), (2, 4, 0, 1), (2, 1, 0, 0), (0, 0, 1, tu.NONE), (3, 0, 2, 5), (1, 0, 3, 7)],
                    dtype=ca.TRANSCRIPT_HITS_DTYPE)
    assert ca.format_hits(rows) == ["0/0", "2/4", "2/1", "?/?", "?/?", "?/?"]
    assert ca.format_hits(rows[:0]) == []
    assert ca.TRANSCRIPT_HITS_DTYPE == tu.DTYPE and ca.TRANSCRIPT_HITS_DTYPE.itemsize == 16
    assert [tu.hits_text(tuple(r)) for r in rows.tolist()] == ca.format_hits(rows)


def test_model_integers():
    assert tu.to_int(b"+12") == 12 and tu.to_int("-0") == 0 and tu.to_int(str((1 << 63) - 1)) == (1 << 63) - 1
    for bad in ("", "+", "1_0", " 1", "1.0", "1e3", str(1 << 63), "١"):
        with pytest.raises(tu.FormatError):
            tu.to_int(bad)


def test_executable_needs_a_device(tmp_path):
    """Without a GPU the executable exits 1 with the library's ISSL_E_DEVICE message and writes nothing (with one it
    answers: tests/test_transcripts_gpu.py compares every case).  A malformed annotation is refused for its format either way."""
    import torch
    case = next(c for c in CASES if c["name"] == "sample")
    out = tmp_path / "out.csv"
    r = subprocess.run([EXE, "-a", str(case["annotation"]), "-c", str(case["crackling"]), "-o", str(out)], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0 and out.read_bytes() == case["expected"].read_bytes()
        out.unlink()
    else:
        blob = case["annotation"].read_bytes()
        h = ca._lib.C.c_void_p()
        assert ca.lib.issl_annotation_open(blob, len(blob), 0, ca._lib.C.byref(h)) == -5
        message = ca.lib.issl_last_error().decode()
        assert r.returncode == 1 and r.stdout == "" and message and message in r.stderr and not out.exists()
    bad = next(c for c in CASES if c["name"] == "error_attribute_without_equals")
    r = subprocess.run([EXE, "-a", str(bad["annotation"]), "-c", str(bad["crackling"]), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 1 and "has no '='" in r.stderr and not out.exists()
    r = subprocess.run([EXE, "-a", str(case["annotation"])], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr
