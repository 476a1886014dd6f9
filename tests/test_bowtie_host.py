"""CPU: the host side of the Bowtie step (crackling_amd.bowtie, issl_genome_occurrences*) against the reference's own run
with a brute-force stand-in for Bowtie2 (tests/golden/bowtie, tools/make_golden_bowtie.py), and the model the GPU tests
take their expected rows from (tests/bowtie_util.py), pinned to that run."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import bowtie_util as bu

ROOT = pathlib.Path(__file__).resolve().parent.parent
CONFIGS = bu.golden_configs()
IDS = [c["name"] for c in CONFIGS]


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _names():
    return [n for n, _ in bu.golden_model().records]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_read_bowtie_output_gives_the_reference_columns(cfg):
    rows = bu.golden_rows(cfg["name"])
    sel = bu.golden_selection(cfg, rows)
    guides = [rows[k]["seq"] for k in sel]
    sam = bu.golden_sam(cfg["name"])
    assert len(sam.splitlines()) == 8 * len(sel)
    got = ca.read_bowtie_output(sam, guides, [n.split()[0] for n in _names()], cfg["page_length"])
    assert got.dtype == ca.OCCURRENCE_DTYPE
    assert ca.format_columns(got, _names()) == bu.golden_columns(rows, sel)
    # every guide outside the selection is untested in the CSV
    rest = sorted(set(range(len(rows))) - set(sel))
    assert all(rows[k][c] == "?" for k in rest for c in ("passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd"))
    assert (got["code"] == 2).any() == (cfg["page_length"] == 0) and (got["code"] == 0).any() and (got["code"] == 1).any()
    assert ((got["code"] == 1) & (got["record"] == 0xFFFFFFFF)).any() and ((got["code"] == 1) & (got["record"] != 0xFFFFFFFF)).any()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_bowtie_input_is_what_the_reference_wrote(cfg):
    rows = bu.golden_rows(cfg["name"])
    guides = [rows[k]["seq"] for k in bu.golden_selection(cfg, rows)]
    reads = []
    for line in bu.golden_sam(cfg["name"]).splitlines():
        f = line.split("\t")
        reads.append(bu.rc(f[9]) if int(f[1]) & 16 else f[9])
    assert ca.bowtie_input(guides) == "".join(r + "\n" for r in reads)
    assert ca.bowtie_input([]) == "" and ca.BOWTIE_PAMS == bu.PAMS


def test_read_bowtie_output_as_written():
    a, b = "ACGTACGTACGTACGTACGTAGG", "ACGTACGTACGTACGTACGTCGG"  # one 20-mer
    c = "TTGCATGCATGCATGCATGCAGG"
    hit = "0\t0\tchr1\t11\t42\t23M\t*\t0\t0\t{}\tI\tAS:i:0\tXM:i:0\tYT:Z:UU"
    rev = "0\t16\tchr2\t5\t1\t23M\t*\t0\t0\t{}\tI\tAS:i:0\tXS:i:0\tXM:i:0\tYT:Z:UU"
    miss = "0\t4\t*\t0\t0\t*\t*\t0\t0\t{}\tI\tYT:Z:UU"

    def sam(g, first, fourth=miss):
        reads = [g[:20] + p for p in ca.BOWTIE_PAMS]
        return "".join((first if v == 0 else fourth if v == 3 else miss).format(bu.rc(r) if (first if v == 0 else fourth) is rev and v in (0, 3) else r) + "\n"
                       for v, r in enumerate(reads))

    text = sam(a, hit) + sam(b, hit) + sam(c, rev)
    got = ca.read_bowtie_output(text, [a, b, c], ["chr1", "chr2"])
    assert got["code"].tolist() == [2, 1, 0] and got["owner"].tolist() == [0, 1, 1]
    assert got["nb"].tolist() == [1, 1, 2] and got["aligned"].tolist() == [1, 1, 1] and got["repeated"].tolist() == [0, 0, 1]
    assert got["record"].tolist() == [0, 0, 1] and got["pos"].tolist() == [10, 10, 4] and got["strand"].tolist() == [0, 0, 1]
    assert got["source"].tolist() == [0xFFFFFFFF, 1, 2]
    assert ca.format_columns(got, ["chr1 x", "chr2"]) == {"passedBowtie": ["?", "1", "0"], "bowtieChr": ["?", "chr1", "chr2"],
                                                          "bowtieStart": ["?", "11", "5"], "bowtieEnd": ["?", "33", "27"]}
    # pages of one: both guides of the 20-mer are tested; an unknown name is no record
    got = ca.read_bowtie_output(text, [a, b, c], ["chr1"], page_length=1)
    assert got["code"].tolist() == [1, 1, 0] and got["record"].tolist() == [0, 0, 0xFFFFFFFF] and got["pos"].tolist() == [10, 10, 0]
    assert ca.format_columns(got, ["chr1"])["bowtieEnd"] == ["33", "33", "22"]
    # the tags are looked for in the whole line, and a second variant counts
    got = ca.read_bowtie_output(sam(c, miss, hit), [c], ["chr1"])
    assert got["nb"].tolist() == [1] and got["aligned"].tolist() == [8] and got["code"].tolist() == [1] and got["record"].tolist() == [0xFFFFFFFF]
    with pytest.raises(ValueError):
        ca.read_bowtie_output(text, [a, b], ["chr1"])
    with pytest.raises(ValueError):
        ca.read_bowtie_output(sam(c, hit), [a], ["chr1"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_model_agrees_with_the_reference(cfg):
    """nb, code and the first occurrence of the model's rows are what the CSV and the recorded SAM say."""
    m = bu.golden_model()
    assert len(m.records) >= 3 and any(len(s) < 23 for _, s in m.records)
    rows = bu.golden_rows(cfg["name"])
    sel = bu.golden_selection(cfg, rows)
    guides = [rows[k]["seq"] for k in sel]
    sigs = np.array([bu.sig(g[:20]) for g in guides], dtype=np.uint64)
    assert np.array_equal(sigs, ca.encode_guides([g[:20] for g in guides]))
    got = m.rows(sigs, cfg["page_length"])
    bu.same_rows(got, m.rows_slow([g[:20] for g in guides], cfg["page_length"]))
    assert ca.format_columns(got, _names()) == bu.golden_columns(rows, sel)
    sam = ca.read_bowtie_output(bu.golden_sam(cfg["name"]), guides, [n.split()[0] for n in _names()],
                                cfg["page_length"])
    bu.same_rows(got, sam, [f for f in bu.FIELDS if f != "n_perfect"])
    assert (got["n_perfect"] >= sam["aligned"].astype(bool)).all()
    if cfg["page_length"] == 0:  # the reference's look-up by printed sequence: a group that names another guide's 20-mer
        other = [k for k in range(len(sel)) if got["owner"][k] and guides[got["source"][k]][:20] != guides[k][:20]]
        assert other and all(guides[k].startswith("CCT") and bu.rc(guides[got["source"][k]][3:20]) == guides[k][3:20] for k in other)


@pytest.mark.parametrize("page_length", [0, 1, 5, 1 << 30])
def test_model_fast_and_slow_agree_on_adversarial_text(page_length):
    """The rows the GPU is compared with (Model.rows, numpy) against the line-by-line restatement of the reference."""
    _, model, planted, sigs = bu.adversarial()
    assert 2000 < sum(len(s) for _, s in model.records) < 3500 and len(sigs) > 8000
    fast = model.rows(sigs, page_length)
    bu.same_rows(fast, model.rows_slow([bu.unsig(x) for x in sigs], page_length))
    assert (fast["owner"] == 1).all() == (page_length == 1)
    k = np.nonzero(sigs == bu.sig(planted["both"][:20]))[0]
    if page_length in (0, 1 << 30):  # one page: the guide on strand 0 of the CCT ... AGG window takes the verdict of the one on strand 1
        assert (sigs[fast["source"][k[-1]]] == bu.sig(bu.rc(planted["both"])[:20])) and fast["strand"][k[-1]] == 1
    assert {0, 1, 2} <= set(fast["nb"].tolist()) and (fast["n_perfect"] > 8).any() and (fast["repeated"] != 0).any()


def test_symbols_layout_and_arguments():
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("issl_genome_occurrences", "issl_genome_occurrences_device"):
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTS, name
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_occurrence;", header)
    fields = re.findall(r"(uint\d+_t)\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert [f[1] for f in fields] == list(ca.OCCURRENCE_DTYPE.names) == list(bu.DTYPE.names)
    sizes = [int(f[0][4:-2]) // 8 * int(f[2] or 1) for f in fields]
    assert sum(sizes) == ca.OCCURRENCE_DTYPE.itemsize == 32
    assert [ca.OCCURRENCE_DTYPE.fields[f[1]][1] for f in fields] == [sum(sizes[:k]) for k in range(len(sizes))]  # no holes
    assert ca.OCCURRENCE_DTYPE == bu.DTYPE
    sites = (C.c_uint64 * 1)(0)
    rows = (C.c_uint8 * 32)()
    assert _lib.lib.issl_genome_occurrences(None, sites, 1, 0, rows) == -1 and _lib.lib.issl_last_error()
    assert _lib.lib.issl_genome_occurrences(None, sites, 0, 0, rows) == -1
    assert _lib.lib.issl_genome_occurrences_device(None, sites, 1, 0, rows, None) == -1
    assert bytes(rows) == bytes(32)


def test_without_a_device_there_is_no_answer():
    """A genome handle needs a device (no CPU fallback), so without one the step cannot be reached."""
    if _has_gpu():
        return
    with pytest.raises(ca.IsslError) as e:
        ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    assert e.value.code == -5 and e.value.message
