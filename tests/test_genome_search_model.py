"""CPU: the brute force the genome search tests take their expected rows from (tests/search_util.py), pinned to the
extraction's own brute force (tests/locate_util.py, itself pinned to the reference-made site lists) and to rows written
out by hand."""
import pathlib

import numpy as np
import pytest

import locate_util as lu
import search_util as su

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
EXTRACTION = "VNNNNNNNNNNNNNNNNNNNNRG"  # [ACG][ACGT]{20}[AG]G; its reverse complement is C[CT][ACGT]{20}[TGC]


@pytest.mark.parametrize("fasta", ["extract/multi.fa", "extract/repeat.fa", "bowtie/genome.fa"])
def test_extraction_pattern_gives_the_extraction_matches(fasta):
    """The all-N query under the extraction's forward pattern lists every match of the extraction's two patterns: strand 0
    the forward one, strand 1 the reverse one, whose site -- the reverse complement of the first 20 of the 23 matched
    characters -- is t[3:23]."""
    records = lu.parse([(GOLDEN / fasta).read_bytes()])
    truth = lu.brute_force(records)
    offsets, rows, profile = su.brute_force(records, EXTRACTION, ["N" * 23], 0)
    assert len(truth) > 100 and offsets.tolist() == [0, len(truth)] and profile.tolist() == [[len(truth)]]
    assert np.array_equal(rows["record"], truth["record"]) and np.array_equal(rows["pos"], truth["pos"])
    assert np.array_equal(rows["strand"], truth["strand"])
    assert set(truth["strand"].tolist()) == {0, 1}
    site = np.where(rows["strand"] == 0, rows["site"] & np.uint64((1 << 40) - 1), rows["site"] >> np.uint64(6))
    assert np.array_equal(site, truth["site"])
    assert not rows["dist"].any() and not rows["mism"].any() and not rows["query"].any()


def _rows(seqs, pattern, queries, max_dist):
    records = [(b"r%d" % i, s.upper().encode()) for i, s in enumerate(seqs)]
    offsets, rows, profile = su.brute_force(records, pattern, queries, max_dist)
    assert offsets[0] == 0 and offsets[-1] == len(rows)
    for k in range(len(queries)):
        mine = rows[int(offsets[k]):int(offsets[k + 1])]
        assert (mine["query"] == k).all()
        assert profile[k].tolist() == np.bincount(mine["dist"], minlength=max_dist + 1).tolist()
    return su.as_tuples(rows, len(pattern))


ONE_BASE = {  # (pos, strand, site) of pattern <code>, query N, in the text ACGTN
    "A": [(0, 0, "A"), (3, 1, "A")],
    "C": [(1, 0, "C"), (2, 1, "C")],
    "G": [(1, 1, "G"), (2, 0, "G")],
    "T": [(0, 1, "T"), (3, 0, "T")],
    "R": [(0, 0, "A"), (1, 1, "G"), (2, 0, "G"), (3, 1, "A")],
    "Y": [(0, 1, "T"), (1, 0, "C"), (2, 1, "C"), (3, 0, "T")],
    "S": [(1, 0, "C"), (1, 1, "G"), (2, 0, "G"), (2, 1, "C")],
    "W": [(0, 0, "A"), (0, 1, "T"), (3, 0, "T"), (3, 1, "A")],
    "K": [(0, 1, "T"), (1, 1, "G"), (2, 0, "G"), (3, 0, "T")],
    "M": [(0, 0, "A"), (1, 0, "C"), (2, 1, "C"), (3, 1, "A")],
    "B": [(0, 1, "T"), (1, 0, "C"), (1, 1, "G"), (2, 0, "G"), (2, 1, "C"), (3, 0, "T")],
    "D": [(0, 0, "A"), (0, 1, "T"), (1, 1, "G"), (2, 0, "G"), (3, 0, "T"), (3, 1, "A")],
    "H": [(0, 0, "A"), (0, 1, "T"), (1, 0, "C"), (2, 1, "C"), (3, 0, "T"), (3, 1, "A")],
    "V": [(0, 0, "A"), (1, 0, "C"), (1, 1, "G"), (2, 0, "G"), (2, 1, "C"), (3, 1, "A")],
    "N": [(0, 0, "A"), (0, 1, "T"), (1, 0, "C"), (1, 1, "G"), (2, 0, "G"), (2, 1, "C"), (3, 0, "T"), (3, 1, "A")],
}


@pytest.mark.parametrize("code", sorted(ONE_BASE))
def test_every_iupac_code_at_length_one(code):
    want = [(0, 0, p, s, 0, t) for p, s, t in ONE_BASE[code]]
    assert _rows(["ACGTN"], code, ["N"], 0) == want
    assert _rows(["acgtn"], code.lower(), ["n"], 0) == want


def test_palindromic_window_gives_two_rows_strand_0_first():
    assert _rows(["ACGT"], "NNNN", ["ACGT"], 0) == [(0, 0, 0, 0, 0, "ACGT"), (0, 0, 0, 1, 0, "ACGT")]


def test_no_window_spans_two_records():
    # ACGT would lie across the boundary of AACG | TTAA; the all-N query sees the four window-strands there are
    assert _rows(["AACG", "TTAA"], "NNNN", ["ACGT", "NNNN"], 0) == [
        (1, 0, 0, 0, 0, "AACG"), (1, 0, 0, 1, 0, "CGTT"), (1, 1, 0, 0, 0, "TTAA"), (1, 1, 0, 1, 0, "TTAA")]


def test_a_window_holding_n_is_no_hit():
    assert _rows(["ACNGTA"], "NNN", ["NNN"], 0) == [(0, 0, 3, 0, 0, "GTA"), (0, 0, 3, 1, 0, "TAC")]


def test_lower_case_fasta_is_upper_cased():
    records = lu.parse([b">r\nacgt\n"])
    assert records == [(b"r", b"ACGT")]
    _, rows, _ = su.brute_force(records, "NNNN", ["ACGT"], 0)
    assert su.as_tuples(rows, 4) == [(0, 0, 0, 0, 0, "ACGT"), (0, 0, 0, 1, 0, "ACGT")]


def test_five_prime_pam():
    """Cas12a: TTTV in front of the protospacer.  The text holds TTTA + guide at 2, the reverse complement of TTTC + the
    guide with one mismatch at 28, and TTTT + guide (V excludes T) at 54."""
    guide = "GATTACAGATTACAGATTAC"
    text = "CCTTTAGATTACAGATTACAGATTACGGGTAATCTGAAATCTGTAATCGAAAAATTTTGATTACAGATTACAGATTACC"
    assert text[2:26] == "TTTA" + guide and text[54:78] == "TTTT" + guide
    pattern = "TTTV" + "N" * 20
    assert _rows([text], pattern, ["NNNN" + guide], 0) == [(0, 0, 2, 0, 0, "TTTAGATTACAGATTACAGATTAC")]
    assert _rows([text], pattern, ["NNNN" + guide], 1) == [(0, 0, 2, 0, 0, "TTTAGATTACAGATTACAGATTAC"),
                                                           (0, 0, 28, 1, 1, "TTTCGATTACAGATTtCAGATTAC")]


def test_max_dist_0_1_and_length():
    assert _rows(["ACGTAC"], "NNN", ["ACT"], 0) == []
    assert _rows(["ACGTAC"], "NNN", ["ACT"], 1) == [(0, 0, 0, 0, 1, "ACg"), (0, 0, 1, 1, 1, "ACg")]
    assert _rows(["ACGTAC"], "NNN", ["ACT"], 3) == [
        (0, 0, 0, 0, 1, "ACg"), (0, 0, 0, 1, 2, "cgT"), (0, 0, 1, 0, 2, "cgT"), (0, 0, 1, 1, 1, "ACg"),
        (0, 0, 2, 0, 3, "gta"), (0, 0, 2, 1, 3, "tac"), (0, 0, 3, 0, 3, "tac"), (0, 0, 3, 1, 3, "gta")]


def test_row_fields_and_formatting():
    records = [(b"chr1 test", b"ACGTAC")]
    offsets, rows, profile = su.brute_force(records, "NNN", ["ACT", "NNN"], 1)
    assert rows.dtype.itemsize == 32 and offsets.tolist() == [0, 2, 10] and profile.tolist() == [[0, 2], [8, 0]]
    assert rows["site"][0] == 0 | 1 << 2 | 2 << 4 and rows["mism"][0] == 0b100 and not rows["reserved"].any()
    assert su.format_rows(records, ["ACT", "NNN"], rows[:2]) == b"ACT\tchr1 test\t0\t+\t1\tACg\nACT\tchr1 test\t1\t-\t1\tACg\n"
    assert su.format_profile(["ACT", "NNN"], profile) == b"ACT\t0\t2\nNNN\t8\t0\n"
