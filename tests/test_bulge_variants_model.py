"""CPU: the model the tests of the bulge search on a variant-aware text take their expected rows from
(tests/bulge_variant_util.py), pinned to the bulge search's model on a text without codes, to the variant search's model
without bulges and to rows written out by hand -- and the plane functions of
crackling_amd/csrc/issl_bulge_variants_text.hpp pinned to character loops through a stand-alone CPU program under
AddressSanitizer + UBSan (tools/bulge_variants_sanitize.cpp)."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import bulge_util as bu
import bulge_variant_util as bvu
import search_util as su
import variant_util as vu
from test_variants_model import random_text, with_codes

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("pattern,span", [("N" * 11 + "GG", (0, 10)), ("TTTV" + "N" * 8, (4, 8))])
def test_clean_text_and_max_variants_0_equal_the_bulge_model(pattern, span):
    rng = np.random.default_rng(len(pattern))
    L = len(pattern)
    clean = random_text(rng, 700)
    coded = with_codes(rng, clean, 30)
    queries = ["N" * L, random_text(rng, L), clean[100:100 + L], su.revcomp(clean[200:200 + L]), random_text(rng, L, "ACGTN")]
    for text, limits in ((coded + "N" + clean[:50], (0,)), (clean + "NN" + clean[:40], (0, 2, L))):
        records = [(b"r0", text[:400].encode()), (b"r1 x", text[400:].encode())]
        off, rows, prof = bu.brute_force(records, pattern, queries, span, 2, 2, 2)
        assert len(rows) > 0 and len(set(rows["bulge"].tolist())) == 5
        for mv in limits:
            v_off, v_rows, v_prof = bvu.brute_force(records, pattern, queries, span, 2, 2, 2, mv)
            assert v_off.tobytes() == off.tobytes() and v_prof.tobytes() == prof.tobytes()
            assert v_rows.tobytes() == bvu.from_bulges(rows, L).tobytes() and not v_rows["n_var"].any()


def test_without_bulges_equals_the_variant_model():
    rng = np.random.default_rng(77)
    pattern, L = "N" * 9 + "RG", 11
    text = with_codes(rng, random_text(rng, 1500), 12)
    records = [(b"r0", text[:700].encode()), (b"r1", (text[700:] + "N" + text[:30]).encode())]
    queries = ["N" * L, random_text(rng, L), text[100:100 + L].translate(str.maketrans("RYSWKMBDHV", "ACGTACGTAC"))]
    for mv in (0, 1, 3):
        off, rows, prof = vu.brute_force(records, pattern, queries, 3, mv)
        assert len(rows) > 0
        b_off, b_rows, b_prof = bvu.brute_force(records, pattern, queries, (1, 7), 3, 0, 0, mv)
        assert b_off.tobytes() == off.tobytes() and b_prof.reshape(prof.shape).tobytes() == prof.tobytes()
        assert b_rows.tobytes() == bvu.from_variants(rows).tobytes() and not b_rows["bulge"].any() and not b_rows["at"].any()
    assert rows["n_var"].max() == 3


# Four records of about ten bases, NGG behind a guide of six, no mismatch allowed.  Query 0 is a guide, query 1 compares nothing.
CODED = [(b"r0", b"GAWCTCATGG"),  # W = A or T: with T the guide binds with one unpaired C; the reference base A gives nothing
         (b"r1", b"GATCATRG"),    # R = A or G: with G the PAM behind an RNA bulge of one base; the reference has TAG
         (b"r2", b"GATSTCATGG"),  # the code is the unpaired base itself: counted in n_var, compared with nothing
         (b"r3", b"ACRTACGGGK")]  # two codes in the ten bases of b = +1, one in the nine of b = 0 and the eight of b = -1
REFERENCE = [(b"r0", b"GAACTCATGG"), (b"r1", b"GATCATAG"), (b"r2", b"GATCTCATGG"), (b"r3", b"ACATACGGGG")]
PATTERN, SPAN, QUERIES = "NNNNNNNGG", (0, 6), ["GATTCANNN", "NNNNNNNNN"]


def test_rows_by_hand():
    off, rows, prof = bvu.brute_force(CODED, PATTERN, QUERIES, SPAN, 0, 1, 1, 2)
    assert rows.dtype.itemsize == 48 and off.tolist() == [0, 3, 16] and not rows["reserved"].any()
    # (query, record, pos, strand, dist, bulge, at, n_var, site, mism)
    assert bvu.as_tuples(rows[:3], 9) == [(0, 0, 0, 0, 0, 1, 3, 1, "GAWCTCATGG", 0),  # an alt allele makes a D1 row
                                          (0, 1, 0, 0, 0, -1, 2, 1, "GATCATRG", 0),   # an alt allele makes the PAM of an R1 row
                                          (0, 2, 0, 0, 0, 1, 3, 1, "GATSTCATGG", 0)]  # a code on the unpaired base
    assert rows["site"][1].tolist() == [0b01010010, 0b00001000, 0b11000001, 0b00100100]
    assert prof[0].tolist() == [[1], [0], [2]]
    # the reference text shows only the third of them, and the plain bulge search skips all three on the coded text
    plain = bu.as_tuples(bu.brute_force(REFERENCE, PATTERN, QUERIES[:1], SPAN, 0, 1, 1)[1], 9)
    assert plain == [(0, 2, 0, 0, 0, 1, 3, "GATCTCATGG", 0)]
    assert len(bu.brute_force(CODED, PATTERN, QUERIES[:1], SPAN, 0, 1, 1)[1]) == 0
    # whichever code the unpaired base is, it counts in n_var and not in dist.  A code that holds T can also pair with the
    # query's T, the T before it being the unpaired base: a tie of break points, and the smaller one is kept
    for code in "RYSWKMBDHV":
        _, one, _ = bvu.brute_force([(b"r2", b"GAT" + code.encode() + b"TCATGG")], PATTERN, QUERIES[:1], SPAN, 0, 1, 0, 2)
        assert [(int(r["bulge"]), int(r["at"]), int(r["dist"]), int(r["n_var"])) for r in one] == [(1, 2 if "T" in su.IUPAC[code] else 3, 0, 1)], code
    # max_variants one below the window's count removes the row of that b only
    at_r3 = lambda rs: [(int(r["pos"]), int(r["bulge"]), int(r["n_var"])) for r in rs if r["query"] == 1 and r["record"] == 3]
    assert at_r3(rows) == [(0, -1, 1), (0, 0, 1), (0, 1, 2), (1, -1, 1), (1, 0, 2), (2, -1, 2)]
    _, fewer, _ = bvu.brute_force(CODED, PATTERN, QUERIES, SPAN, 0, 1, 1, 1)
    assert at_r3(fewer) == [(0, -1, 1), (0, 0, 1), (1, -1, 1)]
    assert bvu.as_tuples(fewer[:3], 9) == bvu.as_tuples(rows[:3], 9)
    assert len(bvu.brute_force(CODED, PATTERN, QUERIES, SPAN, 0, 1, 1, 0)[1]) == 0
    # the lines of the executable
    assert bvu.format_rows(CODED, QUERIES, rows[:3], SPAN) == (b"GAT-TCANNN\tr0\t0\t+\t0\tD1\tGAWCTCATGG\n"
                                                               b"GATTCANNN\tr1\t0\t+\t0\tR1\tGA-TCATRG\n"
                                                               b"GAT-TCANNN\tr2\t0\t+\t0\tD1\tGATSTCATGG\n")
    _, near, _ = bvu.brute_force(CODED[:1], PATTERN, ["GCTTCANNN"], SPAN, 1, 1, 0, 2)
    assert bvu.format_rows(CODED, ["GCTTCANNN"], near, SPAN) == b"GCT-TCANNN\tr0\t0\t+\t1\tD1\tGaWCTCATGG\n"
    assert bvu.format_profile(QUERIES[:1], prof[:1]) == b"GATTCANNN\t1\t0\t2\n"


def test_plane_functions_under_asan_and_ubsan(tmp_path):
    """tools/bulge_variants_sanitize.cpp: the bound, the walk and the row of the header against character loops for every
    L in 2..32, every span start, every b in -3..3, every break point, both strands and windows with 0, 1 and 2 codes; the
    bound is never above the minimum."""
    exe = tmp_path / "bulge_variants_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "bulge_variants_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0 and b"ERROR" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode(errors="replace")[-4000:]
    got = run.stdout.decode().split("\n")[:-1]
    assert re.fullmatch(r"bulge variants ok \d+", got[0]) and int(got[0].split()[-1]) > 100000
    # the sample lines: a D1 row on strand 1 with a code, an R2 row with a mismatch on a code, a row without a bulge
    assert got[1:] == ["CCGTACGTAC-TGCAACGTACNGG\tchr\t1234567890123\t-\t2\tD1\taCGTACGTACRtGCAACGTACGGG",
                       "TTTACGTACGTACTTGCAACGTA\tchr\t1234567890123\t-\t2\tR2\tACgTAcG--yACTTGCAACGTAc",
                       "ATG\t\t1234567890123\t-\t2\t0\tAkG"]
