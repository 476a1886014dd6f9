"""CPU: the numpy model of the efficiency consensus (consensus_util.Model) against the reference's own rows for every
golden configuration (tests/golden/consensus, recipe: tools/make_golden_consensus.py), the reading of RNAfold's output,
and the argument errors of issl_consensus_* that need no device.  test_consensus.py holds the GPU side."""
import ctypes as C

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import consensus_util as cu

CONFIGS = cu.golden_configs()
SYMBOLS = ["issl_consensus_begin", "issl_consensus_fold_list", "issl_consensus_fold_copy", "issl_consensus_finish",
           "issl_consensus_copy", "issl_consensus_device", "issl_consensus_close"]


def test_golden_set_has_the_nine_configurations():
    assert [c["name"] for c in CONFIGS] == ["ultralow", "low", "medium", "high", "high_n1", "high_n3", "high_no_mm10db",
                                            "ultralow_no_mm10db", "medium_no_sgrnascorer2"]
    sv, coef, _ = cu.golden_model()
    assert sv.shape == (215, 80) and sv.dtype == np.uint8 and coef.shape == (215,) and set(np.unique(sv)) == {0, 1}


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c["name"] for c in CONFIGS])
def test_model_reproduces_the_reference(cfg):
    want = cu.golden_rows(cfg["name"])
    guides = [w["seq"] for w in want]
    seen = [1 if w["isUnique"] == "1" else 2 for w in want]
    m = cu.Model(guides, seen, **cu.golden_keywords(cfg))
    folded = [j for j, w in enumerate(want) if w["ssEnergy"] != "?"]  # the reference fills ssEnergy for every line it folded
    assert m.fold_rows.tolist() == folded
    if not cfg["mm10db"]:
        assert len(m.fold_rows) == 0
    text = cu.fold_text()
    if cfg["name"] == "ultralow":  # fold.txt is what RNAfold's stand-in printed for this list, in order
        assert ["G" + guides[j][1:20] + ca.SCAFFOLD for j in m.fold_rows] == text.splitlines()[0::2]
    folds = ca.read_rnafold_output(text, [guides[j] for j in m.fold_rows])
    assert folds["present"].all()
    m.finish(folds)
    cu.compare_with_reference(m.rows, guides, seen, want, cu.fold_energies(text))
    # the selection: what the reference's filter for the specificity stage yields with passedBowtie untested
    if cfg["optimisation"] == "ultralow":
        expect = list(range(len(want)))
    elif cfg["optimisation"] == "low":
        expect = [j for j, w in enumerate(want) if w["isUnique"] == "1"]
    else:
        expect = [j for j, w in enumerate(want) if w["isUnique"] == "1" and int(w["consensusCount"]) >= cfg["n"]]
    assert m.selected.tolist() == expect


def test_scores_equal_the_reference_bit_for_bit():
    want = cu.golden_rows("ultralow")
    scores = cu.sgrna_scores([w["seq"] for w in want], *cu.golden_model())
    assert [repr(float(s)) for s in scores] == [repr(float(w["sgrnascorer2score"])) for w in want]
    assert (scores < 0).any() and (scores > 0).any()


# ---- read_rnafold_output ---------------------------------------------------------------------------------------------

FIXED = "." * 28 + "((((....))))...))))" + "." * 21 + "((((....))))(((((((...)))))))..."
A, B, T = "ACGTACGTACGTACGTACGTAGG", "CCGTACGTACGTACGTACGTTGG", "TTGCATGCATGCATGCATGCAGG"


def rna(guide):
    return "G" + guide[1:20].replace("T", "U") + ca.SCAFFOLD


def test_read_rnafold_output_padded_energy_and_scaffold():
    text = rna(A) + "\n" + FIXED + " ( -5.30)\n" + rna(T) + "\n" + "." * 100 + " (-18.00)\n"
    f = ca.read_rnafold_output(text, [A, T, "GGGGGGGGGGGGGGGGGGGGAGG"])
    assert f.dtype == ca.FOLD_DTYPE and f.dtype.itemsize == 16
    assert f.tolist() == [(-5.3, 1, 1), (-18.0, 0, 1), (0.0, 0, 0)]
    assert ca.read_rnafold_output("", [A]).tolist() == [(0.0, 0, 0)]
    assert len(ca.read_rnafold_output(text, [])) == 0


def test_read_rnafold_output_last_pair_of_a_key_wins():
    # A and B share characters [1:20]: one key, the later pair replaces the earlier one for both
    assert A[1:20] == B[1:20]
    text = rna(A) + "\n" + FIXED + " (-35.00)\n" + rna(B) + "\n" + "." * 100 + " (-10.00)\n"
    assert ca.read_rnafold_output(text, [A, B]).tolist() == [(-10.0, 0, 1), (-10.0, 0, 1)]


def test_read_rnafold_output_odd_number_of_lines():
    text = rna(A) + "\n" + FIXED + " (-29.90)\n" + rna(T) + "\n"
    assert ca.read_rnafold_output(text, [A, T]).tolist() == [(-29.9, 1, 1), (0.0, 0, 0)]
    # a structure that differs in one fixed character is not the scaffold's
    text = rna(A) + "\n" + FIXED[:30] + "." + FIXED[31:] + " (-29.90)\n"
    assert ca.read_rnafold_output(text, [A]).tolist() == [(-29.9, 0, 1)]


# ---- the C ABI without a device --------------------------------------------------------------------------------------

def test_consensus_symbols_and_layouts():
    header = (cu.GOLDEN.parents[2] / "include" / "issl_hip.h").read_text()
    for name in SYMBOLS:
        assert f"int {name}(" in header and hasattr(_lib.lib, name) and name in _lib.EXPORTS, name
    assert "#define ISSL_ABI_VERSION 6" in header and _lib.lib.issl_abi_version() == 6
    assert ca.CONSENSUS_DTYPE.itemsize == 32 and ca.CONSENSUS_DTYPE == cu.ROW_DTYPE
    assert [ca.CONSENSUS_DTYPE.fields[f][1] for f in ("sgrna_score", "at", "ss_energy", "g20", "count")] == [0, 8, 16, 24, 31]
    assert C.sizeof(_lib.ConsensusConfig) == 72
    assert len(ca.SCAFFOLD) == 80 and set(ca.SCAFFOLD) == set("ACGU")


def test_consensus_null_arguments():
    lib = _lib.lib
    h, p, q, n = C.c_void_p(1), C.c_void_p(), C.c_void_p(), C.c_uint64()
    cfg = _lib.ConsensusConfig()
    assert lib.issl_consensus_begin(None, C.byref(cfg), C.byref(h)) == -1 and h.value is None  # *out is not left dangling
    assert b"null" in lib.issl_last_error()
    assert lib.issl_consensus_begin(None, None, C.byref(h)) == -1
    assert lib.issl_consensus_begin(None, C.byref(cfg), None) == -1
    assert lib.issl_consensus_fold_list(None, C.byref(p), C.byref(n)) == -1
    assert lib.issl_consensus_fold_copy(None, None, 0) == -1
    assert lib.issl_consensus_finish(None, None, 0) == -1
    assert lib.issl_consensus_copy(None, None, 0) == -1
    assert lib.issl_consensus_device(None, C.byref(p), C.byref(q), C.byref(n)) == -1
    assert lib.issl_consensus_close(None) == 0  # as issl_guides_close
