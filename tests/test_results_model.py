"""CPU: the host model of the result table (tests/results_util.py) pinned byte for byte to the reference's own output files
(tests/golden/results, tools/make_golden_results.py), crackling_amd.read_rnafold_text pinned to their ss columns, and the
part of the C ABI that answers before any device call (issl_results_*, issl_repr_f64_device)."""
import csv
import ctypes as C
import re
import pathlib

import numpy as np
import pytest

import results_util as ru

ROOT = pathlib.Path(__file__).resolve().parent.parent
RUNS = ru.golden_runs()
IDS = [r["name"] for r in RUNS]
SYMBOLS = ["issl_results_build", "issl_results_info", "issl_results_times", "issl_results_device", "issl_results_copy", "issl_results_write",
           "issl_results_close", "issl_repr_f64_device"]


def test_the_runs_the_recipe_keeps():
    assert IDS == ["ultralow_page0", "ultralow_page7", "medium_page0", "medium_page7", "high_page0", "high_page7", "noscore",
                   "headers"]
    assert not (ru.GOLDEN / "tab.txt.gz").exists()  # the reference cannot write that file (tools/make_golden_results.py)
    seen = {c: set() for c in ru.ORDER}
    for run in RUNS:
        rows = list(csv.reader(ru.golden_bytes(run["name"]).decode().splitlines(keepends=True), delimiter=run["delimiter"]))
        assert rows[0] == ru.ORDER and all(len(r) == 26 for r in rows)
        for r in rows[1:]:
            for c, v in zip(ru.ORDER, r):
                seen[c].add(v)
    for c in ("passedG20", "passedTTTT", "passedATPercent", "acceptedByMm10db", "acceptedBySgRnaScorer", "passedAvoidLeadingT",
              "passedBowtie", "passedOffTargetScore"):
        assert seen[c] == {"0", "1", "?"}, c
    assert seen["passedSecondaryStructure"] == {"0", "1", "?", "!"} and seen["isUnique"] == {"0", "1"}
    assert {"", "?"} < seen["ssEnergy"] and {"*", "?"} < seen["bowtieChr"] and "-1.0" in seen["cfdOfftargetscore"]
    assert any('"' in h for h in seen["header"]) and any("," in h for h in seen["header"]) and any(h.startswith(" ") for h in seen["header"])


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_model_writes_the_reference_file(run):
    got, offsets = ru.model_table(**ru.host_stages(run, ru.golden_fold_text(run)))
    want = ru.golden_bytes(run["name"])
    assert got == want
    lines = want.splitlines(keepends=True)  # (no field of these files holds a line end)
    assert offsets.tolist() == np.cumsum([len(x) for x in lines]).tolist()


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_read_rnafold_text_gives_the_ss_columns(run):
    import crackling_amd as ca
    rows = list(csv.DictReader(ru.golden_bytes(run["name"]).decode().splitlines(keepends=True), delimiter=run["delimiter"]))
    folded = [r for r in rows if r["ssL1"] != "?"]
    assert len(folded) > 20 or run["name"] == "noscore"
    got = ca.read_rnafold_text(ru.golden_fold_text(run), [r["seq"] for r in rows])
    for r, g in zip(rows, got):
        if r["ssL1"] != "?":
            assert g == (r["ssL1"], r["ssStructure"], r["ssEnergy"])
    assert got == ru.read_rnafold_text(ru.golden_fold_text(run), [r["seq"] for r in rows])
    assert any(g is not None and g[2] == "" for g in got)


def test_read_rnafold_text_rules():
    import crackling_amd as ca
    g = ["ACGTACGTACGTACGTACGTAGG", "TCGTACGTACGTACGTACGTAGG", "AAAAACGTACGTACGTACGTAGG"]
    text = "GCGUACGUACGUACGUACGUxyz\n.(.) (-1.50)\nGCGUACGUACGUACGUACGUxyz  \n... ( -2.00) \nunpaired"
    assert ca.read_rnafold_text(text, g) == [("GCGUACGUACGUACGUACGUxyz", "...", ""), ("GCGUACGUACGUACGUACGUxyz", "...", ""), None]
    assert ca.read_rnafold_text(text, [x[:20] for x in g]) == ca.read_rnafold_text(text, g)
    assert ca.read_rnafold_text("GCGUACGUACGUACGUACGU\n.... x(-1.50)y z\n", g[:1]) == [("GCGUACGUACGUACGUACGU", "....", "(-1.50)")]
    with pytest.raises(ValueError):
        ca.read_rnafold_text("GCGUACGUACGUACGUACGU\n....(-1.50)\n", g[:1])
    assert ca.read_rnafold_text("", g) == [None, None, None]


def test_eight_names_are_declared_exported_and_bound():
    import crackling_amd as ca
    from crackling_amd import _lib
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTS, name
    for name in ("issl_results", "issl_text_span", "issl_results_config"):
        assert re.search(r"^(typedef struct %s |\} )%s;" % (name, name), header, re.M), name
    assert C.sizeof(_lib.TextSpan) == 16 and ca.results.TEXT_SPAN_DTYPE.itemsize == 16
    assert [ca.results.TEXT_SPAN_DTYPE.fields[n][1] for n in ("offset", "length", "reserved")] == [0, 8, 12]
    for name in ("ResultTable", "read_rnafold_text", "repr_f64", "pipeline"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert callable(ca.pipeline.run) and tuple(ru.ORDER) == ca.results.COLUMNS and tuple(ru.DELIMITERS) == ca.results.DELIMITERS
    assert "ISSL_RESULTS_DIRECT = 1" in header and ca.results.DIRECT == 1


def test_argument_errors_come_before_any_device_call():
    from crackling_amd import _lib
    lib = _lib.lib
    cfg = _lib.ResultsConfig(b",", 0, b"and", 75.0)
    fake = C.c_void_p(0x1000)  # never read: every call below fails on an argument ahead of it
    h = C.c_void_p(0x1234)
    args = (None, 0, None, 0, None, 0, None, None, None, None, 0)
    assert lib.issl_results_build(None, fake, *args, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    assert b"null" in lib.issl_last_error()
    assert lib.issl_results_build(fake, None, *args, C.byref(cfg), C.byref(h)) == -1
    assert lib.issl_results_build(fake, fake, *args, None, C.byref(h)) == -1
    assert lib.issl_results_build(fake, fake, *args, C.byref(cfg), None) == -1
    assert lib.issl_results_build(fake, fake, *args, C.byref(_lib.ResultsConfig(b",", 0, None, 75.0)), C.byref(h)) == -1
    for bad in (b"\x00", b"\n", b'"', b"a", b"0", b".", b"-", b"?", b":"):
        h = C.c_void_p(0x1234)
        assert lib.issl_results_build(fake, fake, *args, C.byref(_lib.ResultsConfig(bad, 0, b"and", 75.0)), C.byref(h)) == -4, bad
        assert h.value is None and b"delimiter" in lib.issl_last_error()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.issl_results_info(None, C.byref(a), C.byref(b), C.byref(c)) == -1
    assert lib.issl_results_times(None, None, None, None) == -1
    p, q = C.c_void_p(), C.c_void_p()
    assert lib.issl_results_device(None, C.byref(p), C.byref(q)) == -1
    buf = C.create_string_buffer(8)
    assert lib.issl_results_copy(None, buf, 8) == -1
    assert lib.issl_results_write(None, b"/nonexistent/x", 0) == -1
    assert lib.issl_results_close(None) == 0
    assert lib.issl_repr_f64_device(None, 3, fake, fake, None) == -1
    assert lib.issl_repr_f64_device(fake, 3, None, fake, None) == -1
    assert lib.issl_repr_f64_device(fake, 3, fake, None, None) == -1
    assert lib.issl_repr_f64_device(None, 0, None, None, None) == 0


def test_host_text_code_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/results_sanitize.cpp: the quoting, the span checks and the number formatting shared with the kernels, as a
    stand-alone CPU program."""
    import subprocess
    exe = tmp_path / "results_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "results_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
