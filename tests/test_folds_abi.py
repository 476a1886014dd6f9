"""CPU: the part of RNAfold's exchange (issl_folds_*, issl_consensus_finish_folds, issl_results_build_rows_folds) that
answers before any device call: the names are declared in include/issl_hip.h, exported, bound in _lib.py, and NULL
arguments are ISSL_E_ARG."""
import ctypes as C
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_folds_open", "issl_folds_info", "issl_folds_times", "issl_folds_input", "issl_folds_input_copy", "issl_folds_input_write",
           "issl_folds_read", "issl_folds_read_file", "issl_folds_device", "issl_folds_text_device", "issl_folds_copy",
           "issl_folds_text_copy", "issl_folds_close", "issl_consensus_finish_folds", "issl_results_build_rows_folds"]


def test_names_are_declared_exported_and_bound():
    import crackling_amd as ca
    from crackling_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert f"int {name}(" in HEADER and hasattr(lib, name) and name in _lib.EXPORTS, name
    assert re.search(r"^typedef struct issl_folds issl_folds;", HEADER, re.M)
    assert "#define ISSL_ABI_VERSION 6" in HEADER and _lib.lib.issl_abi_version() == 6
    version = (ROOT / "crackling_amd" / "csrc" / "libissl_hip.map").read_text()
    assert "issl_*" in version and "local: *" in version
    assert "Folds" in ca.__all__ and callable(ca.Consensus.folds)
    for name in ("input", "write_input", "read", "read_file", "texts", "folds", "n_read"):
        assert hasattr(ca.Folds, name), name
    assert "Crackling.py:406-497" in HEADER and "211 bytes per" in HEADER
    for src in ("issl_folds.hip", "issl_folds.cpp"):
        assert src in (ROOT / "Makefile").read_text() and (ROOT / "crackling_amd" / "csrc" / src).exists()
    assert "rnafold_reader" in ca.pipeline.batches.__doc__


def test_null_arguments_come_back_before_any_device_call():
    from crackling_amd import _lib
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never read: every call below fails on an argument ahead of it
    h = C.c_void_p(0x1234)
    assert lib.issl_folds_open(None, C.byref(h)) == -1 and h.value is None and b"null" in lib.issl_last_error()
    assert lib.issl_folds_open(fake, None) == -1
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.issl_folds_info(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == -1
    assert lib.issl_folds_times(None, None, None) == -1
    p, n = C.c_void_p(0x1234), C.c_uint64(7)
    assert lib.issl_folds_input(None, 0, 0, C.byref(p), C.byref(n)) == -1 and p.value is None and n.value == 0
    assert lib.issl_folds_input(fake, 0, 0, None, C.byref(n)) == -1
    assert lib.issl_folds_input(fake, 0, 0, C.byref(p), None) == -1
    buf = C.create_string_buffer(8)
    assert lib.issl_folds_input_copy(None, 0, 0, buf, 8) == -1
    assert lib.issl_folds_input_write(None, 0, 0, b"/nonexistent/x") == -1
    assert lib.issl_folds_input_write(fake, 0, 0, None) == -1
    assert lib.issl_folds_read(None, 0, 0, b"x", 1) == -1
    assert lib.issl_folds_read(fake, 0, 0, None, 1) == -1
    assert lib.issl_folds_read_file(None, 0, 0, b"/nonexistent/x") == -1
    assert lib.issl_folds_read_file(fake, 0, 0, None) == -1
    q = C.c_void_p()
    assert lib.issl_folds_device(None, C.byref(p), C.byref(q)) == -1
    assert lib.issl_folds_device(fake, None, C.byref(q)) == -1 and lib.issl_folds_device(fake, C.byref(p), None) == -1
    assert lib.issl_folds_text_device(None, C.byref(p), C.byref(n)) == -1
    assert lib.issl_folds_copy(None, None, None, 0) == -1
    size = C.c_size_t(5)
    assert lib.issl_folds_text_copy(None, 0, 0, buf, 8, C.byref(size)) == -1 and size.value == 0
    assert lib.issl_folds_text_copy(fake, 0, 0, buf, 8, None) == -1
    assert lib.issl_folds_text_copy(fake, 0, 3, buf, 8, C.byref(size)) == -1
    assert lib.issl_folds_text_copy(fake, 0, -1, buf, 8, C.byref(size)) == -1
    assert lib.issl_folds_close(None) == 0
    assert lib.issl_consensus_finish_folds(None, fake) == -1 and lib.issl_consensus_finish_folds(fake, None) == -1
    cfg = _lib.ResultsConfig(b",", 0, b"and", 75.0)
    rest = (None, 0, None, None, None, None, 0, 0, 0)
    h = C.c_void_p(0x1234)
    assert lib.issl_results_build_rows_folds(fake, fake, None, *rest, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    assert lib.issl_results_build_rows_folds(None, fake, fake, *rest, C.byref(cfg), C.byref(h)) == -1
    assert lib.issl_results_build_rows_folds(fake, None, fake, *rest, C.byref(cfg), C.byref(h)) == -1
    assert lib.issl_results_build_rows_folds(fake, fake, fake, *rest, None, C.byref(h)) == -1
    assert lib.issl_results_build_rows_folds(fake, fake, fake, *rest, C.byref(cfg), None) == -1
    assert lib.issl_results_build_rows_folds(fake, fake, fake, *rest, C.byref(_lib.ResultsConfig(b"x", 0, b"and", 75.0)), C.byref(h)) == -4
