"""CPU: the part of the log's entry points (issl_runlog_*, issl_guides_file_counts,
issl_genome_occurrences_paged_events_device) that needs no device: they exist, refuse NULL arguments with ISSL_E_ARG, the
header documents the structures' sizes, and ISSL_ABI_VERSION is still 6 -- only additions were made.  The errors that
need a consensus (ISSL_E_STATE before finish, folds of another consensus, lengths that differ) are in
tests/test_runlog_gpu.py."""
import ctypes as C
import pathlib
import re

import crackling_amd as ca
from crackling_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_runlog_batches", "issl_runlog_info", "issl_runlog_copy", "issl_runlog_close", "issl_guides_file_counts", "issl_guides_files",
           "issl_genome_occurrences_paged_events_device"]


def test_symbols_are_declared_exported_and_bound():
    lib = ca.lib
    for name in SYMBOLS:
        assert f"int {name}(" in HEADER and hasattr(lib, name) and name in _lib.EXPORTS, name
    assert "issl_*" in (ROOT / "crackling_amd" / "csrc" / "libissl_hip.map").read_text()
    assert "issl_runlog.hip" in (ROOT / "Makefile").read_text()


def test_abi_version_is_still_6():
    assert ca.lib.issl_abi_version() == 6 and re.search(r"#define ISSL_ABI_VERSION 6\b", HEADER)


def test_structure_sizes_as_documented():
    assert re.search(r"\} issl_runlog_batch; /\* 112 bytes, no padding \*/", HEADER)
    assert re.search(r"\} issl_guides_file;\s+/\* 16 bytes \*/", HEADER)
    assert ca.BATCH_DTYPE.itemsize == 112 and len(ca.BATCH_DTYPE.names) == 28
    body = HEADER[HEADER.index("typedef struct issl_runlog issl_runlog;"):HEADER.index("} issl_runlog_batch;")]
    declared = re.findall(r"\b([a-z0-9_]+)(?=[,;])", body[body.index("{"):])
    assert tuple(declared) == ca.BATCH_DTYPE.names, "the Python mirror lists the fields in the header's order"


def test_null_arguments():
    lib = ca.lib
    h, fake = C.c_void_p(5), C.c_void_p(8)
    assert lib.issl_runlog_batches(None, None, None, 0, None, None, None, 0, 75.0, b"and", 0, 0, C.byref(h)) == -1 and h.value is None
    assert b"null" in lib.issl_last_error()
    assert lib.issl_runlog_batches(fake, None, None, 0, None, None, None, 0, 75.0, None, 0, 0, C.byref(h)) == -1
    assert lib.issl_runlog_batches(fake, None, None, 0, None, None, None, 0, 75.0, b"and", 0, 0, None) == -1
    n = C.c_uint64(9)
    assert lib.issl_runlog_info(None, C.byref(n), None, None, None) == -1 and n.value == 9
    assert lib.issl_runlog_copy(None, None, 0, None, 0, None, 0) == -1
    assert lib.issl_runlog_close(None) == 0
    out = (C.c_uint32 * 4)()
    assert lib.issl_guides_file_counts(None, 0, out) == -1
    assert lib.issl_guides_files(None, C.byref(n)) == -1 and lib.issl_guides_files(fake, None) == -1
    assert lib.issl_genome_occurrences_paged_events_device(None, None, 0, None, 0, None, None, None) == -1
    assert lib.issl_genome_occurrences_paged_events_device(fake, None, 0, None, 2, None, None, None) == -1
    assert lib.issl_genome_occurrences_paged_events_device(fake, None, 0, fake, 2, None, None, None) == -1
