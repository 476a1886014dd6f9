"""CPU: the C ABI of the transcript hit counts (include/issl_hip.h, issl_annotation_*): declarations, sizes, argument
checks, and the order of errors -- a malformed annotation is ISSL_E_FORMAT before any device is asked for."""
import ctypes as C
import pathlib
import re

import pytest

import crackling_amd as ca
from crackling_amd import _lib
import transcripts_util as tu

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
CALLS = ("issl_annotation_open", "issl_annotation_open_file", "issl_annotation_info", "issl_annotation_seq", "issl_annotation_lookup",
         "issl_annotation_hits", "issl_annotation_hits_device", "issl_annotation_hits_occurrences_device", "issl_annotation_close")
E_ARG, E_IO, E_FORMAT, E_DEVICE = -1, -2, -3, -5
ANNOTATIONS = sorted({c["annotation"] for c in tu.cases()})
MALFORMED = {c["annotation"] for c in tu.cases() if c.get("error") and c["name"].startswith(("error_attribute", "error_trailing", "error_empty", "error_exon"))}


def has_gpu():
    import torch
    return torch.cuda.is_available()


def test_header_declares_the_calls():
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, HEADER) and hasattr(_lib.lib, name) and name in _lib.EXPORTS, name
    assert "#define ISSL_ABI_VERSION 6" in HEADER and _lib.lib.issl_abi_version() == 6
    assert "typedef struct { uint32_t hit, total, status, first; } issl_transcript_hits;" in HEADER
    assert ca.TRANSCRIPT_HITS_DTYPE.itemsize == 16 and ca.TRANSCRIPT_HITS_DTYPE.names == ("hit", "total", "status", "first")
    assert all(ca.TRANSCRIPT_HITS_DTYPE.fields[n][1] == 4 * k for k, n in enumerate(ca.TRANSCRIPT_HITS_DTYPE.names))
    assert len(MALFORMED) == 5


def test_null_arguments():
    lib = _lib.lib
    h = C.c_void_p(0x1234)
    assert lib.issl_annotation_open(None, 5, 0, C.byref(h)) == E_ARG and h.value is None
    assert lib.issl_annotation_open(b"x", 1, 0, None) == E_ARG
    h = C.c_void_p(0x1234)
    assert lib.issl_annotation_open_file(None, 0, C.byref(h)) == E_ARG and h.value is None
    assert lib.issl_annotation_open_file(b"x", 0, None) == E_ARG
    n = C.c_uint64()
    assert lib.issl_annotation_info(None, *[C.byref(n)] * 5) == E_ARG
    name, name_len, seq = C.c_void_p(), C.c_size_t(), C.c_uint32()
    assert lib.issl_annotation_seq(None, 0, C.byref(name), C.byref(name_len)) == E_ARG
    assert lib.issl_annotation_lookup(None, b"x", 1, C.byref(seq)) == E_ARG
    assert lib.issl_annotation_hits(None, None, None, 0, None) == E_ARG
    assert lib.issl_annotation_hits_device(None, None, None, 0, None, None) == E_ARG
    assert lib.issl_annotation_hits_occurrences_device(None, None, None, 0, None, None) == E_ARG
    assert lib.issl_annotation_close(None) == 0
    assert b"null argument" in lib.issl_last_error()


def test_a_file_that_is_not_there(tmp_path):
    h = C.c_void_p(0x1234)
    assert _lib.lib.issl_annotation_open_file(str(tmp_path / "absent.gff").encode(), 0, C.byref(h)) == E_IO and h.value is None


@pytest.mark.parametrize("path", ANNOTATIONS, ids=[p.parent.name for p in ANNOTATIONS])
def test_format_comes_before_the_device(path):
    """Malformed: ISSL_E_FORMAT anywhere.  Well-formed: ISSL_E_DEVICE where there is no GPU, a handle where there is one."""
    blob = path.read_bytes()
    for rc, h in (lambda a, b: ((_lib.lib.issl_annotation_open(blob, len(blob), 0, C.byref(a)), a),
                                (_lib.lib.issl_annotation_open_file(str(path).encode(), 0, C.byref(b)), b)))(C.c_void_p(0x1234), C.c_void_p(0x1234)):
        if path in MALFORMED:
            assert rc == E_FORMAT and h.value is None and b"annotation line" in _lib.lib.issl_last_error()
            with pytest.raises(tu.FormatError):
                tu.Model(blob)
        elif has_gpu():
            assert rc == 0 and h.value
            assert _lib.lib.issl_annotation_close(h) == 0
        else:
            assert rc == E_DEVICE and h.value is None
            tu.Model(blob)
