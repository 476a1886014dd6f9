"""The off-target report's ABI without a device: struct layouts as bound, exported names, argument errors."""
import ctypes as C
import pathlib
import re

import numpy as np

import crackling_amd as ca
from crackling_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ("issl_offtarget_profile", "issl_offtarget_profile_device", "issl_offtargets", "issl_offtargets_device")


def test_struct_layouts():
    assert C.sizeof(_lib.Offtarget) == 40 == ca.OFFTARGET_DTYPE.itemsize
    want = {"site": 0, "mit": 8, "cfd": 16, "guide": 24, "id": 28, "occ": 32, "dist": 36, "slice": 38}
    for name, off in want.items():
        assert getattr(_lib.Offtarget, name).offset == off == ca.OFFTARGET_DTYPE.fields[name][1]
    assert C.sizeof(_lib.Profile) == 88 == ca.PROFILE_DTYPE.itemsize
    for name, off in {"sites": 0, "pad": 28, "occurrences": 32}.items():
        assert getattr(_lib.Profile, name).offset == off == ca.PROFILE_DTYPE.fields[name][1]
    header = (ROOT / "include" / "issl_hip.h").read_text()
    assert re.search(r"#define\s+ISSL_PROFILE_BINS\s+7\b", header) and _lib.PROFILE_BINS == 7
    body = re.search(r"typedef struct \{([^}]*)\} issl_offtarget;", header).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == list(want)   # the header's field order is the bound one


def test_names_in_header_map_and_library():
    header = (ROOT / "include" / "issl_hip.h").read_text()
    lib = C.CDLL(_lib.LIB_PATH)
    assert "issl_*" in (ROOT / "crackling_amd" / "csrc" / "libissl_hip.map").read_text()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and hasattr(lib, name) and name in _lib.EXPORTS


def test_argument_errors_without_a_device(golden_uniform):
    ix = ca.IsslIndex.open(golden_uniform.issl)   # not uploaded
    sigs = ca.encode_guides([s.encode() for s in golden_uniform.guides])
    off = np.zeros(len(sigs) + 1, dtype=np.uint64)
    prof = np.zeros(len(sigs), dtype=ca.PROFILE_DTYPE)
    n = C.c_size_t()
    L = _lib.lib
    try:
        for bad in (-1, 7, 100):   # max_dist outside 0..6: an argument error, before the state of the handle is looked at
            assert L.issl_offtarget_profile(ix._h, sigs.ctypes.data, len(sigs), bad, prof.ctypes.data) == -1
            assert L.issl_offtarget_profile_device(ix._h, sigs.ctypes.data, len(sigs), bad, prof.ctypes.data, None) == -1
            assert L.issl_offtargets(ix._h, sigs.ctypes.data, len(sigs), bad, off.ctypes.data, None, 0, C.byref(n)) == -1
            assert L.issl_offtargets_device(ix._h, sigs.ctypes.data, len(sigs), bad, off.ctypes.data, None, 0, C.byref(n), None) == -1
            assert b"max_dist" in L.issl_last_error()
        assert L.issl_offtarget_profile(None, sigs.ctypes.data, len(sigs), 4, prof.ctypes.data) == -1
        assert L.issl_offtarget_profile(ix._h, None, len(sigs), 4, prof.ctypes.data) == -1
        assert L.issl_offtarget_profile(ix._h, sigs.ctypes.data, len(sigs), 4, None) == -1
        assert L.issl_offtargets(ix._h, sigs.ctypes.data, len(sigs), 4, None, None, 0, C.byref(n)) == -1
        assert L.issl_offtargets(ix._h, sigs.ctypes.data, len(sigs), 4, off.ctypes.data, None, 0, None) == -1
        assert L.issl_offtargets(ix._h, sigs.ctypes.data, len(sigs), 4, off.ctypes.data, None, 5, C.byref(n)) == -1
        assert L.issl_offtargets(ix._h, None, len(sigs), 4, off.ctypes.data, None, 0, C.byref(n)) == -1
        # well-formed calls on a handle without a device image: ISSL_E_STATE
        assert L.issl_offtarget_profile(ix._h, sigs.ctypes.data, len(sigs), 4, prof.ctypes.data) == -7
        assert L.issl_offtargets(ix._h, sigs.ctypes.data, len(sigs), 4, off.ctypes.data, None, 0, C.byref(n)) == -7
        assert L.issl_offtarget_profile_device(ix._h, sigs.ctypes.data, len(sigs), 4, prof.ctypes.data, None) == -7
        assert L.issl_offtargets_device(ix._h, sigs.ctypes.data, len(sigs), 4, off.ctypes.data, None, 0, C.byref(n), None) == -7
    finally:
        ix.close()
