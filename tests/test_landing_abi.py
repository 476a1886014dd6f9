"""CPU: the off-target landings part of the C ABI (issl_offtarget_landings*, issl_offtarget_landing_profile*), its two
structs as the header, ctypes and numpy lay them out, and bin/isslLandOfftargets' argument handling."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np

import crackling_amd as ca
from crackling_amd import _lib
import landing_util as mu

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ["issl_offtarget_landings", "issl_offtarget_landings_device", "issl_offtarget_landing_profile",
           "issl_offtarget_landing_profile_device"]
STRUCTS = ["issl_landing", "issl_landing_profile"]
EXE = str(ROOT / "bin" / "isslLandOfftargets")
HEADER = (ROOT / "include" / "issl_hip.h").read_text()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_six_names_are_declared_exported_and_bound():
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", HEADER))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    for name in STRUCTS:
        assert re.search(r"\}\s*%s;" % name, HEADER), name
    assert (_lib.Landing, _lib.LandingProfile) and (ca.LANDING_DTYPE, ca.LANDING_PROFILE_DTYPE)
    assert lib.issl_abi_version() == 6
    assert "#define ISSL_ABI_VERSION 6" in HEADER
    for method in ("landings", "landing_profile", "landings_device", "landing_profile_device"):
        assert callable(getattr(ca.IsslIndex, method))


def test_struct_layouts():
    assert C.sizeof(_lib.Landing) == 64 and C.sizeof(_lib.LandingProfile) == 144
    want = {"site": 0, "pos": 8, "record": 16, "strand": 20, "guide": 24, "rank": 28, "id": 32, "occ": 36, "dist": 40, "slice": 42, "pad": 44,
            "hits": 48}
    assert {k: getattr(_lib.Landing, k).offset for k in want} == want
    assert ca.LANDING_DTYPE.itemsize == 64 and {k: ca.LANDING_DTYPE.fields[k][1] for k in want} == want
    assert ca.LANDING_DTYPE.fields["hits"][0] == ca.TRANSCRIPT_HITS_DTYPE
    assert ca.LANDING_DTYPE == mu.LANDING and ca.LANDING_PROFILE_DTYPE == mu.PROFILE
    want = {"located": 0, "in_exon": 56, "absent": 112, "pad": 140}
    assert {k: getattr(_lib.LandingProfile, k).offset for k in want} == want
    assert ca.LANDING_PROFILE_DTYPE.itemsize == 144 and {k: ca.LANDING_PROFILE_DTYPE.fields[k][1] for k in want} == want
    # the header's field order
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_landing;", HEADER)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [n.strip() for t, names in re.findall(r"(uint\d+_t|issl_transcript_hits)\s+([\w, ]+);", body) for n in names.split(",")]
    assert fields == ["site", "pos", "record", "strand", "guide", "rank", "id", "occ", "dist", "slice", "pad", "hits"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_landing_profile;", HEADER)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(uint\d+_t)\s+(\w+)(?:\[ISSL_PROFILE_BINS\])?;", body) == [
        ("uint64_t", "located"), ("uint64_t", "in_exon"), ("uint32_t", "absent"), ("uint32_t", "pad")]


def test_null_arguments():
    lib = _lib.lib
    h = C.c_void_p(0x1234)  # never dereferenced: the argument checks come first
    guides = (C.c_uint64 * 1)(0)
    offs = (C.c_uint64 * 2)()
    tot = C.c_size_t()
    rows = (C.c_uint8 * 64)()
    prof = (C.c_uint8 * 144)()
    E_ARG = -1
    for fn, tail in ((lib.issl_offtarget_landings, ()), (lib.issl_offtarget_landings_device, (None,))):
        assert fn(None, h, None, guides, 1, 4, offs, None, 0, C.byref(tot), *tail) == E_ARG
        assert fn(h, None, None, guides, 1, 4, offs, None, 0, C.byref(tot), *tail) == E_ARG
        assert fn(None, None, None, None, 1, 4, offs, None, 0, C.byref(tot), *tail) == E_ARG
        assert fn(None, h, None, guides, 1, 4, None, None, 0, C.byref(tot), *tail) == E_ARG
        assert fn(None, h, None, guides, 1, 4, offs, None, 0, None, *tail) == E_ARG
        assert fn(None, h, None, guides, 1, 4, offs, None, 5, C.byref(tot), *tail) == E_ARG  # room claimed, no rows
        assert fn(None, h, None, guides, 1, 4, offs, rows, 1, C.byref(tot), *tail) == E_ARG
    for fn, tail in ((lib.issl_offtarget_landing_profile, ()), (lib.issl_offtarget_landing_profile_device, (None,))):
        assert fn(None, h, None, guides, 1, 4, prof, *tail) == E_ARG
        assert fn(h, None, None, guides, 1, 4, prof, *tail) == E_ARG
        assert fn(None, h, None, None, 1, 4, prof, *tail) == E_ARG
        assert fn(None, h, None, guides, 1, 4, None, *tail) == E_ARG
    assert lib.issl_last_error()


def test_an_index_that_is_not_uploaded_answers_as_the_report_does():
    lib = _lib.lib
    ix = ca.IsslIndex.open(ROOT / "tests" / "golden" / "uniform" / "index.issl")
    guides = np.zeros(1, dtype=np.uint64)
    offs = np.zeros(2, dtype=np.uint64)
    tot = C.c_size_t()
    g = C.c_void_p(0x1234)  # never dereferenced: the state of the index comes before the genome is touched
    want = lib.issl_offtargets(ix._h, guides.ctypes.data, 1, 4, offs.ctypes.data, None, 0, C.byref(tot))
    assert want != 0
    assert lib.issl_offtarget_landings(ix._h, g, None, guides.ctypes.data, 1, 4, offs.ctypes.data, None, 0, C.byref(tot)) == want
    prof = np.zeros(1, dtype=ca.LANDING_PROFILE_DTYPE)
    assert lib.issl_offtarget_landing_profile(ix._h, g, None, guides.ctypes.data, 1, 4, prof.ctypes.data) == want
    assert lib.issl_offtarget_landings(ix._h, g, None, guides.ctypes.data, 1, 7, offs.ctypes.data, None, 0, C.byref(tot)) == -1  # max_dist 0..6
    ix.close()


def test_cli_argument_and_file_errors(tmp_path):
    issl = str(ROOT / "tests" / "golden" / "uniform" / "index.issl")
    fasta = str(ROOT / "tests" / "golden" / "extract" / "multi.fa")
    good = tmp_path / "q.txt"
    good.write_text("ACGTACGTACGTACGTACGT\n")
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGT\n")
    for args in ([], [issl], [issl, str(good)], [issl, str(good), "4"], ["--profile", issl, str(good), "4"],
                 [issl, str(good), "4", fasta, "--annotation"], [issl, str(good), "x", fasta], [issl, str(good), "7", fasta],
                 [issl, str(good), "-1", fasta], [str(tmp_path / "nope.issl"), str(good), "4", fasta],
                 [issl, str(tmp_path / "nope.txt"), "4", fasta], [issl, str(bad), "4", fasta]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr, args
    r = subprocess.run([EXE], capture_output=True)
    assert b"Usage" in r.stderr and b"--annotation" in r.stderr and b"--profile" in r.stderr
    if not _has_gpu():
        r = subprocess.run([EXE, issl, str(good), "4", fasta], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr
