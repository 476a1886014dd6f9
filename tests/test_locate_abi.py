"""CPU: the genome / locate part of the C ABI (issl_genome_*), bin/isslLocateOfftargets' argument handling, and the
brute force the GPU tests take their expected locations from, pinned to the reference-made site lists."""
import ctypes as C
import json
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import locate_util as lu

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXTRACT = ROOT / "tests" / "golden" / "extract"
SYMBOLS = ["issl_genome_open", "issl_genome_open_files", "issl_genome_info", "issl_genome_record", "issl_genome_locate",
           "issl_genome_locate_device", "issl_genome_close"]
EXE = str(ROOT / "bin" / "isslLocateOfftargets")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_seven_symbols_are_exported_and_declared():
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert lib.issl_abi_version() == 6
    assert "#define ISSL_ABI_VERSION 6" in header
    assert "first 20 of the 23" in header.lower()


def test_location_layout():
    assert C.sizeof(_lib.Location) == 16
    assert (_lib.Location.pos.offset, _lib.Location.record.offset, _lib.Location.strand.offset) == (0, 8, 12)
    assert ca.LOCATION_DTYPE.itemsize == 16
    assert [ca.LOCATION_DTYPE.fields[k][1] for k in ("pos", "record", "strand")] == [0, 8, 12]
    header = (ROOT / "include" / "issl_hip.h").read_text()
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_location;", header)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [("uint64_t", "pos"), ("uint32_t", "record"), ("uint32_t", "strand")]


def test_null_and_zero_arguments():
    lib = _lib.lib
    h = C.c_void_p(0x1234)
    blob = (C.c_char_p * 1)(b">a\nACGT\n")
    lens = (C.c_size_t * 1)(8)
    assert lib.issl_genome_open(None, lens, 1, 0, C.byref(h)) == -1 and h.value is None  # *out is not left dangling
    assert lib.issl_genome_open(blob, None, 1, 0, C.byref(h)) == -1
    assert lib.issl_genome_open(blob, lens, 0, 0, C.byref(h)) == -1
    assert lib.issl_genome_open(blob, lens, -3, 0, C.byref(h)) == -1
    assert lib.issl_genome_open(blob, lens, 1, 0, None) == -1
    assert lib.issl_genome_open_files(None, 1, 0, C.byref(h)) == -1
    assert lib.issl_genome_open_files((C.c_char_p * 1)(b"x.fa"), 0, 0, C.byref(h)) == -1
    assert lib.issl_genome_open_files((C.c_char_p * 1)(b"x.fa"), 1, 0, None) == -1
    n, m = C.c_uint64(), C.c_uint64()
    assert lib.issl_genome_info(None, C.byref(n), C.byref(m)) == -1
    name, ln, length = C.c_void_p(), C.c_size_t(), C.c_uint64()
    assert lib.issl_genome_record(None, 0, C.byref(name), C.byref(ln), C.byref(length)) == -1
    offs = (C.c_uint64 * 2)()
    sites = (C.c_uint64 * 1)(0)
    tot = C.c_size_t()
    assert lib.issl_genome_locate(None, sites, 1, offs, None, 0, C.byref(tot)) == -1
    assert lib.issl_genome_locate_device(None, sites, 1, offs, None, 0, C.byref(tot), None) == -1
    assert lib.issl_last_error()
    assert lib.issl_genome_close(None) == 0  # as issl_index_close


def test_open_without_a_device_fails_loudly(tmp_path):
    if _has_gpu():
        pytest.skip("GPU present")
    lib = _lib.lib
    h = C.c_void_p(0x1234)
    blob = (C.c_char_p * 1)(b">a\nACGTACGTACGTACGTACGTACGTAGG\n")
    lens = (C.c_size_t * 1)(len(blob[0]))
    assert lib.issl_genome_open(blob, lens, 1, 0, C.byref(h)) == -5
    assert h.value is None and lib.issl_last_error()
    with pytest.raises(ca.IsslError) as e:
        ca.Genome.open([EXTRACT / "multi.fa"])
    assert e.value.code == -5 and e.value.message
    p = tmp_path / "missing.fa"
    assert lib.issl_genome_open_files((C.c_char_p * 1)(os.fsencode(p)), 1, 0, C.byref(h)) == -2  # the file comes first


def test_cli_argument_and_file_errors(tmp_path):
    good = tmp_path / "sites.txt"
    good.write_text("ACGTACGTACGTACGTACGT\n")
    fasta = str(EXTRACT / "multi.fa")
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGT\n")
    badtsv = tmp_path / "bad.tsv"
    badtsv.write_text("ACGTACGTACGTACGTACGT\tACGT\t1\t1\t0\t0\n")
    for args in ([], [str(good)], ["--report", str(good)], [str(tmp_path / "nope.txt"), fasta], [str(bad), fasta],
                 ["--report", str(badtsv), fasta], ["--report", str(good), fasta], ["--report", str(tmp_path / "nope.tsv"), fasta],
                 [str(good), str(tmp_path / "nope.fa")]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr, args
    r = subprocess.run([EXE], capture_output=True)
    assert b"Usage" in r.stderr
    if not _has_gpu():
        r = subprocess.run([EXE, str(good), fasta], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr


def _fixtures():
    out = [("multi", [EXTRACT / "multi.fa"], EXTRACT / "multi.sites.txt"), ("repeat", [EXTRACT / "repeat.fa"], EXTRACT / "repeat.sites.txt")]
    for c in json.loads((EXTRACT / "cases" / "cases.json").read_text()):
        d = EXTRACT / "cases" / c["case"]
        if (d / "sites.txt").exists():
            out.append((c["case"], sorted(d / i for i in c["inputs"] if not i.startswith(".")), d / "sites.txt"))
    return out


@pytest.mark.parametrize("name,inputs,sites", _fixtures(), ids=[f[0] for f in _fixtures()])
def test_brute_force_is_the_reference_site_list(name, inputs, sites):
    """The expected locations of tests/test_locate.py come from locate_util.brute_force; its sites, as a multiset, are the
    lines the reference wrote for the same inputs."""
    truth = lu.brute_force(lu.parse([p.read_bytes() for p in inputs]))
    assert sorted(lu.sig_text(truth["site"])) == sorted(sites.read_bytes().split())
    assert np.array_equal(ca.encode_guides(lu.sig_text(truth["site"])), truth["site"])
