"""CPU: the bulge search part of the C ABI (issl_genome_search_bulges*), every error of its contract through all four entry
points, bin/isslSearchGenome's new options, and the shared bulge arithmetic under AddressSanitizer + UBSan
(tools/bulge_sanitize.cpp, a stand-alone program)."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_genome_search_bulges", "issl_genome_search_bulges_device", "issl_genome_search_bulges_profile",
           "issl_genome_search_bulges_profile_device"]
EXE = str(ROOT / "bin" / "isslSearchGenome")
FASTA = str(ROOT / "tests" / "golden" / "extract" / "multi.fa")
NGG = "N" * 21 + "GG"


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_symbols_are_declared_exported_and_bound():
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", HEADER))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, HEADER) and name in declared, name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.issl_abi_version() == 6 and "#define ISSL_ABI_VERSION 6" in HEADER  # additions only
    for name in ("search_bulges", "search_bulges_profile", "search_bulges_device", "search_bulges_profile_device"):
        assert callable(getattr(ca.Genome, name))
    assert "These rows are listed" in HEADER  # no filtering of the shifted windows: the header says so


def _header_fields(name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, HEADER)
    assert m, name
    out = []
    for kind, names in re.findall(r"(u?int\d+_t)\s+([\w, ]+);", m.group(1)):
        out += [(kind, n.strip()) for n in names.split(",")]
    return out


def test_struct_layouts_agree():
    assert _header_fields("issl_search_bulges") == [("uint32_t", n) for n in ("guide_start", "guide_length", "max_dna", "max_rna")]
    assert _header_fields("issl_bulge_hit") == [("uint64_t", "site"), ("uint64_t", "pos"), ("uint32_t", "record"), ("uint32_t", "query"),
                                                ("uint32_t", "mism"), ("uint8_t", "strand"), ("uint8_t", "dist"), ("int8_t", "bulge"),
                                                ("uint8_t", "at")]
    B, H = _lib.SearchBulges, _lib.BulgeHit
    assert (C.sizeof(B), C.sizeof(H)) == (16, 32)
    assert [getattr(B, k).offset for k in ("guide_start", "guide_length", "max_dna", "max_rna")] == [0, 4, 8, 12]
    names = ("site", "pos", "record", "query", "mism", "strand", "dist", "bulge", "at")
    offsets = [0, 8, 16, 20, 24, 28, 29, 30, 31]
    assert [getattr(H, k).offset for k in names] == offsets
    assert ca.BULGE_HIT_DTYPE.itemsize == 32 and ca.BULGE_HIT_DTYPE.names == names
    assert [ca.BULGE_HIT_DTYPE.fields[k][1] for k in names] == offsets
    assert ca.BULGE_HIT_DTYPE["bulge"] == np.int8 and ca.BULGE_HIT_DTYPE["at"] == np.uint8
    # the mismatch search's row with its two reserved bytes named: D = R = 0 gives the same bytes
    assert [ca.SEARCH_HIT_DTYPE.fields[k][1] for k in names[:7]] == offsets[:7]


def _error():
    return _lib.lib.issl_last_error().decode(errors="replace")


def test_errors_come_before_any_device_work():
    """A sentinel handle that is never dereferenced: every refusal is made on the arguments alone, by all four entry points."""
    lib = _lib.lib
    g = C.c_void_p(0x1234)
    pat, q = ca.search_prepare(NGG, ["ACGTACGTACGTACGTACGTNNN"])
    offs = np.zeros(2, dtype=np.uint64)
    hits = np.zeros(4, dtype=ca.BULGE_HIT_DTYPE)
    counts = np.zeros(7 * 24, dtype=np.uint64)
    tot = C.c_size_t()
    P, Q, O, H, K = C.byref(pat), q.ctypes.data, offs.ctypes.data, hits.ctypes.data, counts.ctypes.data

    def every_entry(bulges, max_dist=1, pat_ref=P, queries=Q):
        bg = _lib.SearchBulges(*bulges)
        return [lib.issl_genome_search_bulges(g, pat_ref, C.byref(bg), queries, 1, max_dist, O, H, 4, C.byref(tot)),
                lib.issl_genome_search_bulges_device(g, pat_ref, C.byref(bg), queries, 1, max_dist, O, H, 4, C.byref(tot), None),
                lib.issl_genome_search_bulges_profile(g, pat_ref, C.byref(bg), queries, 1, max_dist, K),
                lib.issl_genome_search_bulges_profile_device(g, pat_ref, C.byref(bg), queries, 1, max_dist, K, None)]

    refused = [-1] * 4
    # the span
    for span in ((4, 20), (0, 1), (0, 0), (23, 2), (22, 2), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF), (0, 24)):
        assert every_entry(span + (1, 1)) == refused and "span (%d, %d)" % span in _error(), span
    # D or R above 3
    assert every_entry((0, 20, 4, 0)) == refused and "max_dna 4" in _error()
    assert every_entry((0, 20, 0, 4)) == refused and "max_rna 4" in _error()
    assert every_entry((0, 20, 0xFFFFFFFF, 0)) == refused and "max_dna" in _error()
    # L + D > 32
    long_pat, long_q = ca.search_prepare("N" * 28 + "NGG", ["N" * 31])
    assert every_entry((0, 28, 2, 0), pat_ref=C.byref(long_pat), queries=long_q.ctypes.data) == refused
    assert "max_dna 2" in _error() and "31" in _error()
    # R > G - 2
    assert every_entry((0, 3, 0, 2)) == refused and "max_rna 2" in _error() and "guide_length 3" in _error()
    assert every_entry((0, 2, 0, 1)) == refused and "max_rna 1" in _error()
    # a restricted position that is not N: named
    assert every_entry((0, 23, 1, 0)) == refused and "position 21" in _error()
    assert every_entry((1, 22, 0, 1)) == refused and "position 21" in _error()
    coded, _ = ca.search_prepare("NNNNNRNNNNNNNNNNNNNNNGG", [])
    assert every_entry((0, 20, 0, 1), pat_ref=C.byref(coded)) == refused and "position 5" in _error()
    # everything issl_genome_search refuses
    for d in (-1, 24, 1 << 20):
        assert every_entry((0, 20, 1, 1), max_dist=d) == refused and "max_dist" in _error()
    bad = _lib.SearchPattern()
    for length in (0, 33):
        C.memmove(C.byref(bad), C.byref(pat), 32)
        bad.length = length
        assert every_entry((0, 20, 1, 1), pat_ref=C.byref(bad)) == refused and "length" in _error()
    C.memmove(C.byref(bad), C.byref(pat), 32)
    bad.allow[2] |= 1 << 23
    assert every_entry((0, 20, 1, 1), pat_ref=C.byref(bad)) == refused and "allow[2]" in _error()
    C.memmove(C.byref(bad), C.byref(pat), 32)
    for b in range(4):
        bad.allow[b] &= ~(1 << 5)
    assert every_entry((0, 20, 1, 1), pat_ref=C.byref(bad)) == refused and "position 5" in _error()
    for sig, care in ((1 << 46, 0), (0, 1 << 47), (0, 1), (2, 0)):
        bq = np.array([(sig, care)], dtype=ca.SEARCH_QUERY_DTYPE)
        bg = _lib.SearchBulges(0, 20, 1, 1)
        assert lib.issl_genome_search_bulges(g, P, C.byref(bg), bq.ctypes.data, 1, 1, O, H, 4, C.byref(tot)) == -1 and "query 0" in _error()
        assert lib.issl_genome_search_bulges_profile(g, P, C.byref(bg), bq.ctypes.data, 1, 1, K) == -1
    # NULLs
    bg = _lib.SearchBulges(0, 20, 1, 1)
    G = C.byref(bg)
    assert lib.issl_genome_search_bulges(None, P, G, Q, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, None, G, Q, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, P, None, Q, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, P, G, None, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, P, G, Q, 1, 1, None, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, P, G, Q, 1, 1, O, None, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges(g, P, G, Q, 1, 1, O, H, 4, None) == -1
    assert lib.issl_genome_search_bulges_device(g, P, None, Q, 1, 1, O, H, 4, C.byref(tot), None) == -1
    assert lib.issl_genome_search_bulges_device(g, P, G, Q, 1, 1, O, None, 4, C.byref(tot), None) == -1
    assert lib.issl_genome_search_bulges_profile(g, P, None, Q, 1, 1, K) == -1
    assert lib.issl_genome_search_bulges_profile(g, P, G, Q, 1, 1, None) == -1
    assert lib.issl_genome_search_bulges_profile_device(g, P, None, Q, 1, 1, K, None) == -1
    assert lib.issl_genome_search_bulges_profile_device(g, P, G, None, 1, 1, K, None) == -1
    assert "null" in _error()


def test_cli_argument_errors(tmp_path):
    good = tmp_path / "queries.txt"
    good.write_text("ACGTACGTACGTACGTACGTNNN\n")
    tail = [NGG, str(good), "2", FASTA]
    for args in (["--dna-bulge", "1"] + tail, ["--rna-bulge", "1"] + tail, ["--profile", "--dna-bulge", "1", "--rna-bulge", "1"] + tail,
                 tail + ["--dna-bulge", "1"]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr and b"--guide" in r.stderr, args
    for args, message in ((["--guide"], b"Usage"), (["--guide", "0:20", "--dna-bulge"], b"Usage"),
                          (["--guide", "0"] + tail, b"START:LEN"), (["--guide", "0:"] + tail, b"START:LEN"),
                          (["--guide", ":20"] + tail, b"START:LEN"), (["--guide", "0:20x"] + tail, b"START:LEN"),
                          (["--guide", "-1:20"] + tail, b"START:LEN"), (["--guide", "0:20", "--dna-bulge", "one"] + tail, b"0 to 3"),
                          (["--guide", "0:20", "--rna-bulge", "-1"] + tail, b"0 to 3"),
                          (["--guide", "0:20", "--dna-bulge", "4"] + tail, b"max_dna 4"),
                          (["--guide", "0:20", "--rna-bulge", "4"] + tail, b"max_rna 4"),
                          (["--guide", "4:20"] + tail, b"span (4, 20)"), (["--guide", "0:1"] + tail, b"span (0, 1)"),
                          (["--guide", "0:23"] + tail, b"position 21"), (["--guide", "0:3", "--rna-bulge", "2"] + tail, b"max_rna 2"),
                          (["--guide", "0:20", NGG, str(good), "24", FASTA], b"max_dist"),
                          (["--profile", "--guide", "0:20", NGG, str(tmp_path / "nope.txt"), "2", FASTA], b"cannot open")):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and message in r.stderr, (args, r.stderr)
    if not _has_gpu():
        for mode in ([], ["--profile"]):
            r = subprocess.run([EXE] + mode + ["--guide", "0:20", "--dna-bulge", "2", "--rna-bulge", "2"] + tail, capture_output=True)
            assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr


def test_bulge_arithmetic_under_asan_and_ubsan(tmp_path):
    """tools/bulge_sanitize.cpp: the packed-word functions the kernels, the finish pass and the executable share against
    character loops over the derived pairs of the contract -- every L in 2..32, every legal span start, every b with
    L + b <= 32, every break point, with and without N in the query, and the bound never above the minimum."""
    exe = tmp_path / "bulge_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "bulge_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0 and b"ERROR" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode(errors="replace")[-4000:]
    got = run.stdout.decode().split("\n")[:-1]
    m = re.fullmatch(r"bulges ok (\d+)", got[0])
    assert m and int(m.group(1)) > 100000
    assert got[1:4] == ["accepted"] * 3
    for line, message in zip(got[4:15], ["span (4, 20)", "span (0, 1)", "span (24, 2)", "span (4294967295, 2)", "span (2, 4294967295)",
                                         "max_dna 4", "max_rna 4", "max_dna 1 with a pattern of 32", "max_rna 2 with guide_length 3",
                                         "pattern position 21", "pattern position 5"]):
        assert line.startswith("refused ") and message in line, line
    assert got[15:] == ["CCGTACGTAC-TGCAACGTACNGG\tchr\t1234567890123\t-\t2\tD1\taCGTACGTACTtGCAACGTACGGG",
                        "TTTACGTACGTACTTGCAACGTA\tchr\t1234567890123\t-\t2\tR2\tACgTAcG--TACTTGCAACGTAc",
                        "ATG\t\t1234567890123\t-\t2\t0\tAcG"]
