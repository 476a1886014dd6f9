"""CPU: the guide-extraction part of the C ABI (issl_guides_*), and the brute force the GPU tests take their expected
guide sets from (tests/guides_util.py), pinned row for row to what the reference's own extraction wrote
(tests/golden/guides/, tools/make_golden_guides.py)."""
import ctypes as C
import os
import pathlib
import re
import subprocess

import pytest

import guides_util as gu

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ["issl_guides_extract", "issl_guides_extract_files", "issl_guides_info", "issl_guides_record", "issl_guides_copy",
           "issl_guides_device", "issl_guides_close"]
TYPES = ["issl_guide_set", "issl_guide"]  # with the seven functions: the nine names the header adds
EXE = str(ROOT / "bin" / "cracklingGuides")
CASES = gu.golden_cases()
FIELDS = [("uint64_t", "guide23"), ("uint64_t", "start"), ("uint32_t", "record"), ("uint32_t", "strand"), ("uint32_t", "seen"),
          ("uint32_t", "reserved")]


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_nine_names_are_declared_and_exported():
    """Seven functions, declared in the header, exported by the library and bound by the package; the two type names are
    only pinned to the header's text as it spells the typedefs today (`typedef struct issl_guide_set issl_guide_set;`,
    `} issl_guide;`) -- nothing else can see a C type."""
    from crackling_amd import _lib
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    for name in TYPES:
        assert re.search(r"^(typedef struct %s |\} )%s;" % (name, name), header, re.M), name
    assert lib.issl_abi_version() == 6
    assert "#define ISSL_ABI_VERSION 6" in header
    assert "ISSL_GUIDES_TIMING" in header and "Crackling.py:151-305" in header


def test_guide_layout():
    import crackling_amd as ca
    from crackling_amd import _lib
    assert C.sizeof(_lib.Guide) == 32 and ca.GUIDE_DTYPE.itemsize == 32
    offsets = [0, 8, 16, 20, 24, 28]
    assert [getattr(_lib.Guide, n).offset for _, n in FIELDS] == offsets
    assert [ca.GUIDE_DTYPE.fields[n][1] for _, n in FIELDS] == offsets
    assert list(ca.GUIDE_DTYPE.names) == [n for _, n in FIELDS]
    header = (ROOT / "include" / "issl_hip.h").read_text()
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_guide;", header)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == FIELDS


def test_null_and_zero_arguments():
    from crackling_amd import _lib
    lib = _lib.lib
    h = C.c_void_p(0x1234)
    blob = (C.c_char_p * 1)(b">a\nACGT\n")
    lens = (C.c_size_t * 1)(8)
    assert lib.issl_guides_extract(None, lens, 1, 0, C.byref(h)) == -1 and h.value is None  # *out is not left dangling
    assert lib.issl_guides_extract(blob, None, 1, 0, C.byref(h)) == -1
    assert lib.issl_guides_extract(blob, lens, 0, 0, C.byref(h)) == -1
    assert lib.issl_guides_extract(blob, lens, -3, 0, C.byref(h)) == -1
    assert lib.issl_guides_extract(blob, lens, 1, 0, None) == -1
    assert lib.issl_guides_extract((C.c_char_p * 1)(None), lens, 1, 0, C.byref(h)) == -1
    h = C.c_void_p(0x1234)
    assert lib.issl_guides_extract_files(None, 1, 0, C.byref(h)) == -1 and h.value is None
    assert lib.issl_guides_extract_files((C.c_char_p * 1)(b"x.fa"), 0, 0, C.byref(h)) == -1
    assert lib.issl_guides_extract_files((C.c_char_p * 1)(b"x.fa"), 1, 0, None) == -1
    assert lib.issl_guides_extract_files((C.c_char_p * 1)(None), 1, 0, C.byref(h)) == -1
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.issl_guides_info(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == -1
    name, ln, length = C.c_void_p(), C.c_size_t(), C.c_uint64()
    assert lib.issl_guides_record(None, 0, C.byref(name), C.byref(ln), C.byref(length)) == -1
    assert lib.issl_guides_copy(None, None, 0) == -1
    p, q = C.c_void_p(), C.c_void_p()
    assert lib.issl_guides_device(None, C.byref(p), C.byref(q)) == -1
    assert lib.issl_last_error()
    assert lib.issl_guides_close(None) == 0  # as issl_index_close


def test_format_and_file_errors_come_before_the_device(tmp_path):
    """What the host pass refuses needs no device: a blank line is ISSL_E_FORMAT and the message names the input and the
    line; a missing file is ISSL_E_IO."""
    import crackling_amd as ca
    from crackling_amd import _lib
    blank = [c for c in CASES if c[0] == "blankline"][0][1][0]
    with pytest.raises(ca.IsslError) as e:
        ca.GuideSet.extract([blank])
    assert e.value.code == -3 and str(blank) in e.value.message and "line 4" in e.value.message
    with pytest.raises(ca.IsslError) as e:
        ca.GuideSet.extract([b">a\nACGT\n", blank.read_bytes()])
    assert e.value.code == -3 and "input 1" in e.value.message and "line 4" in e.value.message
    h = C.c_void_p(0x1234)
    missing = (C.c_char_p * 1)(os.fsencode(tmp_path / "missing.fa"))
    assert _lib.lib.issl_guides_extract_files(missing, 1, 0, C.byref(h)) == -2 and h.value is None
    (tmp_path / "empty").mkdir()
    assert _lib.lib.issl_guides_extract_files((C.c_char_p * 1)(os.fsencode(tmp_path / "empty")), 1, 0, C.byref(h)) == -2
    with pytest.raises(TypeError):
        ca.GuideSet.extract([])


def test_extract_without_a_device_fails_loudly():
    if _has_gpu():
        pytest.skip("GPU present")
    import crackling_amd as ca
    from crackling_amd import _lib
    h = C.c_void_p(0x1234)
    blob = (C.c_char_p * 1)(b">a\nACGTACGTACGTACGTACGTAGG\n")
    lens = (C.c_size_t * 1)(len(blob[0]))
    assert _lib.lib.issl_guides_extract(blob, lens, 1, 0, C.byref(h)) == -5
    assert h.value is None and _lib.lib.issl_last_error()
    multi = [c for c in CASES if c[0] == "multi"][0][1]
    with pytest.raises(ca.IsslError) as e:
        ca.GuideSet.extract(multi)
    assert e.value.code == -5 and e.value.message


def test_cli_argument_and_file_errors(tmp_path):
    blank = str([c for c in CASES if c[0] == "blankline"][0][1][0])
    for args in ([], ["--unique"], [str(tmp_path / "nope.fa")], ["--unique", str(tmp_path / "nope.fa")], [blank]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr, args
    assert b"Usage" in subprocess.run([EXE], capture_output=True).stderr
    r = subprocess.run([EXE, "--uniq", blank], capture_output=True)  # a mistyped option is not a path
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    assert b"line 4" in subprocess.run([EXE, blank], capture_output=True).stderr
    if not _has_gpu():
        multi = str([c for c in CASES if c[0] == "multi"][0][1][0])
        r = subprocess.run([EXE, multi], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr


def test_every_golden_case_is_listed():
    want = {"multi", "headers", "crlf", "dir3", "nomatch", "blankline"}
    assert {c[0] for c in CASES} == want
    assert {p.name[:-len(".guides.csv")] for p in gu.GOLDEN.glob("*.guides.csv")} == want
    assert [c[0] for c in CASES if c[3] != "ok"] == ["nomatch", "blankline"]


@pytest.mark.parametrize("case,paths,as_dir,reference,rows", CASES, ids=[c[0] for c in CASES])
def test_brute_force_is_the_reference_row_for_row(case, paths, as_dir, reference, rows):
    """The expected sets of tests/test_guides.py come from guides_util.parse / brute_force; here they are the reference's
    own rows: sequence, header, start, end, strand and isUnique, in its order."""
    blobs = [p.read_bytes() for p in paths]
    if as_dir:  # the order the reference reads a directory in
        assert [p.name for p in paths] == sorted((p.name for p in paths[0].parent.iterdir()), reverse=True)
        assert [p.name for p in paths] != sorted(p.name for p in paths)
    if reference == "raises IndexError":
        with pytest.raises(gu.BlankLine) as e:
            gu.parse(blobs)
        assert e.value.args == (0, 4) and rows == []
        return
    records = gu.parse(blobs)
    got = gu.reference_rows(records, gu.brute_force(records))
    assert got == rows
    if reference == "ok":
        assert len(rows) > 30
    else:  # the reference divides by its number of matches (Crackling.py:254): nothing found is an empty set here
        assert reference == "raises ZeroDivisionError" and rows == []


def test_the_golden_cases_hold_what_they_are_for():
    by = {c[0]: c for c in CASES}
    multi = by["multi"][4]
    assert sum(r[5] == "0" for r in multi) >= 3
    assert any("," in r[1] and '"' in r[1] for r in multi)
    assert {r[4] for r in multi} == {"+", "-"}
    records = gu.parse([by["multi"][1][0].read_bytes()])
    per_start = {}
    for r, (_, seq) in enumerate(records):
        for start, strand, _ in gu.matches(seq):
            per_start.setdefault((r, start), set()).add(strand)
    assert any(len(v) == 2 for v in per_start.values())  # one start, both patterns
    assert any(b"G" * 30 in seq for _, seq in records) and any(b"N" * 30 in seq for _, seq in records)
    assert any(seq != seq.upper() for _, seq in records)
    seen = gu.brute_force(records)["seen"]
    assert 3 in seen.tolist()
    headers = gu.parse([by["headers"][1][0].read_bytes()])
    assert [n for n, _ in headers] == [b"", b"alpha", b"beta indented", b"empty", b"gamma", b"", b"", b"alpha"]
    assert b"\r\n" in by["crlf"][1][0].read_bytes()
    assert len(by["dir3"][1]) == 3 and by["dir3"][2]
