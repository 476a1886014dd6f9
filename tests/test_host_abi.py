"""CPU: host logic of the product library and its C ABI (no compute calls: there is no GPU here)."""
import ctypes as C
import json
import os
import pathlib
import re
import resource
import subprocess
import sys

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import oracle_util as ou
from synth import random_sites, random_guides, sigs_to_text, text_order_key

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 24
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/issl_hip.h but not exported"
    assert declared == set(_lib.EXPORTS)
    assert lib.issl_abi_version() == 6


def test_builder_bytes_match_reference_golden(golden, tmp_path):
    ix = ca.IsslIndex.build_from_text(golden.sites_txt.read_bytes())
    out = tmp_path / "x.issl"
    ix.write(out)
    assert out.read_bytes() == golden.issl.read_bytes()


def test_builder_cli_matches_reference_golden(golden, tmp_path):
    out = tmp_path / "cli.issl"
    subprocess.run([str(ROOT / "bin" / "isslCreateIndex"), str(golden.sites_txt), "20", "8", str(out)], check=True,
                   capture_output=True)
    assert out.read_bytes() == golden.issl.read_bytes()


def test_builder_from_sites_equals_from_text_and_oracle():
    sigs, occ = random_sites(50000, seed=5)
    text = sigs_to_text(sigs, occ)
    a = ca.IsslIndex.build_from_sites(sigs, occ)
    b = ca.IsslIndex.build_from_text(text)
    assert a.header == b.header
    assert a.header["n_lines"] == 50000 and a.header["n_sites"] == len(sigs)
    assert np.array_equal(a.bucket_sizes(), b.bucket_sizes())
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        pa, pb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        a.write(pa); b.write(pb)
        da = open(pa, "rb").read()
        assert da == open(pb, "rb").read()
        assert da == ou.build_issl(text)


def test_builder_other_slice_widths_match_oracle():
    sigs, occ = random_sites(3000, seed=6)
    text = sigs_to_text(sigs, occ)
    import tempfile
    for w in (4, 5):
        ix = ca.IsslIndex.build_from_text(text, slice_width=w)
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a")
            ix.write(p)
            assert open(p, "rb").read() == ou.build_issl(text, slice_width=w), w


def test_builder_rejects_bad_geometry():
    sigs, occ = random_sites(100, seed=7)
    with pytest.raises(ca.IsslError):
        ca.IsslIndex.build_from_sites(sigs, occ, slice_width=9)  # reference truncates slice values to 8 bits
    with pytest.raises(ca.IsslError):
        ca.IsslIndex.build_from_sites(sigs, occ, slice_width=1)


def test_encode_decode_roundtrip_and_non_acgt():
    seqs = ["ACGTACGTACGTACGTACGT", "TTTTTTTTTTTTTTTTTTTT", "ACGTNCGTACGTACGTACGT", "acgtacgtacgtacgtacgt"]
    sig = ca.encode_guides(seqs)
    assert np.array_equal(sig, ou.encode(seqs))
    dec = ca.decode_guides(sig)
    assert dec[0] == seqs[0] and dec[1] == seqs[1]
    assert dec[2] == "ACGTACGTACGTACGTACGT" and dec[3] == "A" * 20  # other bytes pack as 'A' (:99-102)
    assert int(sig[1]) == (1 << 40) - 1


def test_open_validates_like_the_reference_or_stricter(golden_uniform, tmp_path):
    data = golden_uniform.issl.read_bytes()
    ix = ca.IsslIndex.from_bytes(data)
    hd = ix.header
    assert hd["seq_len"] == 20 and hd["slice_width"] == 8 and hd["n_slices"] == 5 and hd["n_scores"] == 6195
    assert int(ix.bucket_sizes().sum()) == 5 * hd["n_sites"]
    for cut, msg in [(20, "header invalid"), (48 + 16 * 100, "scores"), (48 + 16 * 6195 + 80, "off-target"),
                     (48 + 16 * 6195 + 8 * hd["n_sites"] + 64, "slice list sizes"), (len(data) - 8, "slice contents")]:
        with pytest.raises(ca.IsslError) as e:
            ca.IsslIndex.from_bytes(data[:cut])
        assert msg in str(e.value), (cut, str(e.value))
    with pytest.raises(ca.IsslError):
        ca.IsslIndex.open(tmp_path / "does-not-exist.issl")
    bad = bytearray(data)
    bad[8:16] = (99).to_bytes(8, "little")  # seq_len 99
    with pytest.raises(ca.IsslError):
        ca.IsslIndex.from_bytes(bytes(bad))


def test_query_file_rules(tmp_path):
    lib = _lib.lib
    p = tmp_path / "q.txt"
    p.write_text("ACGTACGTACGTACGTACGT\nTTTTTTTTTTTTTTTTTTTT\n")
    out = C.c_void_p(); n = C.c_size_t()
    assert lib.issl_read_query_file(os.fsencode(p), 20, C.byref(out), C.byref(n)) == 0
    assert n.value == 2
    arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(2,)).copy()
    lib.issl_free(out)
    assert np.array_equal(arr, ca.encode_guides(["ACGTACGTACGTACGTACGT", "T" * 20]))
    p.write_text("ACGTACGTACGTACGTACGT\r\n")  # CRLF: not a multiple of 21 (:277-282)
    assert lib.issl_read_query_file(os.fsencode(p), 20, C.byref(out), C.byref(n)) != 0
    assert "multiple of the expected line length" in lib.issl_last_error().decode()
    p.write_text("")  # empty: "Failed to read in query file." (:290-293)
    assert lib.issl_read_query_file(os.fsencode(p), 20, C.byref(out), C.byref(n)) != 0


def test_count_candidates_matches_bucket_arithmetic(golden_uniform):
    ix = ca.IsslIndex.open(golden_uniform.issl)
    sigs = ca.encode_guides([g for g in golden_uniform.guides])
    sizes = ix.bucket_sizes().reshape(5, 256)
    want = sum(int(sizes[s, (int(g) >> (8 * s)) & 0xFF]) for g in sigs for s in range(5))
    assert ix.count_candidates(sigs) == want


def test_scoring_without_device_fails_loudly(golden_uniform):
    """No silent CPU fallback: on a box without a GPU every compute entry point reports an error."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ix = ca.IsslIndex.open(golden_uniform.issl)
    with pytest.raises(ca.IsslError) as e:
        ix.upload(0)
    assert e.value.code == -5
    with pytest.raises(ca.IsslError) as e:
        ix.score(golden_uniform.guides[:3])
    assert e.value.code == -7  # no device image
    r = subprocess.run([str(ROOT / "bin" / "isslScoreOfftargets"), str(golden_uniform.issl),
                        str(golden_uniform.guides_txt), "4", "75", "and"], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr


def test_cli_argument_and_file_errors(golden_uniform, tmp_path):
    exe = str(ROOT / "bin" / "isslScoreOfftargets")
    r = subprocess.run([exe, str(golden_uniform.issl), str(golden_uniform.guides_txt), "4"], capture_output=True)
    assert r.returncode == 1 and b"Usage" in r.stderr and r.stdout == b""
    r = subprocess.run([exe, str(tmp_path / "nope.issl"), str(golden_uniform.guides_txt), "4", "75", "and"],
                       capture_output=True)
    assert r.returncode == 1 and r.stdout == b""
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGT\n")
    r = subprocess.run([exe, str(golden_uniform.issl), str(bad), "4", "75", "and"], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"multiple of the expected line length" in r.stderr


def test_scan_word_packing_host_model():
    """Host model of the device packing (issl_kernels.hpp scan_word): the fold of two scan words counts exactly
    the mismatches outside the bucket's own slice."""
    rng = np.random.default_rng(3)

    def gather_even16(x):
        x &= 0x55555555
        x = (x | (x >> 1)) & 0x33333333
        x = (x | (x >> 2)) & 0x0F0F0F0F
        x = (x | (x >> 4)) & 0x00FF00FF
        x = (x | (x >> 8)) & 0x0000FFFF
        return x

    def scan_word(sig, s):
        sh = 8 * s
        rem = ((sig & ((1 << sh) - 1)) | ((sig >> (sh + 8)) << sh)) & 0xFFFFFFFF
        return gather_even16(rem) | (gather_even16(rem >> 1) << 16)

    for _ in range(2000):
        a = int(rng.integers(0, 1 << 40)); b = int(rng.integers(0, 1 << 40)); s = int(rng.integers(0, 5))
        b = (b & ~(0xFF << (8 * s))) | (a & (0xFF << (8 * s)))  # same bucket
        x = a ^ b
        mm = ((x & 0xAAAAAAAAAAAAAAAA) >> 1) | (x & 0x5555555555555555)
        y = scan_word(a, s) ^ scan_word(b, s)
        assert bin((y | (y >> 16)) & 0xFFFF).count("1") == bin(mm).count("1")


def test_image_layouts_and_their_sizes(golden_uniform):
    """The layouts an upload tries, in order, and what each keeps in HBM per site (issl_index_device_bytes needs no
    device): the sections that differ between them (at scale: sorted 152 B per site, compact 92, compact with the slice
    lists in host memory 52; list order 108 / 68, with site table and lists in host memory 25)."""
    n = 8000
    sizes = {}
    for name, opts in {"sorted": {"sorted_layout": 1, "compact": 0, "host_cold": 0}, "compact": {"compact": 1, "host_cold": 0},
                       "compact_cold": {"compact": 1, "host_cold": 1}, "list_esig": {"sorted_layout": 0, "inline_sigs": 1, "host_cold": 0},
                       "list": {"sorted_layout": 0, "inline_sigs": 0, "host_cold": 0}, "host_cold": {"sorted_layout": 0, "host_cold": 1}}.items():
        ix = ca.IsslIndex.open(golden_uniform.issl)
        for k, v in opts.items():
            ix.set_option(k, v)
        sizes[name] = ix.device_bytes()
        ix.close()
    auto = ca.IsslIndex.open(golden_uniform.issl)
    assert auto.device_bytes() == sizes["sorted"]          # what an upload tries first
    auto.close()
    ref = ca.IsslIndex.open(golden_uniform.issl)
    tiles = int(((ref.bucket_sizes() + 2047) // 2048).sum())     # every bucket is padded to whole tiles of 2048 candidates
    ref.close()
    slack = 16 * 256                                             # (sections are 256-byte aligned)
    assert abs((sizes["sorted"] - sizes["compact"]) - 12 * 2048 * tiles) <= slack         # 16-byte records vs 4-byte ids per stream position
    assert abs((sizes["compact"] - sizes["compact_cold"]) - 40 * n) <= slack               # the slice lists
    assert abs((sizes["list_esig"] - sizes["list"]) - 40 * n) <= slack                     # the in-list signatures
    assert abs((sizes["list"] - sizes["host_cold"]) - (48 - 5) * n) <= slack               # site table + lists out, one byte per entry in
    assert abs((sizes["compact_cold"] - sizes["host_cold"]) - (4 * 2048 * tiles + 12 * n - 5 * n)) <= slack + 4 * 1280 * 257 + 256
    bad = ca.IsslIndex.open(golden_uniform.issl)
    bad.set_option("sorted_layout", 0).set_option("compact", 1)
    bad.set_option("inline_sigs", 1)
    with pytest.raises(ca.IsslError):
        ca.IsslIndex.open(golden_uniform.issl).set_option("compact", 2)
    bad.close()


def _libc_f(values):
    """glibc's own printf("%f") of every value (the reference prints its scores with it, isslScoreOfftargets.cpp:517-525)."""
    libc = C.CDLL(None)
    libc.snprintf.restype = C.c_int
    buf = C.create_string_buffer(512)
    out = []
    for v in values:
        k = libc.snprintf(buf, C.c_size_t(512), b"%f", C.c_double(float(v)))
        out.append(buf.raw[:k])
    return out


def test_own_percent_f_is_glibcs_digit_for_digit(golden):
    """issl_format_scores prints "%f" with a formatter of its own (a million lines through printf are as long as their
    scoring).  It must print what glibc prints: the exact binary value rounded to six decimals, ties to even."""
    rng = np.random.default_rng(11)
    ties = np.arange(1, 4001, 2, dtype=np.float64) / 128.0          # k/128 with k odd: x.xxxxxx5 exactly -- the ties
    near = np.concatenate([ties * (1 + 2.0 ** -52), ties * (1 - 2.0 ** -53), np.nextafter(ties, 0), np.nextafter(ties, 1e9)])
    scores = 10000.0 / (100.0 + np.concatenate([rng.exponential(30.0, 200000), rng.exponential(1e6, 20000), [0.0]]))  # :505-506
    special = np.array([0.0, -0.0, 100.0, 99.9999995, 99.99999949999999, 5e-7, 4.9999999999999996e-07, 5.000000000000001e-07,
                        1.5e-6, 2.5e-6, 2.4999999999999998e-06, 1e-300, 5e-324, 2.0 ** 39, 2.0 ** 40 - 0.5, 2.0 ** 40, 1e22, 1.7976931348623157e308,
                        np.inf, -np.inf, np.nan, -1.0, -1e-9, 0.1, 0.3, 1 / 3, 123456.7890125, 0.0078125, 0.0234375, 1e15 + 0.3])
    bits = rng.integers(0, 2 ** 63, size=100000, dtype=np.int64).view(np.float64)   # every exponent, sign bit clear
    vals = np.concatenate([ties, near, scores, special, bits, -bits[:2000]])
    sigs = rng.integers(0, 1 << 40, size=len(vals), dtype=np.uint64)
    want_f = _libc_f(vals)
    for i in rng.integers(0, len(vals), size=3000):   # Python's % is correctly rounded too: a second witness
        if np.isfinite(vals[i]):
            assert want_f[i] == (b"%f" % vals[i]), vals[i]
    seqs = [s.encode() for s in ca.decode_guides(sigs)]
    for threads in (1, 0, 5):
        got = ca.format_scores_native(sigs, vals, vals[::-1].copy(), "and", threads=threads)
        want = b"".join(s + b"\t" + m + b"\t" + c + b"\n" for s, m, c in zip(seqs, want_f, want_f[::-1]))
        assert got == want, threads
    # the method decides which columns are printed (:517-525), as in the reference's golden stdout
    small = slice(0, 50)
    for method, cols in (("mit", (1, 0)), ("cfd", (0, 1)), ("or", (1, 1)), ("avg", (1, 1)), ("bogus", (0, 0))):
        got = ca.format_scores_native(sigs[small], vals[small], vals[small], method)
        want = b"".join(s + b"\t" + (m if cols[0] else b"-1") + b"\t" + (m if cols[1] else b"-1") + b"\n" for s, m in zip(seqs[small], want_f[small]))
        assert got == want, method
    assert ca.format_scores_native(sigs[:0], vals[:0], vals[:0], "and") == b""
    # and the Python restatement the parity tests compare stdout with says the same
    assert ca.format_scores_native(sigs[:5000], scores[:5000], scores[5000:10000], "and").decode() == ca.format_scores(sigs[:5000], scores[:5000], scores[5000:10000], "and")


def test_query_file_reader_threads_and_rules(tmp_path):
    """issl_read_query_file (isslScoreOfftargets.cpp:275-305): lines of seq_len + 1 bytes, any other byte packs as 'A'; large
    files are read by several threads -- same guides, same order."""
    rng = np.random.default_rng(12)
    sigs = rng.integers(0, 1 << 40, size=300_001, dtype=np.uint64)
    text = "".join(s + "\n" for s in ca.decode_guides(sigs))
    path = tmp_path / "q.txt"
    path.write_text(text)
    out, n = C.c_void_p(), C.c_size_t()
    _lib.check(_lib.lib.issl_read_query_file(os.fsencode(path), 20, C.byref(out), C.byref(n)))
    got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n.value,)).copy()
    _lib.lib.issl_free(out)
    assert np.array_equal(got, sigs)
    for bad, code in ((text[:-3], "multiple of the expected line length"), ("", "Failed to read in query file")):
        path.write_text(bad)
        assert _lib.lib.issl_read_query_file(os.fsencode(path), 20, C.byref(out), C.byref(n)) != 0
        assert code in _lib.lib.issl_last_error().decode()
    assert _lib.lib.issl_read_query_file(os.fsencode(tmp_path / "absent"), 20, C.byref(out), C.byref(n)) != 0


def test_cli_without_its_library_fails_loudly(golden, tmp_path):
    """bin/isslScoreOfftargets is host code that loads libissl_hip.so on demand (never when a resident server answers).  Away from
    the library -- a copy of the executable alone -- it says what it tried and exits 1 with nothing on stdout; ISSL_LIBRARY
    points it at the library again (and then it fails for want of a GPU, here)."""
    import shutil
    exe = tmp_path / "isslScoreOfftargets"
    shutil.copy(ROOT / "bin" / "isslScoreOfftargets", exe)
    args = [str(exe), str(golden.issl), str(golden.guides_txt), "4", "75", "and"]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_LIBRARY_PATH", "ISSL_LIBRARY", "ISSL_SERVER")}
    r = subprocess.run(args, capture_output=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 1 and r.stdout == b"" and b"cannot load libissl_hip.so" in r.stderr and b"ISSL_LIBRARY" in r.stderr
    r = subprocess.run(args, capture_output=True, env=dict(env, ISSL_LIBRARY=_lib.LIB_PATH), cwd=str(tmp_path))
    assert r.stdout == b"" and b"cannot load" not in r.stderr
    if not _has_gpu():
        assert r.returncode == 1 and b"no HIP device" in r.stderr
    # usage errors need no library at all
    r = subprocess.run([str(exe), str(golden.issl)], capture_output=True, env=env)
    assert r.returncode == 1 and b"Usage:" in r.stderr


def _other_dlopen_executables():
    """name -> arguments that pass its usage check (g: the golden index, fasta: a small FASTA file, out: a path to write)."""
    sample = ROOT / "tests" / "golden" / "transcripts" / "sample"
    return {
        "isslReportOfftargets": lambda g, fasta, out: [str(g.issl), str(g.guides_txt), "4"],
        "isslLocateOfftargets": lambda g, fasta, out: [str(g.guides_txt), str(fasta)],
        "cracklingGuides": lambda g, fasta, out: [str(fasta)],
        "cracklingBowtie": lambda g, fasta, out: [str(g.guides_txt), str(fasta)],
        "countHitTranscripts": lambda g, fasta, out: ["-a", str(sample / "annotation.gff"), "-c", str(sample / "crackling.csv"), "-o", str(out)],
    }


@pytest.mark.parametrize("name", sorted(_other_dlopen_executables()))
def test_cli_without_its_library_fails_loudly_every_executable(name, golden_uniform, tmp_path):
    """The other five executables load libissl_hip.so through the same loader (csrc/cli_api.hpp), each under its own name:
    a copy of the executable alone says what it tried and exits 1 with nothing on stdout; ISSL_LIBRARY points it at the
    library again (and then it fails for want of a GPU, here)."""
    import shutil
    exe = tmp_path / name
    shutil.copy(ROOT / "bin" / name, exe)
    fasta = tmp_path / "g.fa"
    fasta.write_text(">r1\nACGTACGTACGTACGTACGTACGTAGGTTCCATGCATGCATGCATGCATGCAGG\n")
    out = tmp_path / "out.csv"
    args = [str(exe)] + _other_dlopen_executables()[name](golden_uniform, fasta, out)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_LIBRARY_PATH", "ISSL_LIBRARY", "ISSL_SERVER")}
    r = subprocess.run(args, capture_output=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 1 and r.stdout == b"" and b"cannot load libissl_hip.so" in r.stderr and b"ISSL_LIBRARY" in r.stderr
    assert r.stderr.startswith(name.encode() + b": ") and not out.exists()
    r = subprocess.run(args, capture_output=True, env=dict(env, ISSL_LIBRARY=_lib.LIB_PATH), cwd=str(tmp_path))
    assert b"cannot load" not in r.stderr
    if not _has_gpu():
        assert r.returncode == 1 and b"no HIP device" in r.stderr


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


def _option_table():
    """(key, environment name) of every settable option: the rows of the library's option table."""
    src = (ROOT / "crackling_amd" / "csrc" / "issl_options.cpp").read_text()
    rows = re.findall(r'\{"([a-z_0-9]+)", "(ISSL_[A-Z_0-9]+)"', src)
    assert len(rows) >= 24, rows
    return rows


# (a value inside the option's range, one outside it) for every settable option that can be read back
OPTION_CASES = {"prune": (1, 2), "lanes": (3, 4), "hit_slots": (2, 3), "lean_tail": (0, 2), "small_bin": (0, 2), "scan_events": (1, 3),
                "scan_threads": (768, 63), "scan_blocks": (512, 0), "upload_threads": (3, 33), "upload_chunk_kib": (64, 3),
                "upload_ring_min_kib": (0, -1), "fine_items": (16, -1), "expect_guides": (1000, -1), "scan_generic": (1, 2),
                "stage_timing": (1, 2), "tail_shapes": (0, 2), "item_guides": (64, 7), "raw_chunks": (1000, -1),
                "inline_sigs": (0, 2), "host_cold": (1, -2), "sorted_layout": (0, 2), "compact": (1, -2), "keep_lists": (0, 2)}


def test_every_documented_option_can_be_set_and_read_back(golden_uniform):
    """Every settable option (scan_stamps, a file name, can be set but not read): the header lists it with its environment
    name; it takes a value of its range and gives it back through issl_index_get_option; a value outside the range, or
    one that is not a number, is refused and leaves the option as it was.  No device needed: options live on the handle."""
    header = (ROOT / "include" / "issl_hip.h").read_text()
    rows = _option_table()
    missing = sorted(k for k, env in rows if k not in header or env not in header)
    assert not missing, f"options of the library that the header does not list: {missing}"
    assert set(OPTION_CASES) == {k for k, _ in rows} - {"scan_stamps"}
    ix = ca.IsslIndex.open(golden_uniform.issl)
    try:
        for name, (good, bad) in OPTION_CASES.items():
            before = ix.get_option(name)
            ix.set_option(name, good)
            assert ix.get_option(name) == good, name
            for refused in (bad, "x", "", "99999999999999999999999"):
                if name in ("upload_ring_min_kib", "raw_chunks", "expect_guides", "fine_items") and refused == "99999999999999999999999":
                    continue  # (no upper bound: strtoll's clamp is a value of the range)
                with pytest.raises(ca.IsslError):
                    ix.set_option(name, refused)
                assert ix.get_option(name) == good, (name, refused)
            ix.set_option(name, before)
        ix.set_option("scan_stamps", "")
        with pytest.raises(ca.IsslError):
            ix.get_option("scan_stamps")
    finally:
        ix.close()


WORKSPACE_KEYS = ("ws_cap_guides", "ws_slot_width", "ws_fine_ways", "ws_cap_chunks", "ws_cap_fitems", "ws_lean",
                  "ws_scan_verified", "ws_scan_lds_buffers", "ws_scan_raw_top", "ws_raw_chunks")


def test_workspace_keys_are_read_only_and_zero_before_the_first_batch(golden_uniform):
    """The keys that describe the first lane's scoring workspace: a handle that has scored nothing -- here one without a device
    -- answers 0 for each; issl_index_set_option refuses them with ISSL_E_ARG and leaves them as they were; the header and the
    README list them; they are no rows of the option table (no environment variable sets them)."""
    header = (ROOT / "include" / "issl_hip.h").read_text()
    readme = (ROOT / "README.md").read_text()
    assert not set(WORKSPACE_KEYS) & {k for k, _ in _option_table()}
    ix = ca.IsslIndex.open(golden_uniform.issl)
    try:
        for key in WORKSPACE_KEYS:
            assert key in header and "`%s`" % key in readme, key
            assert ix.get_option(key) == 0, key
            for value in (0, 1, 2048, "x", ""):
                rc = _lib.lib.issl_index_set_option(ix._h, key.encode(), str(value).encode())
                assert rc == -1, (key, value, rc)   # ISSL_E_ARG
                assert b"read-only" in _lib.lib.issl_last_error()
            assert ix.get_option(key) == 0, key
        with pytest.raises(ca.IsslError):
            ix.get_option("ws_nothing")
    finally:
        ix.close()
    for key in ("small_bin", "fine_items", "expect_guides", "scan_events", "upload_threads"):   # settable keys the README had missed
        assert "`%s`" % key in readme, key


_ENV_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import crackling_amd as ca
ix = ca.IsslIndex.open(sys.argv[2])
print(json.dumps({k: ix.get_option(k) for k in sys.argv[3:]}))
ix.close()
"""


def test_every_option_is_read_from_its_environment_variable(golden_uniform):
    """A handle reads every option from its environment variable (ISSL_FORCE_HOST_COLD for host_cold); a value out of
    range there leaves the default in place.  One child process per environment."""
    rows = [(k, env) for k, env in _option_table() if k in OPTION_CASES]
    base = {k: v for k, v in os.environ.items() if not k.startswith("ISSL_")}

    def read(extra):
        run = subprocess.run([sys.executable, "-c", _ENV_CHILD, str(ROOT), str(golden_uniform.issl)] + [k for k, _ in rows],
                             env={**base, **extra}, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        return json.loads(run.stdout.strip().splitlines()[-1])

    defaults = read({})
    good = read({env: str(OPTION_CASES[k][0]) for k, env in rows})
    assert good == {k: OPTION_CASES[k][0] for k, _ in rows}
    assert all(good[k] != defaults[k] for k, _ in rows if OPTION_CASES[k][0] != defaults[k])
    assert read({env: str(OPTION_CASES[k][1]) for k, env in rows}) == defaults
    assert read({env: "x" for _, env in rows}) == defaults


def test_dynamic_symbol_table_is_the_header(tmp_path):
    """libissl_hip.so defines exactly the functions include/issl_hip.h declares in its dynamic symbol table: no internal
    C++ symbol another library in the caller's process could interpose."""
    header = (ROOT / "include" / "issl_hip.h").read_text()
    declared = set(re.findall(r"\b(issl_[a-z_0-9]+)\s*\(", header))
    run = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert run.returncode == 0, f"cannot read the dynamic symbol table: {run.stderr}"
    defined = {line.split()[-1] for line in run.stdout.splitlines() if len(line.split()) == 3 and line.split()[1] in "TtWwiDdBbRrVv"}
    defined = {name.split("@")[0] for name in defined}
    assert declared, "no declarations found in the header"
    assert defined == declared, f"exported but not declared: {sorted(defined - declared)[:20]}; declared but missing: {sorted(declared - defined)}"


_NOMEM_CHILD = r"""
import ctypes as C, resource, sys
lib = C.CDLL(sys.argv[1])
lib.issl_last_error.restype = C.c_char_p
n = 8 << 20
big = b"ACGTACGTACGTACGTACGT\n" * n                      # made before the limit: 176 MB of text
small = b"".join((a + b + c + "A" * 17 + "\n").encode() for a in "ACGT" for b in "ACGT" for c in "ACGT")  # 64 sorted lines
with open("/proc/self/statm") as f:
    vm = int(f.read().split()[0]) * resource.getpagesize()
resource.setrlimit(resource.RLIMIT_AS, (vm + (64 << 20), resource.getrlimit(resource.RLIMIT_AS)[1]))
h = C.c_void_p()
rc = lib.issl_index_build_from_text(big, C.c_size_t(n), C.c_size_t(20), C.c_size_t(8), C.byref(h))
print(rc, lib.issl_last_error().decode(), flush=True)
assert rc == -6 and lib.issl_last_error(), rc                   # ISSL_E_NOMEM, with a message
rc = lib.issl_index_build_from_text(small, C.c_size_t(64), C.c_size_t(20), C.c_size_t(8), C.byref(h))
assert rc == 0, (rc, lib.issl_last_error())
lib.issl_index_close(h)
print("ok", flush=True)
"""


def test_allocation_failure_comes_back_as_an_error_code():
    """The C ABI never throws: an index the process has no memory for is ISSL_E_NOMEM with a message, and the library goes
    on working -- not std::terminate inside the caller's process.  Host-side entry points only (no device is opened); the
    address space is capped after the library has loaded, the threads' stacks at 1 MiB so that a small build still fits."""
    def limits():
        resource.setrlimit(resource.RLIMIT_STACK, (1 << 20, resource.getrlimit(resource.RLIMIT_STACK)[1]))
    run = subprocess.run([sys.executable, "-c", _NOMEM_CHILD, _lib.LIB_PATH], capture_output=True, text=True, timeout=120,
                         preexec_fn=limits)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-2000:]}"
    assert run.stdout.startswith("-6 ") and run.stdout.rstrip().endswith("ok"), run.stdout
