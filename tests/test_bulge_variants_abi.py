"""CPU: the C ABI of the bulge search on a variant-aware text (issl_genome_search_bulges_variants*): names, the 48-byte row
in the header, in ctypes and in the dtype, every refusal made on the arguments alone through all four entry points, and
bin/isslSearchGenome's --guide-variants and --guide-vcf."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np

import crackling_amd as ca
from crackling_amd import _lib
from variant_util import VCF

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_genome_search_bulges_variants", "issl_genome_search_bulges_variants_device", "issl_genome_search_bulges_variants_profile",
           "issl_genome_search_bulges_variants_profile_device"]
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
    for name in ("search_bulges_variants", "search_bulges_variants_profile", "search_bulges_variants_device",
                 "search_bulges_variants_profile_device"):
        assert callable(getattr(ca.Genome, name))
    assert "BULGE_VARIANT_HIT_DTYPE" in ca.__all__ and hasattr(ca, "BULGE_VARIANT_HIT_DTYPE")
    assert "not offered" not in HEADER  # the sentence the definition replaces


def test_struct_layout_agrees():
    m = re.search(r"typedef struct \{([^}]*)\}\s*issl_bulge_variant_hit;", HEADER)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "uint64_t pos; uint32_t site[4]; uint32_t record; uint32_t query; uint32_t mism; uint8_t strand; uint8_t dist; uint8_t n_var; "
        "int8_t bulge; uint8_t at; uint8_t reserved[7];")
    H = _lib.BulgeVariantHit
    names = ("pos", "site", "record", "query", "mism", "strand", "dist", "n_var", "bulge", "at", "reserved")
    offsets = [0, 8, 24, 28, 32, 36, 37, 38, 39, 40, 41]
    assert C.sizeof(H) == 48 and [getattr(H, k).offset for k in names] == offsets
    D = ca.BULGE_VARIANT_HIT_DTYPE
    assert D.itemsize == 48 and D.names == names and [D.fields[k][1] for k in names] == offsets
    assert D["bulge"] == np.int8 and D["at"] == np.uint8 and D["site"].shape == (4,) and D["reserved"].shape == (7,)
    # the variant search's row up to n_var: D = R = 0 gives the same leading bytes
    assert [ca.VARIANT_HIT_DTYPE.fields[k][1] for k in names[:8]] == offsets[:8]


def _error():
    return _lib.lib.issl_last_error().decode(errors="replace")


def test_errors_come_before_any_device_work():
    """A sentinel handle that is never dereferenced: every refusal is made on the arguments alone, by all four entry points."""
    lib = _lib.lib
    g = C.c_void_p(0x1234)
    pat, q = ca.search_prepare(NGG, ["ACGTACGTACGTACGTACGTNNN"])
    offs = np.zeros(2, dtype=np.uint64)
    hits = np.zeros(4, dtype=ca.BULGE_VARIANT_HIT_DTYPE)
    counts = np.zeros(7 * 24, dtype=np.uint64)
    tot = C.c_size_t()
    P, Q, O, H, K = C.byref(pat), q.ctypes.data, offs.ctypes.data, hits.ctypes.data, counts.ctypes.data

    def every_entry(bulges, max_dist=1, max_variants=1, pat_ref=P, queries=Q):
        bg = _lib.SearchBulges(*bulges)
        return [lib.issl_genome_search_bulges_variants(g, pat_ref, C.byref(bg), queries, 1, max_dist, max_variants, O, H, 4, C.byref(tot)),
                lib.issl_genome_search_bulges_variants_device(g, pat_ref, C.byref(bg), queries, 1, max_dist, max_variants, O, H, 4,
                                                              C.byref(tot), None),
                lib.issl_genome_search_bulges_variants_profile(g, pat_ref, C.byref(bg), queries, 1, max_dist, max_variants, K),
                lib.issl_genome_search_bulges_variants_profile_device(g, pat_ref, C.byref(bg), queries, 1, max_dist, max_variants, K, None)]

    refused = [-1] * 4
    # max_variants outside 0..L
    for v in (-1, 24, 1 << 20):
        assert every_entry((0, 20, 1, 1), max_variants=v) == refused and "max_variants" in _error(), v
    # every ISSL_E_ARG of the bulge search: the span
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
    bg = _lib.SearchBulges(0, 20, 1, 1)
    G = C.byref(bg)
    for sig, care in ((1 << 46, 0), (0, 1 << 47), (0, 1), (2, 0)):
        bq = np.array([(sig, care)], dtype=ca.SEARCH_QUERY_DTYPE)
        assert lib.issl_genome_search_bulges_variants(g, P, G, bq.ctypes.data, 1, 1, 1, O, H, 4, C.byref(tot)) == -1 and "query 0" in _error()
        assert lib.issl_genome_search_bulges_variants_profile(g, P, G, bq.ctypes.data, 1, 1, 1, K) == -1 and "query 0" in _error()
    # NULLs
    assert lib.issl_genome_search_bulges_variants(None, P, G, Q, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, None, G, Q, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, P, None, Q, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, P, G, None, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, P, G, Q, 1, 1, 1, None, H, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, P, G, Q, 1, 1, 1, O, None, 4, C.byref(tot)) == -1
    assert lib.issl_genome_search_bulges_variants(g, P, G, Q, 1, 1, 1, O, H, 4, None) == -1
    assert lib.issl_genome_search_bulges_variants_device(None, P, G, Q, 1, 1, 1, O, H, 4, C.byref(tot), None) == -1
    assert lib.issl_genome_search_bulges_variants_device(g, P, None, Q, 1, 1, 1, O, H, 4, C.byref(tot), None) == -1
    assert lib.issl_genome_search_bulges_variants_device(g, P, G, Q, 1, 1, 1, O, None, 4, C.byref(tot), None) == -1
    assert lib.issl_genome_search_bulges_variants_profile(g, P, None, Q, 1, 1, 1, K) == -1
    assert lib.issl_genome_search_bulges_variants_profile(g, P, G, Q, 1, 1, 1, None) == -1
    assert lib.issl_genome_search_bulges_variants_profile_device(g, P, None, Q, 1, 1, 1, K, None) == -1
    assert lib.issl_genome_search_bulges_variants_profile_device(g, P, G, None, 1, 1, 1, K, None) == -1
    assert "null" in _error()


def test_cli_usage_and_argument_errors(tmp_path):
    good = tmp_path / "queries.txt"
    good.write_text("ACGTACGTACGTACGTACGTNNN\n")
    vcf = tmp_path / "file.vcf"
    vcf.write_bytes(VCF)
    tail = [NGG, str(good), "2", FASTA]
    # either option without --guide, an option without its value, and the old pair next to --guide
    for args in (["--guide-variants", "2"] + tail, ["--guide-vcf", str(vcf)] + tail, ["--profile", "--guide-variants", "2"] + tail,
                 ["--variants", "2", "--guide-variants", "2"] + tail, ["--guide", "0:20", "--guide-variants"], ["--guide", "0:20", "--guide-vcf"],
                 ["--guide", "0:20"] + tail + ["--guide-variants"], ["--guide", "0:20", "--guide-variants", "2", "--variants", "2"] + tail,
                 ["--guide", "0:20", "--guide-vcf", str(vcf), "--vcf", str(vcf)] + tail):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr, args
    usage = subprocess.run([EXE], capture_output=True).stderr
    assert b"[--guide-variants N] [--guide-vcf FILE]" in usage and b"[--variants N] [--vcf FILE]" in usage
    guide = ["--guide", "0:20"]
    for args, message in ((guide + ["--guide-variants", "24"] + tail, b"--guide-variants '24'"),
                          (guide + ["--guide-variants", "-1"] + tail, b"--guide-variants '-1'"),
                          (guide + ["--guide-variants", "two"] + tail, b"--guide-variants 'two'"),
                          (guide + ["--guide-variants", ""] + tail, b"--guide-variants ''"),
                          (guide + ["--guide-vcf", str(tmp_path / "nope.vcf")] + tail, b"cannot open"),
                          (["--guide", "4:20", "--guide-variants", "2"] + tail, b"span (4, 20)"),
                          (guide + ["--dna-bulge", "4", "--guide-variants", "2"] + tail, b"max_dna 4"),
                          (guide + ["--guide-variants", "2", NGG, str(good), "2", str(tmp_path / "nope.fa")], None)):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr and b"Usage" not in r.stderr, args
        assert message is None or message in r.stderr, (args, r.stderr)
    if not _has_gpu():
        for mode in ([], ["--profile"]):
            r = subprocess.run([EXE] + mode + guide + ["--guide-variants", "2", "--guide-vcf", str(vcf)] + tail, capture_output=True)
            assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr
