"""CPU: the haplotype part of the C ABI (issl_vcf_indels, issl_haplotypes_*): layouts, names, the version, the VCF reader
against the character-level reader of tests/haplotype_util.py, both capacity rules, the malformed lines, and every refusal
made on the arguments alone."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import haplotype_util as hu
import variant_util as vu
from haplotype_util import VCF, VCF_RECORDS

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_vcf_indels", "issl_haplotypes_open", "issl_haplotypes_open_vcf", "issl_haplotypes_info", "issl_haplotypes_close",
           "issl_haplotypes_search", "issl_haplotypes_search_device", "issl_haplotypes_search_profile",
           "issl_haplotypes_search_profile_device"]
EXE = str(ROOT / "bin" / "isslSearchGenome")
FASTA = str(ROOT / "tests" / "golden" / "extract" / "multi.fa")


def _error():
    return _lib.lib.issl_last_error().decode(errors="replace")


def test_symbols_are_declared_exported_and_bound_and_the_version_stays():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, HEADER), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    for name in ("haplotypes", "haplotypes_vcf"):
        assert callable(getattr(ca.Genome, name)), name
    for name in ("search", "search_profile", "search_device", "search_profile_device", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(ca.Haplotypes, name)), name
    for name in ("INDEL_DTYPE", "HAPLOTYPE_HIT_DTYPE", "Haplotypes", "vcf_indels"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert _lib.lib.issl_abi_version() == 6 and re.search(r"#define ISSL_ABI_VERSION 6\b", HEADER)
    assert re.search(r"#define ISSL_INDEL_MAX_ALLELE 65535\b", HEADER) and hu.MAX_ALLELE == 65535


def test_struct_layouts_agree():
    assert (C.sizeof(_lib.Indel), C.sizeof(_lib.VcfIndelCounts), C.sizeof(_lib.HaplotypeHit)) == (32, 56, 48)
    names = ("pos", "record", "ref_len", "alt_len", "ref_at", "alt_at", "reserved")
    offsets = [0, 8, 12, 16, 20, 24, 28]
    assert [getattr(_lib.Indel, k).offset for k in names] == offsets
    assert ca.INDEL_DTYPE.itemsize == 32 and ca.INDEL_DTYPE.names == names and [ca.INDEL_DTYPE.fields[k][1] for k in names] == offsets
    names = ("pos", "site", "record", "query", "mism", "strand", "dist", "n_var", "reserved", "indel", "edit_at")
    offsets = [0, 8, 24, 28, 32, 36, 37, 38, 39, 40, 44]
    assert [getattr(_lib.HaplotypeHit, k).offset for k in names] == offsets
    assert ca.HAPLOTYPE_HIT_DTYPE.itemsize == 48 and ca.HAPLOTYPE_HIT_DTYPE.names == names
    assert [ca.HAPLOTYPE_HIT_DTYPE.fields[k][1] for k in names] == offsets and ca.HAPLOTYPE_HIT_DTYPE["edit_at"] == np.dtype("<i4")
    assert [n for n, _ in _lib.VcfIndelCounts._fields_] == ["lines", "indels", "alleles_skipped", "no_allele", "unknown_chrom",
                                                             "beyond_record", "too_long"]
    assert re.search(r"typedef struct \{ uint64_t lines, indels, alleles_skipped, no_allele, unknown_chrom, beyond_record, too_long; \} "
                     r"issl_vcf_indel_counts;", HEADER)
    assert re.search(r"uint8_t strand, dist, n_var, reserved; uint32_t indel; int32_t edit_at; \} issl_haplotype_hit;", HEADER)


# ---- issl_vcf_indels ---------------------------------------------------------------------------------------------------

def _same(vcf, records):
    want, want_text, want_counts = hu.vcf_indels(vcf, records)
    got, text, counts = ca.vcf_indels(vcf, records)
    assert got.dtype == ca.INDEL_DTYPE and got.tobytes() == want.tobytes() and text == want_text and counts == want_counts
    return got, text, counts


def test_vcf_reader_equals_the_character_level_reader():
    indels, text, counts = _same(VCF, VCF_RECORDS)
    # upper and lower case kept as the file has them; \r\n; no final line end; multi-allelic lines mixing a SNP, indels,
    # <DEL>, * and .; REF past the record's end; CHROM up to the first blank
    assert len(indels) == 9 and text.startswith(b"GAGaaccaAG") and indels["record"].tolist() == [0] * 7 + [1, 1]
    assert counts == dict(lines=14, indels=9, alleles_skipped=12, no_allele=4, unknown_chrom=1, beyond_record=3, too_long=0)
    _same(b"", VCF_RECORDS)
    _same(b"\n\r\n#only a comment", VCF_RECORDS)
    _same(VCF.replace(b"\n", b"\r\n"), VCF_RECORDS)
    _same(VCF + b"\n", VCF_RECORDS)
    _same(VCF, [])
    _same(VCF, [(b"chr2", 3), (b"chr1\x0bvt", 8), (b" chr1", 100)])
    _same(b"chr1\t99999999999999999999999\t.\tAC\tA\n", VCF_RECORDS)  # a POS no record reaches
    rng = np.random.default_rng(6)
    lines = []
    for _ in range(400):
        chrom = [b"chr1", b"chr2", b"chr3", b"chr1 the first"][int(rng.integers(0, 4))]
        alleles = [b"A", b"C", b"AC", b"ac", b"ACG", b"GT", b"t", b"ACGTT", b"<INS>", b"*", b".", b"N", b"AN", b""]
        alt = b",".join(alleles[int(i)] for i in rng.integers(0, len(alleles), size=int(rng.integers(1, 4))))
        lines.append(b"\t".join([chrom, b"%d" % rng.integers(0, 25), b".", alleles[int(rng.integers(0, 10))], alt, b"50", b"PASS"]))
    indels, _, counts = _same(b"\n".join(lines) + b"\n", VCF_RECORDS)
    assert len(indels) > 40 and all(counts[k] > 5 for k in counts if k != "too_long")


def test_an_allele_of_65536_bases_is_too_long():
    records = [(b"big", 70000)]
    long = b"AC" * 32768  # 65536 bases
    vcf = (b"big\t1\t.\tA\tA" + long[:65535] + b",A" + long[:65534] + b",<DEL>\n"   # ALT of 65536: too long; of 65535: taken
           b"big\t2\t.\t" + long + b"\tA,C\n"                                          # REF of 65536: both alleles too long
           b"big\t3\t.\t" + long[:65535] + b"\tA\n")                                   # REF of 65535: taken
    indels, text, counts = _same(vcf, records)
    assert counts == dict(lines=3, indels=2, alleles_skipped=1, no_allele=1, unknown_chrom=0, beyond_record=0, too_long=3)
    assert indels["alt_len"].tolist() == [65535, 1] and indels["ref_len"].tolist() == [1, 65535] and len(text) == 2 * 65536


def test_a_malformed_vcf_line_is_named():
    for bad, line in ((VCF + b"\nchr1\t4\t.\tAC\n", 18), (b"#h\nchr1\t4\t.\tAC\tA\nchr1\tfour\t.\tAC\tA\n", 3), (b"chr1\t-4\t.\tAC\tA\n", 1),
                      (b"chr1\t\t.\tAC\tA\n", 1), (b"chr1 4 . AC A\n", 1), (b"chrX\t4\t.\tAC\n", 1), (b"chr1\t4 \t.\tAC\tA\n", 1)):
        with pytest.raises(vu.Malformed) as m:
            hu.vcf_indels(bad, VCF_RECORDS)
        assert m.value.line == line
        with pytest.raises(ca.IsslError) as e:
            ca.vcf_indels(bad, VCF_RECORDS)
        assert e.value.code == -1 and ("line %d:" % line) in e.value.message, e.value.message
    for bad, what in ((b"chr1\t4\t.\tAC\n", "fewer than five"), (b"chr1\tx\t.\tAC\tA\n", "POS is not a number")):
        with pytest.raises(ca.IsslError) as e:
            ca.vcf_indels(bad, VCF_RECORDS)
        assert what in e.value.message


def test_both_capacity_rules_and_null_arguments():
    lib = _lib.lib
    names = (C.c_char_p * 3)(*[n for n, _ in VCF_RECORDS])
    lens = (C.c_size_t * 3)(*[len(n) for n, _ in VCF_RECORDS])
    lengths = (C.c_uint64 * 3)(*[length for _, length in VCF_RECORDS])
    want, want_text, _ = hu.vcf_indels(VCF, VCF_RECORDS)
    n, nb, counts = C.c_size_t(), C.c_size_t(), _lib.VcfIndelCounts()
    head = (VCF, len(VCF), names, lens, lengths, 3)

    def fresh():
        return np.full(9 * 32, 0xA5, dtype=np.uint8).view(ca.INDEL_DTYPE), C.create_string_buffer(b"\xA5" * len(want_text), len(want_text))

    out, text = fresh()  # one entry short: nothing is written to either buffer
    assert lib.issl_vcf_indels(*head, out.ctypes.data, 8, C.byref(n), text, len(want_text), C.byref(nb), C.byref(counts)) == 0
    assert (n.value, nb.value, counts.indels) == (9, len(want_text), 9)
    assert (out.view(np.uint8) == 0xA5).all() and text.raw == b"\xA5" * len(want_text)
    out, text = fresh()  # one allele byte short: the same
    assert lib.issl_vcf_indels(*head, out.ctypes.data, 9, C.byref(n), text, len(want_text) - 1, C.byref(nb), None) == 0
    assert (n.value, nb.value) == (9, len(want_text))
    assert (out.view(np.uint8) == 0xA5).all() and text.raw == b"\xA5" * len(want_text)
    assert lib.issl_vcf_indels(*head, out.ctypes.data, 9, C.byref(n), text, len(want_text), C.byref(nb), None) == 0
    assert out.tobytes() == want.tobytes() and text.raw == want_text
    assert lib.issl_vcf_indels(None, 5, names, lens, lengths, 3, None, 0, C.byref(n), None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(VCF, len(VCF), None, lens, lengths, 3, None, 0, C.byref(n), None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(VCF, len(VCF), names, None, lengths, 3, None, 0, C.byref(n), None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(VCF, len(VCF), names, lens, None, 3, None, 0, C.byref(n), None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(*head, None, 0, None, None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(*head, None, 0, C.byref(n), None, 0, None, None) == -1
    assert lib.issl_vcf_indels(*head, None, 2, C.byref(n), None, 0, C.byref(nb), None) == -1
    assert lib.issl_vcf_indels(*head, None, 0, C.byref(n), None, 2, C.byref(nb), None) == -1 and "null" in _error()
    assert lib.issl_vcf_indels(None, 0, None, None, None, 0, None, 0, C.byref(n), None, 0, C.byref(nb), None) == 0 and n.value == 0


# ---- refusals on the arguments alone -------------------------------------------------------------------------------------

def test_null_arguments_come_before_any_device_work():
    lib = _lib.lib
    g = C.c_void_p(0x1234)  # a sentinel handle that is never dereferenced
    pat, q = ca.search_prepare("NNNNNGG", ["ACGTNNN"])
    offs, hits, counts = np.zeros(2, dtype=np.uint64), np.zeros(4, dtype=ca.HAPLOTYPE_HIT_DTYPE), np.zeros(8, dtype=np.uint64)
    indel, tot, h = np.zeros(1, dtype=ca.INDEL_DTYPE), C.c_size_t(), C.c_void_p(0x5678)
    P, Q, O, H, K = C.byref(pat), q.ctypes.data, offs.ctypes.data, hits.ctypes.data, counts.ctypes.data
    assert lib.issl_haplotypes_open(None, indel.ctypes.data, 1, b"AC", 2, 7, C.byref(h)) == -1 and h.value is None
    assert lib.issl_haplotypes_open(g, None, 1, b"AC", 2, 7, C.byref(h)) == -1
    assert lib.issl_haplotypes_open(g, indel.ctypes.data, 1, None, 2, 7, C.byref(h)) == -1
    assert lib.issl_haplotypes_open(g, indel.ctypes.data, 1, b"AC", 2, 7, None) == -1
    assert lib.issl_haplotypes_open_vcf(None, VCF, len(VCF), 7, None, C.byref(h)) == -1
    assert lib.issl_haplotypes_open_vcf(g, None, 4, 7, None, C.byref(h)) == -1
    assert lib.issl_haplotypes_open_vcf(g, VCF, len(VCF), 7, None, None) == -1
    assert lib.issl_haplotypes_info(None, C.byref(C.c_uint64()), C.byref(C.c_uint64()), C.byref(C.c_uint32())) == -1 and lib.issl_haplotypes_close(None) == 0
    assert lib.issl_haplotypes_search(None, P, Q, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_haplotypes_search(g, None, Q, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_haplotypes_search(g, P, None, 1, 1, 1, O, H, 4, C.byref(tot)) == -1
    assert lib.issl_haplotypes_search(g, P, Q, 1, 1, 1, None, H, 4, C.byref(tot)) == -1
    assert lib.issl_haplotypes_search(g, P, Q, 1, 1, 1, O, None, 4, C.byref(tot)) == -1
    assert lib.issl_haplotypes_search(g, P, Q, 1, 1, 1, O, H, 4, None) == -1
    assert lib.issl_haplotypes_search_device(None, P, Q, 1, 1, 1, O, H, 4, C.byref(tot), None) == -1
    assert lib.issl_haplotypes_search_device(g, P, Q, 1, 1, 1, O, None, 4, C.byref(tot), None) == -1
    assert lib.issl_haplotypes_search_profile(None, P, Q, 1, 1, 1, K) == -1
    assert lib.issl_haplotypes_search_profile(g, P, Q, 1, 1, 1, None) == -1
    assert lib.issl_haplotypes_search_profile_device(g, None, Q, 1, 1, 1, K, None) == -1
    assert lib.issl_haplotypes_search_profile_device(g, P, None, 1, 1, 1, K, None) == -1 and "null" in _error()


# ---- the executable -----------------------------------------------------------------------------------------------------

def test_cli_usage_errors(tmp_path):
    good = tmp_path / "queries.txt"
    good.write_text("ACGTACGTACGTACGTACGTNNN\n")
    vcf = tmp_path / "file.vcf"
    vcf.write_bytes(VCF)
    pam = "NNNNNNNNNNNNNNNNNNNNNGG"
    for args in (["--indel-vcf"], [pam, str(good), "4", FASTA, "--indel-vcf"],
                 ["--indel-vcf", str(vcf), "--guide", "0:20", pam, str(good), "4", FASTA],
                 ["--indel-vcf", str(vcf), pam, str(good), "4"]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr, args
    assert b"[--indel-vcf FILE]" in subprocess.run([EXE], capture_output=True).stderr
    r = subprocess.run([EXE, "--indel-vcf", str(tmp_path / "nope.vcf"), pam, str(good), "4", FASTA], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"nope.vcf" in r.stderr and b"Usage" not in r.stderr
