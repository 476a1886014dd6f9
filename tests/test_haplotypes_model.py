"""CPU: the model of the search on the ALT haplotypes of indels (tests/haplotype_util.py).  strips() -- what the library
builds -- equals whole_record() -- the definition -- on random small cases; rows written out by hand pin both; and the
header the kernels include runs under AddressSanitizer + UBSan (tools/haplotypes_sanitize.cpp) and reads the VCF as the
character-level reader does."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import haplotype_util as hu
import variant_util as vu

ROOT = pathlib.Path(__file__).resolve().parent.parent


def random_text(rng, n, codes="AC"):
    return "".join(codes[i] for i in rng.integers(0, len(codes), size=n)).encode()


def random_case(rng):
    """-> (records, indels, alleles, pattern, queries, max_dist, max_variants): one to three short records over two
    bases and a few ambiguity codes, one to three edits of every kind, W from 1 to 8."""
    W = int(rng.integers(1, 9))
    records = [(b"r%d" % k, random_text(rng, int(rng.integers(1, 41)), "AACCRYN"[:int(rng.choice([2, 4, 6, 7]))]))
               for k in range(int(rng.integers(1, 4)))]
    entries = []
    while len(entries) < int(rng.integers(1, 4)):
        r = int(rng.integers(0, len(records)))
        seq = records[r][1]
        pos = int(rng.integers(0, len(seq)))
        ref = random_text(rng, int(rng.integers(1, min(4, len(seq) - pos) + 1)))  # (the model does not look at REF's bases)
        alt = random_text(rng, int(rng.integers(1, 6)))
        if rng.random() < 0.3:
            alt = ref[:1] + alt          # an anchor base
        if rng.random() < 0.3:
            alt = alt + ref[-1:]         # a shared suffix
        if rng.random() < 0.2:
            alt = ref[:int(rng.integers(1, len(ref) + 1))]  # a deletion behind what stays
        if alt != ref:
            entries.append((r, pos, ref, alt if rng.random() < 0.8 else alt.lower()))
    indels, alleles = hu.make_indels(entries)
    pattern = "".join("NNNNMR"[int(rng.integers(0, 6))] for _ in range(W))
    queries = ["N" * W, random_text(rng, W).decode(), random_text(rng, W, "ACN").decode()]
    return records, indels, alleles, pattern, queries, int(rng.integers(0, min(W, 2) + 1)), int(rng.integers(0, W + 1))


def test_strips_equal_the_whole_record_definition():
    rng = np.random.default_rng(20)
    rows_seen = inside = junctions = 0
    for _ in range(2500):
        case = random_case(rng)
        want_off, want_rows, want_prof = hu.whole_record(*case)
        off, rows, prof = hu.strips(*case)
        assert off.tobytes() == want_off.tobytes() and prof.tobytes() == want_prof.tobytes(), case
        assert rows.tobytes() == want_rows.tobytes(), case
        rows_seen += len(rows)
        inside += int((rows["edit_at"] < 0).sum())
        junctions += sum(1 for _, _, r, a in hu.edits(case[1], case[2]) if not a)
    assert rows_seen > 20000 and inside > 500 and junctions > 300  # the cases are not empty ones


def tuples(rows, L):
    return [(int(r["query"]), int(r["indel"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["dist"]), int(r["edit_at"]),
             vu.site_text(r["site"], L, r["mism"])) for r in rows]


RECORD = [(b"one", b"AACCGGTTAC")]


@pytest.mark.parametrize("entry, query, want", [
    # CG > C at 3: one G of GG goes; p = 4, the junction lies between hap[3] and hap[4] of AACC|GTTAC
    ((0, 3, "CG", "C"), "CGT", [(0, 0, 0, 3, 0, 0, 1, "CGT")]),
    # A > ATG at 1: TG goes in at p = 2, AA|TG|CCGGTTAC; the window GCC starts inside the insertion
    ((0, 1, "A", "ATG"), "GCC", [(0, 0, 0, 2, 0, 0, -1, "GCC")]),
    # the same, the window ATG: one base ahead of the insertion
    ((0, 1, "a", "atg"), "ATG", [(0, 0, 0, 1, 0, 0, 1, "ATG")]),
    # GGT > CA at 4: AACC|CA|TAC; strand 1 reads CAT as ATG, the window starts at the edit
    ((0, 4, "GGT", "CA"), "ATG", [(0, 0, 0, 4, 1, 0, 0, "ATG")]),
    # every window of that haplotype that overlaps the edit, both strands: CCC CCA CAT ATA at 2, 3, 4, 4
    ((0, 4, "GGT", "CA"), "NNN", [(0, 0, 0, 2, 0, 0, 2, "CCC"), (0, 0, 0, 2, 1, 0, 2, "GGG"), (0, 0, 0, 3, 0, 0, 1, "CCA"),
                                  (0, 0, 0, 3, 1, 0, 1, "TGG"), (0, 0, 0, 4, 0, 0, 0, "CAT"), (0, 0, 0, 4, 1, 0, 0, "ATG"),
                                  (0, 0, 0, 4, 0, 0, -1, "ATA"), (0, 0, 0, 4, 1, 0, -1, "TAT")]),
])
def test_rows_written_out_by_hand(entry, query, want):
    indels, alleles = hu.make_indels([entry])
    for model in (hu.whole_record, hu.strips):
        off, rows, prof = model(RECORD, indels, alleles, "NNN", [query], 0, 0)
        assert tuples(rows, 3) == want and off.tolist() == [0, len(want)] and prof.tolist() == [[len(want)]]


def test_the_reader_counts_every_kind_of_line():
    indels, alleles, counts = hu.vcf_indels(hu.VCF, hu.VCF_RECORDS)
    got = [(int(d["record"]), int(d["pos"]), alleles[int(d["ref_at"]):int(d["ref_at"]) + int(d["ref_len"])],
            alleles[int(d["alt_at"]):int(d["alt_at"]) + int(d["alt_len"])]) for d in indels]
    assert got == [(0, 2, b"GA", b"G"), (0, 4, b"a", b"acc"), (0, 4, b"a", b"AG"), (0, 6, b"AT", b"CG"), (0, 7, b"C", b"CT"),
                   (0, 7, b"C", b"CTT"), (0, 11, b"ACG", b"T"), (1, 8, b"AC", b"A"), (1, 8, b"AC", b"ACGTACGT")]
    assert counts == dict(lines=14, indels=9, alleles_skipped=12, no_allele=4, unknown_chrom=1, beyond_record=3, too_long=0)


def test_text_header_under_sanitizers(tmp_path):
    """tools/haplotypes_sanitize.cpp: trim, layout, strip bytes and row mapping of the header against character loops, and
    its VCF reader on every truncation of the file with one line of every kind and on corrupted copies, as a stand-alone
    program under AddressSanitizer + UBSan; what it reads from the whole file is what the character-level reader reads."""
    exe = tmp_path / "haplotypes_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "haplotypes_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    vcf = tmp_path / "file.vcf"
    vcf.write_bytes(hu.VCF)
    args = [str(exe), str(vcf)]
    for name, length in hu.VCF_RECORDS:
        args += [name.decode(), str(length)]
    run = subprocess.run(args, capture_output=True, text=True,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[0].startswith("layout ok ") and int(lines[0].split()[2]) > 10000
    indels, alleles, counts = hu.vcf_indels(hu.VCF, hu.VCF_RECORDS)
    want = ["indel %d %d %s %s" % (d["record"], d["pos"], alleles[int(d["ref_at"]):int(d["ref_at"]) + int(d["ref_len"])].decode(),
                                   alleles[int(d["alt_at"]):int(d["alt_at"]) + int(d["alt_len"])].decode()) for d in indels]
    want.append("counts " + " ".join(str(counts[k]) for k in ("lines", "indels", "alleles_skipped", "no_allele", "unknown_chrom",
                                                               "beyond_record", "too_long")))
    assert lines[1:-1] == want
    assert lines[-1] == "vcf ok %d" % (len(hu.VCF) + 1 + 3000)
