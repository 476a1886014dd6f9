"""CPU: the model the variant search tests take their expected rows from (tests/variant_util.py), pinned to the plain
search's model, to an enumeration of every sequence a window stands for, to rows written out by hand -- and the plane
functions and the VCF reader of crackling_amd/csrc/issl_variants_text.hpp pinned to the model through a stand-alone CPU
program under AddressSanitizer + UBSan (tools/variants_sanitize.cpp)."""
import itertools
import pathlib
import re
import subprocess

import numpy as np
import pytest

import search_util as su
import variant_util as vu
from variant_util import VCF, VCF_RECORDS

ROOT = pathlib.Path(__file__).resolve().parent.parent


def random_text(rng, n, codes="ACGT"):
    return "".join(codes[i] for i in rng.integers(0, len(codes), size=n))


def with_codes(rng, text, every, codes="RYSWKMBDHV"):
    """`text` with an ambiguity code at about one position in `every`."""
    text = list(text)
    for i in np.flatnonzero(rng.random(len(text)) < 1.0 / every):
        text[i] = codes[int(rng.integers(0, len(codes)))]
    return "".join(text)


@pytest.mark.parametrize("pattern", ["N" * 21 + "GG", "TTTV" + "N" * 8, "N", "NRYSWKMBDHVN"])
def test_max_variants_0_and_clean_text_equal_the_plain_model(pattern):
    rng = np.random.default_rng(len(pattern))
    L = len(pattern)
    clean = random_text(rng, 3000)
    coded = with_codes(rng, clean, 40)
    queries = ["N" * L, random_text(rng, L), clean[100:100 + L], su.revcomp(clean[200:200 + L]), random_text(rng, L, "ACGTN")]
    for text, limits in ((coded + "N" + clean[:50], (0,)), (clean + "NN" + clean[:40], (0, 1, L))):
        records = [(b"r0", text[:1500].encode()), (b"r1 x", text[1500:].encode())]
        off, rows, prof = su.brute_force(records, pattern, queries, min(L, 3))
        assert len(rows) > 0
        for mv in limits:
            v_off, v_rows, v_prof = vu.brute_force(records, pattern, queries, min(L, 3), mv)
            assert v_off.tobytes() == off.tobytes() and v_prof.tobytes() == prof.tobytes()
            assert v_rows.tobytes() == vu.from_plain(rows, L).tobytes() and not v_rows["n_var"].any()


def test_per_position_definition_equals_the_enumeration():
    """dist is the least plain-model distance over every sequence the window stands for that the pattern admits, and the
    window-strand is absent exactly when none is admitted: random windows with up to 3 codes, patterns restricted inside
    and outside the compared span."""
    rng = np.random.default_rng(2024)
    seen_absent = seen_forbidden = 0
    for trial in range(120):
        L = int(rng.integers(4, 11))
        window = list(random_text(rng, L))
        for i in rng.choice(L, size=int(rng.integers(0, 4)), replace=False):
            window[i] = "RYSWKMBDHV"[int(rng.integers(0, 10))]
        window = "".join(window)
        pattern = "".join("ACGTRYSWKMBDHV"[int(rng.integers(0, 14))] if rng.random() < 0.3 else "N" for _ in range(L))
        query = "".join("N" if rng.random() < 0.3 else "ACGT"[int(rng.integers(0, 4))] for _ in range(L))
        records = [(b"w", window.encode())]
        _, rows, _ = vu.brute_force(records, pattern, [query], L, L)
        got = {int(r["strand"]): r for r in rows}
        spelled = ["".join(s) for s in itertools.product(*[su.IUPAC[c] for c in window])]
        for strand in (0, 1):
            best = None
            for s in spelled:
                _, plain, _ = su.brute_force([(b"w", s.encode())], pattern, [query], L)
                for r in plain[plain["strand"] == strand]:
                    best = int(r["dist"]) if best is None else min(best, int(r["dist"]))
            if best is None:
                assert strand not in got
                seen_absent += 1
            else:
                assert strand in got and int(got[strand]["dist"]) == best, (window, pattern, query, strand)
                assert int(got[strand]["n_var"]) == sum(len(su.IUPAC[c]) > 1 for c in window)
                assert bin(int(got[strand]["mism"])).count("1") == best
        seen_forbidden += any(pattern[i] != "N" and query[i] != "N" for i in range(L))
    assert seen_absent > 10 and seen_forbidden > 10


COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
        "D": "H", "H": "D"}


@pytest.mark.parametrize("code", sorted(COMP))
def test_every_text_code_at_length_one(code):
    """Pattern <base>, query N, in the one-base text <code>: strand 0 where the code holds the base, strand 1 where its
    complement does; the site is the set the strand reads."""
    for base in "ACGT":
        _, rows, _ = vu.brute_force([(b"r", code.encode())], base, ["N"], 0, 1)
        want = []
        if base in su.IUPAC[code]:
            want.append((0, 0, 0, 0, 0, int(len(su.IUPAC[code]) > 1), code))
        if base in su.IUPAC[COMP[code]]:
            want.append((0, 0, 0, 1, 0, int(len(su.IUPAC[code]) > 1), COMP[code]))
        assert vu.as_tuples(rows, 1) == want
    # the query's base against the set: a match when it is inside
    _, rows, _ = vu.brute_force([(b"r", code.encode())], "N", ["A"], 1, 1)
    assert [(r[3], r[4]) for r in vu.as_tuples(rows, 1)] == [(0, int("A" not in su.IUPAC[code])), (1, int("A" not in su.IUPAC[COMP[code]]))]
    # with max_variants = 0 an ambiguous code is no window
    assert len(vu.brute_force([(b"r", code.encode())], "N", ["N"], 0, 0)[1]) == (2 if len(su.IUPAC[code]) == 1 else 0)


def test_n_in_the_text_gives_nothing():
    assert len(vu.brute_force([(b"r", b"N")], "N", ["N"], 1, 1)[1]) == 0
    assert vu.as_tuples(vu.brute_force([(b"r", b"ACNRTA")], "NNN", ["NNN"], 0, 3)[1], 3) == [
        (0, 0, 3, 0, 0, 1, "RTA"), (0, 0, 3, 1, 0, 1, "TAY")]


def test_pattern_forbids_what_the_set_holds_and_rows_by_hand():
    # text R = {A, G}; pattern G at that position: only G is left, the query's A is a mismatch although R holds A
    assert vu.as_tuples(vu.brute_force([(b"r", b"CR")], "NG", ["NA", "NG"], 1, 1)[1], 2) == [
        (0, 0, 0, 0, 1, 1, "Cr"), (0, 0, 0, 1, 1, 1, "Yg"), (1, 0, 0, 0, 0, 1, "CR"), (1, 0, 0, 1, 0, 1, "YG")]
    records = [(b"chr1 test", b"ACRTAC")]
    off, rows, prof = vu.brute_force(records, "NNN", ["ACG", "NNN"], 0, 1)
    assert rows.dtype.itemsize == 40 and off.tolist() == [0, 2, 10] and prof.tolist() == [[2], [8]]
    assert vu.as_tuples(rows[:2], 3) == [(0, 0, 0, 0, 0, 1, "ACR"), (0, 0, 1, 1, 0, 1, "AYG")]
    assert rows["site"][0].tolist() == [0b101, 0b010, 0b100, 0] and not rows["reserved"].any()
    assert vu.format_rows(records, ["ACG", "NNN"], rows[:1]) == b"ACG\tchr1 test\t0\t+\t0\tACR\n"
    assert vu.format_profile(["ACG", "NNN"], prof) == b"ACG\t2\nNNN\t8\n"
    assert vu.as_tuples(vu.brute_force(records, "NNN", ["ACT"], 1, 1)[1], 3)[0] == (0, 0, 0, 0, 1, 1, "ACr")


def test_the_models_vcf_reader_by_hand():
    snps, counts = vu.vcf_snps(VCF, VCF_RECORDS)
    assert [(int(s["record"]), int(s["pos"]), int(s["ref"]), int(s["alt"])) for s in snps] == [
        (0, 2, 4, 1), (0, 4, 1, 2 | 4), (0, 7, 2, 8), (1, 9, 8, 4)]
    assert counts == dict(lines=9, snps=4, alleles_skipped=6, no_allele=2, unknown_chrom=1, beyond_record=2)
    with pytest.raises(vu.Malformed) as e:
        vu.vcf_snps(VCF + b"\nchr1\t4\t.\tA\n", VCF_RECORDS)
    assert e.value.line == 13
    with pytest.raises(vu.Malformed):
        vu.vcf_snps(b"chr1\tx4\t.\tA\tC\n", VCF_RECORDS)
    records = [(b"chr1 the first", b"ACGTACGCACGTACGTACGT"), (b"chr2\tsecond", b"ACGTACGTAT"), (b"chr1", b"ACGTA")]
    after, changed = vu.apply_snps(records, snps)
    assert after[0][1] == b"ACRTVCGYACGTACGTACGT" and after[1][1] == b"ACGTACGTAK" and changed == 4
    assert vu.apply_snps(after, snps) == (after, 0)
    with pytest.raises(vu.Refused) as e:
        vu.apply_snps(records, np.array([(2, 0, 4, 1, (0, 0)), (3, 0, 1, 2, (0, 0)), (0, 0, 2, 1, (0, 0))], dtype=vu.SNP_DTYPE))
    assert e.value.index == 1


def test_plane_functions_and_vcf_reader_under_asan_and_ubsan(tmp_path):
    """tools/variants_sanitize.cpp: window_row() of the header on cases the model answers, its self-check of every plane
    function for every length, strand and window offset, and the VCF reader on the file above, on every truncation of it
    and on byte-mutated copies."""
    exe = tmp_path / "variants_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "variants_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(9)
    cases, want = [], []
    for L in list(range(1, 33)) * 3:
        window = with_codes(rng, random_text(rng, L), 6)
        if rng.random() < 0.1:
            window = window[:L // 2] + "Nn-"[int(rng.integers(0, 3))] + window[L // 2 + 1:]
        pattern = "".join("ACGTRYSWKMBDHV"[int(rng.integers(0, 14))] if rng.random() < 0.15 else "N" for _ in range(L))
        query = random_text(rng, L, "ACGTN")
        for strand in (0, 1):
            cases.append("%s %s %s %d" % (pattern, window, query, strand))
            if set(window) - set(vu.TEXT_CODES):
                want.append("none")
                continue
            # the row without the pattern's test: under the all-N pattern the strand is always admitted
            _, free, _ = vu.brute_force([(b"w", window.encode())], "N" * L, ["N" * L], L, L)
            _, rows, _ = vu.brute_force([(b"w", window.encode())], pattern, [query], L, L)
            mine, t = rows[rows["strand"] == strand], free[free["strand"] == strand][0]
            n_var = sum(len(su.IUPAC[c]) > 1 for c in window)
            if len(mine):
                r = mine[0]
                assert r["site"].tolist() == t["site"].tolist()
                want.append("1 %d %x %d %x %x %x %x" % (r["dist"], r["mism"], n_var, *r["site"].tolist()))
            else:
                want.append(("0", n_var, t["site"].tolist()))
    (tmp_path / "cases.txt").write_text("\n".join(cases) + "\n")
    (tmp_path / "file.vcf").write_bytes(VCF)
    args = [a for name, length in VCF_RECORDS for a in (name.decode(), str(length))]
    run = subprocess.run([str(exe), str(tmp_path / "cases.txt"), str(tmp_path / "file.vcf")] + args, capture_output=True,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0 and b"ERROR" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode(errors="replace")[-4000:]
    got = run.stdout.decode().split("\n")[:-1]
    assert len(got) > len(want)
    for line, w in zip(got, want):
        if isinstance(w, tuple):  # not admitted: dist and mism are not the model's business
            f = line.split()
            assert f[0] == w[0] and int(f[3]) == w[1] and [int(x, 16) for x in f[4:]] == w[2], (line, w)
        else:
            assert line == w
    assert sum(isinstance(w, tuple) for w in want) > 10 and want.count("none") > 4
    rest = got[len(want):]
    assert re.fullmatch(r"arithmetic ok \d+", rest[0])
    assert int(rest[0].split()[-1]) > 32 * 6 * 64  # most windows have no N: both strands of more than half of them
    snps, counts = vu.vcf_snps(VCF, VCF_RECORDS)
    assert rest[1:1 + len(snps)] == ["snp %d %d %d %d" % (s["record"], s["pos"], s["ref"], s["alt"]) for s in snps]
    assert rest[1 + len(snps)] == "counts %d %d %d %d %d %d" % tuple(counts[k] for k in ("lines", "snps", "alleles_skipped", "no_allele",
                                                                                         "unknown_chrom", "beyond_record"))
    assert rest[2 + len(snps)] == "vcf ok %d" % (len(VCF) + 1 + 3000)
