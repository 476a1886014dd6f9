#!/usr/bin/env python3
"""Golden vectors for the INPUT SHAPES of the off-target extraction step, from the REFERENCE Python
(/root/reference/src/crackling/utils/extractOfftargets.py), run in the build container only:

    python oracle/make_golden_extract_cases.py

The reference has two modes.  With exactly one input file left after directory expansion (:201-222) it explodes that
file into one temporary file per record (:26-62, every line stripped).  With more it reads each file whole (:74-90): a
line is a header when its first raw character is '>', sequence lines keep their leading blanks, and the records of one
file live in a dict keyed by the header line, so a repeated header drops the earlier record.

Writes tests/golden/extract/cases/<case>/in<k>.fa (inputs, data made here, seeded), <case>/sites.txt (the file the
reference's startMultiprocessing() wrote) and cases/cases.json: per case the input files in order, whether they are
passed as a list or as a directory, and either the line count of sites.txt or the class of the exception the reference
raised -- then also the line count of oracle/extract_oracle.c on the same input ("oracle_lines"; the project accepts
what the reference rejects).  Only data is stored."""
import ctypes as C
import json
import multiprocessing
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, "/root/reference/src")
CASES = ROOT / "tests" / "golden" / "extract" / "cases"


def seq(rng, n, lower=0.0):
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    if lower:
        m = rng.random(n) < lower
        s[m] += 32
    return s.tobytes().decode()


def sprinkle(rng, s, alphabet, p):
    b = bytearray(s.encode())
    for i in np.flatnonzero(rng.random(len(b)) < p):
        b[i] = ord(alphabet[int(rng.integers(0, len(alphabet)))])
    return b.decode()


def wrap(s, width, nl="\n", pre="", post="", last_nl=True):
    lines = [pre + s[i:i + width] + post for i in range(0, len(s), width)]
    return nl.join(lines) + (nl if last_nl else "")


def rec(rng, name, n=450, width=60, nl="\n", **kw):
    return ">" + name + nl + wrap(seq(rng, n, lower=0.2), width, nl, **kw)


def make_cases():
    """[(name, "list" | "dir", [(file name, text)])], every text ASCII."""
    rng = np.random.default_rng(20240607)
    r = lambda name, **kw: rec(rng, name, **kw)
    other = lambda tag: ("in1.fa", r(f"plain {tag}", n=400))
    cases = []

    def both(name, text):
        """The same odd file alone (explode rules) and next to a plain one (per-file rules)."""
        cases.append((name + "_single", "list", [("in0.fa", text)]))
        cases.append((name + "_multi", "list", [("in0.fa", text), other(name)]))

    odd = "RYKMSWBDHVNrykmswbdhvn*-0123456789"
    both("iupac", ">chrA iupac\n" + wrap(sprinkle(rng, seq(rng, 700, lower=0.2), odd, 0.01), 70)
         + ">chrB\n" + wrap(sprinkle(rng, seq(rng, 500), odd, 0.02), 50))
    cases.append(("one_record_per_file", "list", [(f"in{k}.fa", r(f"chr{k}", n=350)) for k in range(3)]))
    cases.append(("several_records_per_file", "list",
                  [(f"in{k}.fa", r(f"f{k} a", n=300) + r(f"f{k} b", n=250) + r(f"f{k} c", n=200)) for k in range(2)]))
    # the same header line three times, LF / CRLF / LF: text mode makes them equal, the last record stands (:83-85)
    both("repeated_header", r("dup x") + r("between", n=300) + r("dup x", nl="\r\n", n=350) + r("dup x", n=300))
    # the last copy ends the file without a line end: a different key, both records stand; in the second file the
    # last copy has its line end and empties the record
    cases.append(("repeated_header_no_final_newline", "list",
                  [("in0.fa", r("dup", n=400) + r("b", n=300) + ">dup"),
                   ("in1.fa", r("dup", n=400) + r("b", n=300) + ">dup\n")]))
    cases.append(("same_header_in_two_files", "list", [("in0.fa", r("chr1 same", n=400)), ("in1.fa", r("chr1 same", n=400))]))
    cases.append(("headerless_file_among_headered", "list",
                  [("in0.fa", r("chr1", n=350)), ("in1.fa", wrap(seq(rng, 500), 80)), ("in2.fa", r("chr2", n=300))]))
    both("sequence_before_first_header", wrap(seq(rng, 400), 60) + r("late", n=400) + r("later", n=300))
    both("blanks_around_sequence_lines",
         ">pad\n" + wrap(seq(rng, 600, lower=0.2), 40, pre="  ", post=" \t ") + ">tabs\n" + wrap(seq(rng, 500), 50, pre="\t"))
    both("header_with_leading_blanks",
         r("first", n=300) + "  >ACGTTGCAAGGCTAGCTAGGATCCGGTTAACCGGAAGGCCTTAGGA indented\n" + wrap(seq(rng, 400), 60) + r("last", n=300))
    both("blank_lines", r("a", n=300) + "\n" + wrap(seq(rng, 200), 50) + "\n\n" + r("b", n=300) + "\n")
    both("crlf", r("a", nl="\r\n", n=400) + r("b", nl="\r\n", n=400))
    both("lone_cr", r("a", nl="\r", n=400) + r("b", n=300) + r("c", nl="\r", n=300))
    both("form_feed_at_line_end", ">ff\n" + wrap(seq(rng, 500), 50, post="\x0c") + ">vt\n" + wrap(seq(rng, 300), 60, post="\x0b"))
    # the separators FS GS RS US are blanks to str.strip() and not to C's isspace()
    both("ascii_separators_at_line_end",
         ">fs\n" + wrap(seq(rng, 400), 50, post="\x1c\x1f") + ">gs\n" + wrap(seq(rng, 300), 60, pre="\x1d", post="\x1e"))
    both("no_final_newline", r("a", n=400) + ">b\n" + wrap(seq(rng, 400), 60, last_nl=False))
    both("gt_inside_sequence_line", ">a\n" + wrap(sprinkle(rng, seq(rng, 600), ">", 0.01), 60) + r("b", n=300))
    cases.append(("directory_with_dot_file", "dir",
                  [("in0.fa", r("chr1", n=350)), ("in1.fa", r("chr2", n=350) + r("chr2", n=300)), (".hidden.fa", r("hidden", n=300))]))
    # one entry besides the dot-file: single-input mode, the repeated header keeps both records
    cases.append(("directory_with_one_file", "dir",
                  [("in0.fa", r("chr1", n=350) + r("chr2", n=300) + r("chr1", n=300)), (".hidden.fa", r("hidden", n=300))]))
    cases.append(("empty_file_among_others", "list", [("in0.fa", r("a", n=350)), ("in1.fa", ""), ("in2.fa", r("b", n=350))]))
    cases.append(("header_only_file", "list", [("in0.fa", r("a", n=350)), ("in1.fa", ">nothing here\n"), ("in2.fa", r("b", n=350))]))
    return cases


def oracle_lines(blobs):
    subprocess.run(["make", "-C", str(ROOT / "oracle"), "_build/libextract_oracle.so"], check=True, capture_output=True)
    lib = C.CDLL(str(ROOT / "oracle" / "_build" / "libextract_oracle.so"))
    lib.oracle_extract.restype = C.c_void_p
    lib.oracle_extract.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t)]
    lib.oracle_extract_free.argtypes = [C.c_void_p]
    n = C.c_size_t()
    p = lib.oracle_extract((C.c_char_p * len(blobs))(*blobs), (C.c_size_t * len(blobs))(*map(len, blobs)), len(blobs), C.byref(n))
    lib.oracle_extract_free(p)
    return n.value // 21


def main():
    import crackling.utils.extractOfftargets as eo
    if CASES.exists():
        shutil.rmtree(CASES)
    CASES.mkdir(parents=True)
    index = []
    pool = multiprocessing.Pool(2)
    for name, how, files in make_cases():
        d = CASES / name
        d.mkdir()
        for fn, text in files:
            (d / fn).write_bytes(text.encode("ascii"))
        entry = {"case": name, "inputs": [fn for fn, _ in files], "as": how}
        with tempfile.TemporaryDirectory() as tmp:      # the inputs alone, in a directory of their own
            for fn, _ in files:
                shutil.copy(d / fn, os.path.join(tmp, fn))
            args = [tmp] if how == "dir" else [os.path.join(tmp, fn) for fn, _ in files]
            out = d / "sites.txt"
            try:
                eo.startMultiprocessing(args, str(out), pool, 2, 100)
                os.chmod(out, 0o644)
                entry["lines"] = sum(1 for _ in open(out))
            except Exception as e:                      # a recorded result: the reference rejects this input
                entry["raises"] = type(e).__name__
                entry["oracle_lines"] = oracle_lines([t.encode("ascii") for fn, t in files if not (how == "dir" and fn[0] == ".")])
        index.append(entry)
        print(name, entry.get("lines", entry.get("raises")), file=sys.stderr)
    pool.close()
    (CASES / "cases.json").write_text(json.dumps(index, indent=1) + "\n")


if __name__ == "__main__":
    main()
