#!/usr/bin/env python3
"""Recipe of tests/golden/guides/: small FASTA inputs and what the reference's own guide extraction
(src/crackling/Crackling.py:151-305) makes of them.

Every case is written to tests/golden/guides/<case>/ and run through `Crackling(ConfigManager(cfg))` of the reference
checkout (--reference, default /root/reference) in a process of its own, with everything behind the extraction switched
off: [consensus] n = 0 and the three tools False, [offtargetscore] enabled = False, the three `binary` keys `true`.  The
run writes <name>-guides.txt; its columns seq, header, start, end, strand, isUnique go to <case>.guides.csv, rows in the
reference's order (first seen).  A case the reference dies on is recorded with the exception's name and no rows.
cases.json lists, per case, the inputs in the order the reference reads them (a directory: reverse sorted names,
ConfigManager.py:181-184).  Data only: nothing of the reference's text is copied.  Never imported by a test.

--time-mbp N: instead, time the reference's extraction alone on the first N Mbp of tools/genome_index.py's seeded repeat
genome and print one JSON line (the context figure of DESIGN.md, "Candidate guides")."""
import argparse
import csv
import json
import os
import pathlib
import random
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "guides"
COLUMNS = ["seq", "header", "start", "end", "strand", "isUnique"]

CONFIG = """[general]
name = golden
optimisation = high
[consensus]
n = 0
mm10db = False
sgrnascorer2 = False
chopchop = False
[input]
exon-sequences = {inputs}
offtarget-sites = unused
gff-annotation = unused
bowtie2-index = unused
batch-size = 5000000
[output]
dir = {outdir}
filename = guides.txt
delimiter = ,
[offtargetscore]
enabled = False
binary = true
method = and
threads = 1
page-length = 5000000
score-threshold = 75
max-distance = 4
[sgrnascorer2]
model = unused
score-threshold = 0
[bowtie2]
binary = true
threads = 1
page-length = 5000000
[rnafold]
binary = true
threads = 1
page-length = 5000000
low_energy_threshold = -30
high_energy_threshold = -18
"""

DRIVER = """import sys
from crackling.ConfigManager import ConfigManager
from crackling.Crackling import Crackling
cm = ConfigManager(sys.argv[1], lambda m: None)
assert cm.isConfigured(), 'configuration refused'
out, err = sys.stdout, sys.stderr
try:
    Crackling(cm)
except Exception as e:
    sys.stdout, sys.stderr = out, err
    print('RAISED ' + type(e).__name__)
    sys.exit(3)
"""


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def wrap(seq, width=60, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def make_cases():
    """-> [(case, {file name: bytes}, input is the directory, note)]"""
    rnd = random.Random(20261017)
    rand = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))  # noqa: E731
    quiet = lambda n: ("AT" * n)[:n]                                  # matches neither pattern  # noqa: E731
    cases = []

    # -- one multi-record file: wrapped lines, soft-masked and N stretches, repeats, both strands
    thrice = rand(21) + "GG"                       # three times in two records
    rev_first = rand(21) + "GG"                    # first met as a reverse match, forward in a later record
    both = "CC" + rand(19) + "GG"                  # one start, both patterns
    masked = (rand(21) + "GG").lower()             # would match if the case were folded
    r1 = rand(150) + thrice + quiet(10) + thrice + rand(90)
    r2 = rand(80) + rc(rev_first) + quiet(7) + masked + rand(40).lower() + "N" * 30 + rand(120)
    r3 = quiet(30) + both + quiet(30) + "G" * 35 + quiet(9) + rand(60) + "N" + rand(60)
    r4 = rand(70) + thrice + quiet(12) + rev_first + rand(100)
    multi = (">chr1 first record\n" + wrap(r1) + ">chr2 \"quoted\", with a comma\n" + wrap(r2, 50) +
             ">chr3\n" + wrap(r3, 70) + ">chr4 last\n" + wrap(r4))
    cases.append(("multi", {"multi.fa": multi.encode()}, False,
                  "wrapped records; lower case and N; a guide three times in two records; reverse first, forward later; "
                  "one start on both patterns; G x 35; a header with a comma and a quote"))

    # -- which records count
    a1, a2, a3, b1, e1, z1, z2 = (rand(120) for _ in range(7))
    headers = (wrap(rand(90)) +                           # text ahead of the first header
               ">alpha\n" + wrap(a1) +
               "  \t>beta indented\n" + wrap(b1) +        # leading blanks before '>'
               ">alpha\n" + wrap(a2) +                    # repeated in mid-file: skipped
               ">empty\n" +                               # a header without sequence is recorded ...
               ">gamma\n" + wrap(rand(100)) +
               ">empty\n" + wrap(e1) +                    # ... so this one is skipped
               ">\n" + wrap(z1) +                         # empty name with sequence: always processed
               ">\n" + wrap(z2) +
               ">alpha\n" + wrap(a3))                     # repeated as the last record: kept
    cases.append(("headers", {"headers.fa": headers.encode()}, False,
                  "text ahead of the first header; blanks before '>'; a header repeated in mid-file and as the last record; "
                  "a header without sequence; empty names"))

    # -- line ends and blanks inside lines
    c1, c2 = rand(200), rand(130)
    crlf = (">one\r\n" + wrap(c1, 40, "\r\n") + ">two  \t\r\n" + wrap(c2[:80], 40, " \t\r\n") + "  " + c2[80:] + "\r" +
            ">three after a lone CR\r\n" + rand(60) + " " + rand(60) + "\r\n")  # a blank inside a line stays in the sequence
    cases.append(("crlf", {"crlf.fa": crlf.encode()}, False, "CRLF line ends, a lone CR, blanks around and inside lines"))

    # -- a directory of three files, a record name shared across files
    shared = rand(140)
    files = {
        "B_second.fa": (">shared\n" + wrap(shared) + ">only_B\n" + wrap(rand(110))).encode(),
        "a_third.fa": (">only_a\n" + wrap(rand(100)) + ">shared\n" + wrap(rand(140)) + ">tail_a\n" + wrap(thrice + rand(40))).encode(),
        "c_first.fa": (">shared\n" + wrap(rand(140)) + ">only_c\n" + wrap(rand(60) + thrice + rand(30))).encode(),
    }
    cases.append(("dir3", files, True, "reverse sorted names (c, a, B) differ from sorted ones (B, a, c); 'shared' is in every file"))

    # -- nothing to find, and the line the reference dies on
    cases.append(("nomatch", {"nomatch.fa": (">quiet\n" + wrap(quiet(300)) + ">short\nACGTACGTACGTACGTACGTGG\n").encode()}, False,
                  "no match anywhere: an empty set here (the reference divides by its count of matches, Crackling.py:254)"))
    cases.append(("blankline", {"blankline.fa": (">one\n" + wrap(rand(100)) + "\n>two\n" + wrap(rand(100))).encode()}, False,
                  "an empty line: IndexError in the reference (Crackling.py:196), ISSL_E_FORMAT here"))
    return cases


def run_reference(reference, inputs, work):
    """-> (rows, name of the exception or None)"""
    outdir = pathlib.Path(work) / "out"
    outdir.mkdir()
    cfg = pathlib.Path(work) / "golden.ini"
    cfg.write_text(CONFIG.format(inputs=inputs, outdir=outdir))
    driver = pathlib.Path(work) / "driver.py"
    driver.write_text(DRIVER)
    env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
    r = subprocess.run([sys.executable, str(driver), str(cfg)], env=env, capture_output=True, text=True, cwd=work)
    if r.returncode == 3:
        return [], r.stdout.strip().split()[-1]
    if r.returncode:
        raise RuntimeError(f"reference failed on {inputs}:\n{r.stdout}\n{r.stderr}")
    with open(outdir / "golden-guides.txt", newline="") as fh:
        rows = list(csv.DictReader(fh, delimiter=",", quotechar='"'))
    return [[row[c] for c in COLUMNS] for row in rows], None


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    index = []
    for case, files, as_dir, note in make_cases():
        d = OUT / case
        d.mkdir()
        for name, data in files.items():
            (d / name).write_bytes(data)
        order = sorted(files, reverse=True)
        with tempfile.TemporaryDirectory() as work:
            rows, raised = run_reference(reference, str(d if as_dir else d / order[0]), work)
        with open(OUT / f"{case}.guides.csv", "w", newline="") as fh:
            w = csv.writer(fh, dialect="unix", quoting=csv.QUOTE_MINIMAL)
            w.writerow(COLUMNS)
            w.writerows(rows)
        index.append({"case": case, "inputs": order, "directory": as_dir,
                      "reference": f"raises {raised}" if raised else "ok", "rows": len(rows), "note": note})
        print(case, "raises " + raised if raised else f"{len(rows)} guides, {sum(r[5] == '0' for r in rows)} ambiguous")
    (OUT / "cases.json").write_text(json.dumps(index, indent=1) + "\n")


def time_reference(reference, mbp):
    sys.path.insert(0, str(ROOT / "tools"))
    import genome_index
    with tempfile.TemporaryDirectory() as work:
        fa = pathlib.Path(work) / "slice.fa"
        genome_index.genome(fa, mbp, "repeat", 20261016)
        t = time.perf_counter()
        rows, raised = run_reference(reference, str(fa), work)
        print(json.dumps({"reference_extraction_mbp": mbp, "seconds_whole_run_everything_else_off": time.perf_counter() - t,
                          "guides": len(rows), "raised": raised}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--time-mbp", type=float, default=None)
    a = ap.parse_args()
    if a.time_mbp:
        time_reference(a.reference, a.time_mbp)
    else:
        make_goldens(a.reference)
