#!/usr/bin/env python3
"""Recipe of tests/golden/consensus/: one small FASTA and what the reference's own efficiency consensus
(src/crackling/Crackling.py:306-598) makes of its guides under nine configurations.

guides.fa is built so that every code of every column occurs (checked below; the recipe fails otherwise): G20 passed and
failed, guides that start with T, 3, 4, 13 and 14 of 20 bases A or T, TTTT inside guide[0:20] and running into the PAM, a
guide seen twice, two guides that share guide[1:20], sgRNAScorer2 scores of both signs.

RNAfold is not to be had, so a stand-in is written to a temporary directory and named as [rnafold] binary.  For every line
of its input it prints the line and a structure with an energy, both chosen by a checksum of the line: the structure of an
undisturbed scaffold or 100 dots; -35, -30, -29.9, -18, -17.9, -10 or the padded form "( -5.30)" RNAfold prints above -10
-- both thresholds from both sides.  What it printed for the configuration that folds every guide (ultralow) is kept as
fold.txt: a line's answer depends on the line alone, so this holds the answer for every guide any configuration folds.
The guides a configuration folded are the rows whose ssEnergy is not '?' (the reference fills it for every line it finds).

Every configuration runs `Crackling(ConfigManager(cfg))` of the reference checkout (--reference, default /root/reference)
in a process of its own with [offtargetscore] enabled = False; the columns COLUMNS of its output go to <config>.csv, rows
in the reference's order.  configs.json lists the configurations; model.npz holds sv, coef and intercept of the reference's
sgRNAScorer2 model as arrays.  Data only: nothing of the reference's text is copied.  Never imported by a test.

--time [--time-mbp M]: instead, time the reference's sgRNAScorer2 block (:541-577) alone, from the time stamps of its own
log, on the guides of the first M Mbp of tools/genome_index.py's seeded repeat genome, and print one JSON line."""
import argparse
import csv
import datetime
import json
import os
import pathlib
import random
import re
import shutil
import stat
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "consensus"
COLUMNS = ["seq", "sgrnascorer2score", "isUnique", "passedG20", "passedTTTT", "passedATPercent", "passedSecondaryStructure",
           "ssEnergy", "acceptedByMm10db", "acceptedBySgRnaScorer", "consensusCount", "AT", "passedAvoidLeadingT"]
THRESHOLDS = {"sgrna_threshold": 0.0, "low_energy": -30.0, "high_energy": -18.0}


def config(name, optimisation, n, mm10db=True, chopchop=True, sgrnascorer2=True):
    return dict(name=name, optimisation=optimisation, n=n, mm10db=mm10db, chopchop=chopchop, sgrnascorer2=sgrnascorer2, **THRESHOLDS)


CONFIGS = [
    config("ultralow", "ultralow", 2), config("low", "low", 2), config("medium", "medium", 2), config("high", "high", 2),
    config("high_n1", "high", 1), config("high_n3", "high", 3),
    config("high_no_mm10db", "high", 2, mm10db=False), config("ultralow_no_mm10db", "ultralow", 2, mm10db=False),
    config("medium_no_sgrnascorer2", "medium", 2, sgrnascorer2=False),
]

CONFIG = """[general]
name = golden
optimisation = {optimisation}
[consensus]
n = {n}
mm10db = {mm10db}
sgrnascorer2 = {sgrnascorer2}
chopchop = {chopchop}
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
model = {model}
score-threshold = {sgrna_threshold}
[bowtie2]
binary = true
threads = 1
page-length = 5000000
[rnafold]
binary = {rnafold}
threads = 1
page-length = 5000000
low_energy_threshold = {low_energy}
high_energy_threshold = {high_energy}
"""

DRIVER = """import sys, warnings
warnings.simplefilter('ignore')
from crackling.ConfigManager import ConfigManager
from crackling.Crackling import Crackling
cm = ConfigManager(sys.argv[1], lambda m: print(m, file=sys.stderr))
assert cm.isConfigured(), 'configuration refused'
Crackling(cm)
"""

# argv: --noPS -j<threads> -i <input> -o; writes RNAfold_output.fold into the working directory, as RNAfold does, and
# keeps a copy of it
STAND_IN = """#!{python}
import shutil, sys, zlib
src = sys.argv[sys.argv.index('-i') + 1]
FREE = '.' * 100
SCAFFOLD = '.' * 28 + '((((....))))...))))' + '.' * 21 + '((((....))))(((((((...)))))))...'
ENERGIES = ['(-35.00)', '(-30.00)', '(-29.90)', '(-18.00)', '(-17.90)', '(-10.00)', '( -5.30)']
with open(src) as fh, open('RNAfold_output.fold', 'w') as out:
    for line in fh:
        line = line.rstrip('\\n')
        h = zlib.crc32(line.encode())
        out.write(line + '\\n' + (SCAFFOLD if h & 1 else FREE) + ' ' + ENERGIES[(h >> 1) % 7] + '\\n')
shutil.copyfile('RNAfold_output.fold', 'RNAfold_output.seen')
"""


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def wrap(seq, width=60):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


def make_fasta():
    rnd = random.Random(20261018)
    rand = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))  # noqa: E731
    quiet = lambda n: ("AT" * n)[:n]                                  # matches neither pattern  # noqa: E731

    def with_at(count, first):
        """20 bases, `count` of them A or T, no TTTT, starting with `first`."""
        while True:
            body = [rnd.choice("AT") for _ in range(count)] + [rnd.choice("GC") for _ in range(20 - count)]
            rnd.shuffle(body)
            s = "".join(body)
            if s[0] == first and "TTTT" not in s:
                return s

    crafted = [with_at(3, "G") + "AGG", with_at(4, "C") + "CGG", with_at(13, "A") + "TGG", with_at(14, "A") + "GGG",
               with_at(10, "T") + "AGG",                                    # leading T
               "GACC" + "TTTT" + with_at(6, "G")[:12] + "AGG",              # TTTT inside [0:20]
               with_at(9, "C")[:17] + "TTT" + "TGG"]                        # TTTT from [17:20] into the PAM
    twice = with_at(9, "G") + "CGG"
    shared = with_at(8, "G")[1:]
    crafted += [twice, "A" + shared + "AGG", "C" + shared + "TGG", rc(with_at(11, "A") + "GGG"), twice]
    assert "TTTT" not in crafted[6][:20] and "TTTT" in crafted[6]
    r1 = rand(800)
    r2 = "".join(quiet(9) + g for g in crafted) + quiet(8)
    r3 = rand(650)
    return ">first random\n" + wrap(r1) + ">crafted\n" + wrap(r2, 70) + ">second random\n" + wrap(r3)


def run_reference(reference, cfg, fasta, work):
    """-> (rows of COLUMNS as dicts, what the stand-in printed, log text)"""
    work = pathlib.Path(work)
    outdir = work / "out"
    outdir.mkdir()
    stand_in = work / "rnafold_stand_in"
    stand_in.write_text(STAND_IN.format(python=sys.executable))
    stand_in.chmod(stand_in.stat().st_mode | stat.S_IXUSR)
    ini = work / "golden.ini"
    ini.write_text(CONFIG.format(inputs=fasta, outdir=outdir, rnafold=stand_in,
                                 model=pathlib.Path(reference) / "src" / "crackling" / "utils" / "data" / "model-py3.txt",
                                 **{k: v for k, v in cfg.items() if k != "name"}))
    driver = work / "driver.py"
    driver.write_text(DRIVER)
    env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
    r = subprocess.run([sys.executable, str(driver), str(ini)], env=env, capture_output=True, text=True, cwd=work)
    errlog = outdir / "golden-golden.errlog"
    if r.returncode:
        raise RuntimeError(f"reference failed on {cfg['name']}:\n{r.stdout}\n{r.stderr}\n{errlog.read_text() if errlog.exists() else ''}")
    with open(outdir / "golden-guides.txt", newline="") as fh:
        rows = [{c: row[c] for c in COLUMNS} for row in csv.DictReader(fh, delimiter=",", quotechar='"')]
    printed = work / "RNAfold_output.seen"   # (the reference moves the output itself away and removes it at its end)
    text = printed.read_text() if printed.exists() else ""
    return rows, text, (outdir / "golden-golden.log").read_text()


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    fasta = OUT / "guides.fa"
    fasta.write_text(make_fasta())
    seen_codes = {c: set() for c in COLUMNS[2:] if c not in ("ssEnergy", "AT", "consensusCount")}
    for cfg in CONFIGS:
        with tempfile.TemporaryDirectory() as work:
            rows, text, _ = run_reference(reference, cfg, fasta, work)
        with open(OUT / f"{cfg['name']}.csv", "w", newline="") as fh:
            w = csv.DictWriter(fh, COLUMNS, dialect="unix", quoting=csv.QUOTE_MINIMAL)
            w.writeheader()
            w.writerows(rows)
        if cfg["name"] == "ultralow":
            (OUT / "fold.txt").write_text(text)
            check_inputs(rows, text)
        for row in rows:
            for c in seen_codes:
                seen_codes[c].add(row[c])
        print(cfg["name"], len(rows), "guides,", sum(r["ssEnergy"] != "?" for r in rows), "folded,", sum(r["consensusCount"] >= str(cfg["n"]) for r in rows), "at or above n")
    want = {c: {"0", "1", "?"} for c in seen_codes}
    want["isUnique"] = {"0", "1"}
    want["passedSecondaryStructure"].add("!")
    assert seen_codes == want, {c: sorted(v) for c, v in seen_codes.items() if v != want[c]}
    (OUT / "configs.json").write_text("[\n" + ",\n".join(json.dumps(c) for c in CONFIGS) + "\n]\n")
    import joblib
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = joblib.load(pathlib.Path(reference) / "src" / "crackling" / "utils" / "data" / "model-py3.txt")
    sv = np.asarray(clf.support_vectors_)
    assert np.all((sv == 0) | (sv == 1))
    np.savez_compressed(OUT / "model.npz", sv=sv.astype(np.uint8), coef=np.asarray(clf._dual_coef_, dtype=np.float64)[0],
                        intercept=np.float64(clf._intercept_[0]))
    for f in sorted(OUT.iterdir()):
        assert f.stat().st_size < 1 << 20, f
        print(f"{f.stat().st_size:8d} {f.name}")


def check_inputs(rows, text):
    """What guides.fa was built to contain, on the rows of the configuration that assesses every guide."""
    seqs = [r["seq"] for r in rows]
    at = lambda s: sum(c in "AT" for c in s[:20])  # noqa: E731
    assert 200 <= len(seqs) <= 230, len(seqs)
    assert {at(s) for s in seqs} >= {3, 4, 13, 14}
    assert any(s[19] == "G" for s in seqs) and any(s[19] != "G" for s in seqs) and any(s[0] == "T" for s in seqs)
    assert any("TTTT" in s[:20] for s in seqs) and any("TTTT" in s and "TTTT" not in s[:20] for s in seqs)
    assert any(r["isUnique"] == "0" for r in rows)
    keys = [s[1:20] for s in seqs]
    assert len(set(keys)) < len(keys), "two guides that share guide[1:20]"
    scores = [float(r["sgrnascorer2score"]) for r in rows]
    assert min(scores) < 0 < max(scores)
    assert any(r["ssEnergy"] == "" for r in rows), "a padded energy"
    answers = set(text.splitlines()[1::2])
    assert len({a.split(" ", 1)[1] for a in answers}) == 7 and len({a.split(" ", 1)[0] for a in answers}) == 2


def time_reference(reference, mbp):
    sys.path.insert(0, str(ROOT / "tools"))
    import genome_index
    cfg = config("time", "ultralow", 1, mm10db=False, chopchop=False)
    with tempfile.TemporaryDirectory() as work:
        fa = pathlib.Path(work) / "slice.fa"
        genome_index.genome(fa, mbp, "repeat", 20261016)
        rows, _, log = run_reference(reference, cfg, fa, work)
    stamp = lambda title: datetime.datetime.strptime(  # noqa: E731
        re.search(r">>> ([0-9-]+ [0-9:]+):\t" + re.escape(title), log).group(1), "%Y-%m-%d %H:%M:%S:%f")
    seconds = (stamp("Evaluating efficiency via consensus approach.") - stamp("sgRNAScorer2 - score using model.")).total_seconds()
    scored = sum(r["sgrnascorer2score"] != "?" for r in rows)
    print(json.dumps({"reference_sgrnascorer2_block": "Crackling.py:541-577", "genome_mbp": mbp, "guides_scored": scored,
                      "seconds": seconds, "microseconds_per_guide": 1e6 * seconds / scored}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--time-mbp", type=float, default=0.2)
    a = ap.parse_args()
    if a.time:
        time_reference(a.reference, a.time_mbp)
    else:
        make_goldens(a.reference)
