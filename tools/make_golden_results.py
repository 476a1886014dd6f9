#!/usr/bin/env python3
"""Recipe of tests/golden/results/: the WHOLE output file (golden-guides.txt, header row included) of the reference's own
run (src/crackling/Crackling.py) for the inputs of tests/golden/bowtie, kept gzipped as <run>.txt.gz.

The stand-ins for RNAfold and Bowtie2, the genome, the index and the configuration text are those of
tools/make_golden_bowtie.py (tests/golden/bowtie must exist: genome.fa, input.fa, index.issl).  Runs:
  ultralow_page0 .. high_page7   the six configurations of the bowtie recipe
  noscore                        medium without mm10db, [offtargetscore] enabled = False
  headers                        medium, method mit, threshold 99 on headers_input.fa: the same sequence cut into records
                                 whose header lines hold a comma, a double quote and blanks, a record without a guide and
                                 one that repeats a stretch, so that its guides are seen twice (kept here, with what
                                 RNAfold's stand-in printed for it)
  tab                            [output] delimiter = a TAB.  The reference cannot make this file: an INI value cannot hold a
                                 lone TAB (configparser strips it), and with the delimiter set on the loaded configuration
                                 the run stops in Crackling.py:300 -- Batchinator.py:7 writes the guides' temporary file
                                 with ',' whatever the delimiter, :287 reads it back with the configured one, and a row
                                 then has one field.  The recipe tries, checks that it fails there and keeps no file
runs.json lists the runs that were kept with their configuration.  The recipe checks that every code of every column
occurs in some file and that a padded energy left an empty ssEnergy.  Data only: nothing of the reference's text is
copied.  Never imported by a test."""
import argparse
import csv
import gzip
import json
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_golden_bowtie as mgb  # noqa: E402
import make_golden_consensus as mgc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "results"
BOWTIE = ROOT / "tests" / "golden" / "bowtie"
ORDER = ["seq", "sgrnascorer2score", "header", "start", "end", "strand", "isUnique", "passedG20", "passedTTTT", "passedATPercent",
         "passedSecondaryStructure", "ssL1", "ssStructure", "ssEnergy", "acceptedByMm10db", "acceptedBySgRnaScorer",
         "consensusCount", "passedBowtie", "passedOffTargetScore", "AT", "bowtieChr", "bowtieStart", "bowtieEnd",
         "mitOfftargetscore", "cfdOfftargetscore", "passedAvoidLeadingT"]
CONFIG = mgb.CONFIG.replace("delimiter = ,", "delimiter = {delimiter}").replace("enabled = True", "enabled = {enabled}")
assert CONFIG.count("{delimiter}") == 1 and CONFIG.count("{enabled}") == 1
# the configuration as loaded, with the delimiter replaced where an INI file cannot say it
DRIVER_TAB = mgc.DRIVER.replace("Crackling(cm)", "cm['output']['delimiter'] = '\\t'\nCrackling(cm)")
HEADERS = ['exons, first part', 'he said "cut here"', '  two  blanks  and, a "quoted" comma  ']


def runs():
    out = [dict(c, input="input.fa", delimiter=",", enabled=True) for c in mgb.CONFIGS]
    base = dict(mgb.CONFIGS[2], input="input.fa", delimiter=",", enabled=True)
    assert base["name"] == "medium_page0"
    out.append(dict(base, name="noscore", enabled=False, mm10db=False))
    out.append(dict(base, name="headers", input="headers_input.fa", method="mit", score_threshold=99))
    out.append(dict(mgb.CONFIGS[0], name="tab", input="input.fa", delimiter="\t", enabled=True))
    return out


def headers_input():
    """input.fa's sequence in three records under HEADERS (a guide across a cut is lost, one inside a record stays), a
    record without a guide and one that repeats 300 bases of the first."""
    seq = "".join(line for line in (BOWTIE / "input.fa").read_text().splitlines() if not line.startswith(">"))
    cuts = [0, len(seq) // 3, 2 * len(seq) // 3, len(seq)]
    return ("".join(f">{h}\n" + mgc.wrap(seq[a:b]) for h, a, b in zip(HEADERS, cuts, cuts[1:])) + ">no guide\nACGTACGT\n" +
            ">again\n" + mgc.wrap(seq[100:400]))


def run_reference(reference, run, fasta, work):
    """-> (bytes of golden-guides.txt or None when the reference failed, its stderr + error log, RNAfold's stand-in's text)"""
    work = pathlib.Path(work)
    outdir = work / "out"
    outdir.mkdir()
    rnafold = mgb.executable(work / "rnafold_stand_in", mgc.STAND_IN.format(python=sys.executable))
    bowtie = mgb.executable(work / "bowtie_stand_in", mgb.BOWTIE_STAND_IN.format(python=sys.executable, tools=str(ROOT / "tools")))
    skip = ("name", "input")
    ini = work / "golden.ini"
    tab = run["delimiter"] == "\t"
    ini.write_text(CONFIG.format(inputs=fasta, genome=BOWTIE / "genome.fa", issl=BOWTIE / "index.issl", outdir=outdir,
                                 rnafold=rnafold, bowtie=bowtie, scorer=ROOT / "oracle" / "_ref" / "isslScoreOfftargets",
                                 model=pathlib.Path(reference) / "src" / "crackling" / "utils" / "data" / "model-py3.txt",
                                 **{k: ("," if k == "delimiter" and tab else v) for k, v in run.items() if k not in skip}))
    driver = work / "driver.py"
    driver.write_text(DRIVER_TAB if tab else mgc.DRIVER)
    env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
    r = subprocess.run([sys.executable, str(driver), str(ini)], env=env, capture_output=True, text=True, cwd=work)
    errlog = outdir / "golden-golden.errlog"
    log = r.stderr + (errlog.read_text() if errlog.exists() else "")
    fold = work / "RNAfold_output.seen"
    fold_text = fold.read_text() if fold.exists() else ""
    if r.returncode:
        return None, log, fold_text
    return (outdir / "golden-guides.txt").read_bytes(), log, fold_text


def check_codes(files):
    """files: run name -> (bytes, delimiter).  Every code of every column occurs somewhere."""
    seen = {c: set() for c in ORDER}
    for name, (data, delimiter) in files.items():
        rows = list(csv.reader(data.decode().splitlines(keepends=True), delimiter=delimiter, quotechar='"'))
        assert rows[0] == ORDER, name
        for row in rows[1:]:
            assert len(row) == len(ORDER), (name, row)
            for c, v in zip(ORDER, row):
                seen[c].add(v)
    for c in ("passedG20", "passedTTTT", "passedATPercent", "acceptedByMm10db", "acceptedBySgRnaScorer", "passedAvoidLeadingT",
              "passedBowtie", "passedOffTargetScore"):
        assert seen[c] == {"0", "1", "?"}, (c, seen[c])
    assert seen["passedSecondaryStructure"] == {"0", "1", "?", "!"}
    assert seen["isUnique"] == {"0", "1"} and seen["strand"] == {"+", "-"}
    assert "-" in seen["header"] and "-" in seen["start"] and "-" in seen["end"]
    assert {(">" + h).strip()[1:] for h in HEADERS} <= seen["header"]  # (the reference strips the line, '>' included)
    assert seen["consensusCount"] <= {"0", "1", "2", "3"} and len(seen["consensusCount"]) >= 3
    for c in ("sgrnascorer2score", "AT", "ssL1", "ssStructure", "mitOfftargetscore", "cfdOfftargetscore", "bowtieStart", "bowtieEnd"):
        assert "?" in seen[c] and len(seen[c]) > 2, c
    assert {"?", "*"} < seen["bowtieChr"]
    assert {"?", ""} < seen["ssEnergy"] and len(seen["ssEnergy"]) > 3, "a padded energy leaves an empty ssEnergy"
    assert any(v.startswith("-") for v in seen["sgrnascorer2score"]) and any(v[0].isdigit() for v in seen["sgrnascorer2score"])
    return seen


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    (OUT / "headers_input.fa").write_text(headers_input())
    files, kept = {}, []
    for run in runs():
        fasta = (OUT if run["input"].startswith("headers") else BOWTIE) / run["input"]
        with tempfile.TemporaryDirectory() as work:
            data, log, fold = run_reference(reference, run, fasta, work)
        if run["name"] == "tab":
            assert data is None and "IndexError" in log, "the reference wrote a TAB-delimited file: keep it and say so above"
            print("tab: the reference stops with IndexError (Crackling.py:300), no file")
            continue
        assert data is not None, log
        files[run["name"]] = (data, run["delimiter"])
        kept.append(run)
        (OUT / f"{run['name']}.txt.gz").write_bytes(gzip.compress(data, 9, mtime=0))
        if run["name"] == "headers":
            (OUT / "headers_fold.txt.gz").write_bytes(gzip.compress(fold.encode(), 9, mtime=0))
        print(run["name"], data.count(b"\n") - 1, "rows,", len(data), "bytes")
    check_codes(files)
    (OUT / "runs.json").write_text("[\n" + ",\n".join(json.dumps(r) for r in kept) + "\n]\n")
    for f in sorted(OUT.iterdir()):
        assert f.stat().st_size < 1 << 20, f
        print(f"{f.stat().st_size:8d} {f.name}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    make_goldens(ap.parse_args().reference)
