#!/usr/bin/env python3
"""Recipe of tests/golden/batches/: the WHOLE output file of the reference's own run (src/crackling/Crackling.py) for
runs of tools/make_golden_results.py with [input] batch-size and [rnafold] page-length changed in the configuration
text, kept gzipped as <run>.txt.gz.  Everything else -- the stand-ins for RNAfold and Bowtie2, the genome, the index,
the inputs -- is that recipe's (tests/golden/bowtie and tests/golden/results must exist; `make -C oracle ref`).

A batch is a run of consecutive guides in first-seen order (Batchinator.py); the reference walks every batch through all
its steps and appends the batch's rows to the file.  Two things depend on the batch: the pages of the Bowtie step and the
pages of RNAfold both start again with every batch.  With [rnafold] page-length = 0 the reference tests no guide's
secondary structure: Paginator.py:29-30 hands out the filter's generator itself, writing RNAfold's input
(Crackling.py:420) consumes it, and the loop that reads the answers (:458) sees nothing.

runs.json lists the runs with the base run's keys plus batch_size and rnafold_page_length (null: the recipe's default of
5000000, one page).  The recipe checks that the files differ from the one-batch files where the batches matter and
equal them where they cannot.  Data only: nothing of the reference's text is copied.  Never imported by a test."""
import argparse
import csv
import gzip
import json
import pathlib
import shutil
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_golden_results as mgr  # noqa: E402

OUT = ROOT / "tests" / "golden" / "batches"
# (base run, batch-size, [rnafold] page-length or None for the default)
RUNS = [("medium_page0", 64, None), ("medium_page0", 50, None), ("medium_page0", 17, None), ("medium_page0", 5000000, 0),
        ("high_page0", 64, None), ("medium_page7", 17, 5), ("ultralow_page7", 17, None), ("headers", 64, 3), ("headers", 1, 3),
        ("headers", 203, 3), ("noscore", 50, None)]
BATCH_LINE = "batch-size = 5000000\n"
RNAFOLD_LINES = "threads = 1\npage-length = 5000000\nlow_energy_threshold"


def name_of(base, batch_size, rnafold_page):
    return f"{base}_batch{batch_size}" + ("" if rnafold_page is None else f"_fold{rnafold_page}")


def config_text(batch_size, rnafold_page):
    assert mgr.CONFIG.count(BATCH_LINE) == 1 and mgr.CONFIG.count(RNAFOLD_LINES) == 1
    text = mgr.CONFIG.replace(BATCH_LINE, f"batch-size = {batch_size}\n")
    if rnafold_page is not None:
        text = text.replace(RNAFOLD_LINES, RNAFOLD_LINES.replace("5000000", str(rnafold_page)))
    return text


def run_reference(reference, run, batch_size, rnafold_page, work):
    """make_golden_results.run_reference under the changed configuration text -> bytes of the output file"""
    fasta = (mgr.OUT if run["input"].startswith("headers") else mgr.BOWTIE) / run["input"]
    plain = mgr.CONFIG
    mgr.CONFIG = config_text(batch_size, rnafold_page)
    try:
        data, log, _ = mgr.run_reference(reference, run, fasta, work)
    finally:
        mgr.CONFIG = plain
    assert data is not None, log
    return data


def table(data):
    rows = list(csv.DictReader(data.decode().splitlines(keepends=True), delimiter=",", quotechar='"'))
    assert rows and list(rows[0]) == mgr.ORDER
    return rows


def one_batch(base):
    return gzip.decompress((mgr.OUT / f"{base}.txt.gz").read_bytes())


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    base_runs = {r["name"]: r for r in mgr.runs()}
    files, kept = {}, []
    for base, batch_size, rnafold_page in RUNS:
        run = base_runs[base]
        with tempfile.TemporaryDirectory() as work:
            data = run_reference(reference, run, batch_size, rnafold_page, work)
        name = name_of(base, batch_size, rnafold_page)
        files[name] = data
        kept.append(dict(run, name=name, base=base, batch_size=batch_size, rnafold_page_length=rnafold_page))
        (OUT / f"{name}.txt.gz").write_bytes(gzip.compress(data, 9, mtime=0))
        whole = one_batch(base)
        differ = sum(a != b for a, b in zip(data.splitlines(), whole.splitlines()))
        print(f"{name}: {data.count(bytes([10])) - 1} rows, {len(data)} bytes; one batch: {len(whole)} bytes, {differ} lines differ")
    # the tests over these files cannot pass where the batches are not modelled
    for name in ("medium_page0_batch64", "medium_page0_batch50", "medium_page0_batch17"):
        assert files[name] != one_batch("medium_page0"), name
    assert files["high_page0_batch64"] != one_batch("high_page0")
    quirk = table(files["medium_page0_batch5000000_fold0"])
    assert all(r["passedSecondaryStructure"] == "?" for r in quirk), "[rnafold] page-length = 0 tested a guide"
    assert any(r["passedSecondaryStructure"] != "?" for r in table(one_batch("medium_page0")))
    n_headers = len(table(one_batch("headers")))
    # (headers has 200 guides: a batch-size of 203 holds them all)
    assert n_headers <= 203 and files["headers_batch203_fold3"] == one_batch("headers"), "one batch of all guides is the one-batch file"
    (OUT / "runs.json").write_text("[\n" + ",\n".join(json.dumps(r) for r in kept) + "\n]\n")
    for f in sorted(OUT.iterdir()):
        assert f.stat().st_size < 1 << 20, f
        print(f"{f.stat().st_size:8d} {f.name}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    make_goldens(ap.parse_args().reference)
