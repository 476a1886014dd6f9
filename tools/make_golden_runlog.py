#!/usr/bin/env python3
"""Recipe of tests/golden/runlog/: the LOG (<name>-<name>.log) of the reference's own run (src/crackling/Crackling.py) for
the runs of tools/make_golden_results.py and tools/make_golden_batches.py, for three more with [offtargetscore]
page-length changed in the configuration text, for one with batches that select no guide under a [bowtie2] page-length
above 0, for one whose RNAfold leaves answers out and for one whose input is a directory of several files (multi/), kept
gzipped as <run>.log.gz; the recipe's own runs with their output file, <run>.txt.gz.  configs/ holds a handful of INI
files and what the reference's ConfigManager derived from each (expected.json).  Everything else -- the stand-ins for RNAfold
and Bowtie2, the genome, the index, the inputs, the configuration text -- is those recipes' (tests/golden/bowtie,
tests/golden/results and tests/golden/batches must exist; `make -C oracle ref`).

The log is what the reference prints while it runs (Helpers.py:31-35: every message behind '>>> <timestamp>:' and
followed by an empty line; the RNAfold rows that were not found are printed bare).  Two things are taken out before a log
is kept, because they name directories of the machine the recipe ran on: the lines of Helpers.runner ('| Calling:',
'| Finished') and 'Batchinator is writing to:', which the comparison drops anyway (tests/runlog_util.py), and the
directory in front of the input's file name in 'Identifying possible target sites in:'.

runs.json lists the runs with their configuration, the base run's keys plus batch_size, rnafold_page_length and
offtarget_page_length (null: the recipe's default of 5000000).  The recipe checks that the kept logs show what the tests
over them need: a batch with rows that erred, one with rows RNAfold did not answer, an empty selection under a page
length of 0 and under one above 0, duplicates in more than one file of the directory run, and a batch whose Bowtie
`failed` figure differs from the number of its rows that end rejected (the events run: the genome of tests/golden/bowtie
repeats no read of a strand-1 guide of a CCT window without repeating the window, so that run's genome has one record more).  Data only: nothing of the reference's text is copied.  Never imported by a test."""
import argparse
import gzip
import json
import pathlib
import re
import shutil
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_golden_batches as mgba  # noqa: E402
import make_golden_results as mgr  # noqa: E402

OUT = ROOT / "tests" / "golden" / "runlog"
# The runs of this recipe alone: (base run, batch-size, [rnafold] page-length or None, [offtargetscore] page-length or None,
# RNAfold answers every line).  Their output files are kept beside their logs, as <run>.txt.gz
OWN_RUNS = [("medium_page0", 5000000, None, 5, True), ("ultralow_page7", 17, None, 5, True), ("high_page0", 64, None, 0, True),
            ("medium_page7", 3, 5, None, True),      # batches without a selected row under a [bowtie2] page-length above 0
            ("medium_page0", 17, None, None, False)]  # RNAfold leaves out the answers whose line has a CRC-32 that 5 divides
# One more: a directory of several files with guides repeated inside a file and across files, at medium in one batch (kept
# with its inputs and with what RNAfold's stand-in printed)
MULTI = "multi"
# And one whose Bowtie `failed` figure is no count of rows (Crackling.py:709-717 counts events): events.fa at ultralow in one
# batch and one page, on events_genome.fa -- the genome of tests/golden/bowtie and one record more (events_files)
EVENTS = "events"
OFFTARGET_LINES = "threads = 1\npage-length = 5000000\nscore-threshold"
ANSWER = "        out.write(line"
DROPPED = ("| Calling:", "| Finished", "Batchinator is writing to:")


def own_name(base, batch_size, rnafold_page, offtarget_page, answers):
    return mgba.name_of(base, batch_size, rnafold_page) + ("" if offtarget_page is None else f"_score{offtarget_page}") + \
        ("" if answers else "_missing")


def multi_inputs():
    """input.fa's sequence cut into records of three files that overlap each other (guides repeated across files) and
    themselves (inside a file); the reference reads a directory's files in reverse sorted order: c, b, a."""
    seq = "".join(line for line in (mgr.BOWTIE / "input.fa").read_text().splitlines() if not line.startswith(">"))
    wrap = mgr.mgc.wrap
    return {"c.fa": ">c one\n" + wrap(seq[850:1400] + seq[1000:1100]) + ">c two\n" + wrap(seq[1500:1800]),
            "b.fa": ">b one\n" + wrap(seq[450:900]) + ">b two\n" + wrap(seq[100:250]),
            "a.fa": ">a one\n" + wrap(seq[0:500]) + ">a two\n" + wrap(seq[300:600]) + ">a three\n" + wrap(seq[1700:])}


def events_files():
    """-> (genome FASTA, input FASTA).  The record added to the genome holds one window W = CCT N17 NGG and, behind it, one
    more copy of the 20-mer of the window's strand-1 guide B = rc(W) in front of CGG: B's reads align twice, those of the
    strand-0 guide A = W once.  The input holds the text of B in one record -- the reference meets B (forward) ahead of A
    (reverse) there -- and B's 20-mer with CGG in a second.  The groups of B and of B[0:20] + CGG print W, their read 0's
    first alignment being on the reverse strand, and so name A; A's own group names A.  A is named reject, accept, reject."""
    w = "CCTGATTGCAGTCAGGTCATCGG"
    b = mgr.mgc.rc(w)
    assert b.endswith("AGG") and w[20:] != "AGG"
    pad = "ATATATATATAT"
    genome = (mgr.BOWTIE / "genome.fa").read_text() + ">window\n" + pad + w + pad + b[:20] + "CGG" + pad + "\n"
    return genome, ">one\n" + pad + b + pad + "\n>two\n" + pad + b[:20] + "CGG" + pad + "\n"


def run_log(reference, run, batch_size, rnafold_page, offtarget_page, answers, work):
    """make_golden_results.run_reference under the changed configuration text -> (the output file, the log's text, what
    RNAfold's stand-in printed last)"""
    fasta = OUT / run["input"] if (OUT / run["input"]).exists() else \
        (mgr.OUT if run["input"].startswith("headers") else mgr.BOWTIE) / run["input"]
    plain, stand_in = mgr.CONFIG, mgr.mgc.STAND_IN
    text = mgba.config_text(batch_size, rnafold_page)
    if offtarget_page is not None:
        assert text.count(OFFTARGET_LINES) == 1
        text = text.replace(OFFTARGET_LINES, OFFTARGET_LINES.replace("5000000", str(offtarget_page)))
    if run.get("genome"):  # (the scores still come from the index of tests/golden/bowtie: any guide can be scored against it)
        assert text.count("{genome}") == 1
        text = text.replace("{genome}", str(OUT / run["genome"]))
    mgr.CONFIG = text
    if not answers:
        assert stand_in.count(ANSWER) == 1
        mgr.mgc.STAND_IN = stand_in.replace(ANSWER, "        if h % 5: out.write(line")
    try:
        data, log, fold = mgr.run_reference(reference, {k: v for k, v in run.items() if k != "genome"}, fasta, work)
        assert data is not None, log
        text = (pathlib.Path(work) / "out" / "golden-golden.log").read_text()
    finally:
        mgr.CONFIG, mgr.mgc.STAND_IN = plain, stand_in
    return data, text.replace(str(fasta.parent) + "/", ""), fold


def kept_text(log):
    """The log without the lines that name the machine's directories (each with the empty line behind it)."""
    out, lines, i = [], log.split("\n"), 0
    while i < len(lines):
        if any(d in lines[i] for d in DROPPED):
            assert lines[i].startswith(">>> ") and lines[i + 1] == "", lines[i]
            i += 2
            continue
        out.append(lines[i])
        i += 1
    return "\n".join(out)


def messages(log):
    return [line.split(":\t", 1)[1] for line in log.split("\n") if line.startswith(">>> ")]


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    base_runs = {r["name"]: r for r in mgr.runs() if r["name"] != "tab"}
    todo = [(name, name, 5000000, None, None, True) for name in base_runs]
    todo += [(mgba.name_of(*r), r[0], r[1], r[2], None, True) for r in mgba.RUNS]
    known = {t[0] for t in todo}
    todo += [(own_name(*r),) + r for r in OWN_RUNS]
    (OUT / MULTI).mkdir()
    for f, text in multi_inputs().items():
        (OUT / MULTI / f).write_text(text)
    base_runs[MULTI] = dict(base_runs["medium_page0"], name=MULTI, input=MULTI)
    todo.append((MULTI, MULTI, 5000000, None, None, True))
    genome, fasta = events_files()
    (OUT / "events_genome.fa").write_text(genome)
    (OUT / "events.fa").write_text(fasta)
    base_runs[EVENTS] = dict(base_runs["ultralow_page0"], name=EVENTS, input="events.fa", genome="events_genome.fa")
    todo.append((EVENTS, EVENTS, 5000000, None, None, True))
    files = {}
    kept, logs = [], {}
    for name, base, batch_size, rnafold_page, offtarget_page, answers in todo:
        with tempfile.TemporaryDirectory() as work:
            data, log, fold = run_log(reference, base_runs[base], batch_size, rnafold_page, offtarget_page, answers, work)
        if name in known:  # the file of the run is the one the other recipes keep
            whole = (mgr.OUT if name == base else mgba.OUT) / f"{name}.txt.gz"
            assert gzip.decompress(whole.read_bytes()) == data, name
        else:
            (OUT / f"{name}.txt.gz").write_bytes(gzip.compress(data, 9, mtime=0))
        files[name] = data
        if name in (MULTI, EVENTS):
            (OUT / f"{name}_fold.txt.gz").write_bytes(gzip.compress(fold.encode(), 9, mtime=0))
        log = kept_text(log)
        assert str(ROOT.parent) not in log and tempfile.gettempdir() not in log, f"{name}: a directory of this machine is left in the log"
        logs[name] = messages(log)
        kept.append(dict(base_runs[base], name=name, base=base, batch_size=batch_size, rnafold_page_length=rnafold_page,
                         offtarget_page_length=offtarget_page, own=name not in known, rnafold_answers=answers))
        (OUT / f"{name}.log.gz").write_bytes(gzip.compress(log.encode(), 9, mtime=0))
        print(f"{name}: {log.count(chr(10))} lines, {sum(m.startswith('Processing batch file') for m in logs[name])} batches")
    # what the tests over these logs cannot show without
    everything = [m for ms in logs.values() for m in ms]
    assert any(re.fullmatch(r"\t[1-9]\d* of \d+ erred here\.", m) for m in everything), "no batch with a row that erred"
    assert any(re.fullmatch(r"\t[1-9]\d* of \d+ not found in RNAfold output\.", m) for m in everything), "no batch with a row RNAfold did not answer"
    pairs = [(a, b, c) for ms in logs.values() for a, b, c in zip(ms, ms[1:], ms[2:]) if a == "Bowtie analysis."]
    assert any(b == "\tConstructing the Bowtie input file." and c == "\t\t0 guides in this page." for _, b, c in pairs), \
        "no empty selection under [bowtie2] page-length 0"
    assert any(b == "\t0 of 0 failed here." for _, b, _ in pairs), "no empty selection under a [bowtie2] page-length above 0"
    # [offtargetscore] page-length 5 changes no byte of the file; 0 does: Paginator.py:29-30 hands out the filter's generator,
    # writing the scorer's input (Crackling.py:748) consumes it, the loop of :789 sees nothing and no guide gets a score
    assert files["medium_page0_batch5000000_score5"] == gzip.decompress((mgr.OUT / "medium_page0.txt.gz").read_bytes())
    assert files["high_page0_batch64_score0"] != gzip.decompress((mgba.OUT / "high_page0_batch64.txt.gz").read_bytes())
    # a Bowtie `failed` that is no count of rows: the events run is one batch, and its file says how many rows end rejected
    at = logs[EVENTS].index("\tStarting to process the Bowtie results.")
    failed = int(re.fullmatch(r"\t([\d,]+) of [\d,]+ failed here\.", logs[EVENTS][at + 1]).group(1).replace(",", ""))
    rows = mgba.table(files[EVENTS])
    rejected = sum(r["passedBowtie"] == "0" for r in rows)
    print(f"{EVENTS}: Bowtie failed {failed}, rows that end rejected {rejected}")
    assert failed != rejected, "no batch whose Bowtie `failed` figure differs from its rejected rows"
    figures = [re.fullmatch(r"\tRemoving ([\d,]+) of .*", m) for m in logs[MULTI]]
    assert sum(1 for m in figures if m and m.group(1) != "0") > 1, "the directory run has duplicates in one file only"
    (OUT / "runs.json").write_text("[\n" + ",\n".join(json.dumps(r) for r in kept) + "\n]\n")
    for f in sorted(p for p in OUT.rglob("*") if p.is_file()):
        assert f.stat().st_size < 1 << 20, f
        print(f"{f.stat().st_size:8d} {f.relative_to(OUT)}")


# ---- configs/: what the reference's ConfigManager derives from a handful of INI files ---------------------------------------
# The files are kept with {dir} where the directory they were read in stood and {python} for an executable that exists
# everywhere; expected.json holds, per file, what ConfigManager.py made of it, paths relative to {dir}.
CONFIG_INI = """[general]
name = {name}
optimisation = medium
[consensus]
n = {n}
mm10db = {mm10db}
sgrnascorer2 = True
chopchop = True
[input]
exon-sequences = {{dir}}/{inputs}
offtarget-sites = {{dir}}/index.issl
gff-annotation = unused
bowtie2-index = {{dir}}/genome.fa
batch-size = 5000000
[output]
dir = {{dir}}/out
filename = guides.txt
delimiter = ,
[offtargetscore]
enabled = True
binary = {{python}}
method = and
threads = 1
page-length = 5000000
score-threshold = 75
max-distance = 4
[sgrnascorer2]
model = {{dir}}/model.txt
score-threshold = 0
[bowtie2]
binary = {{python}}
threads = 1
page-length = 0
[rnafold]
binary = {{python}}
threads = 1
page-length = 5000000
low_energy_threshold = -30
high_energy_threshold = -18
"""
CONFIG_CASES = {"plain": dict(name="plain", n=2, mm10db="True", inputs="single.fa"),
                "empty_name": dict(name="", n=2, mm10db="True", inputs="single.fa"),
                "directory": dict(name="dir", n=2, mm10db="True", inputs="in"),
                "glob": dict(name="glob", n=2, mm10db="True", inputs="in/*.fa"),
                "n_above_tools": dict(name="tools", n=3, mm10db="true", inputs="single.fa"),  # ('true' is not 'True')
                "output_exists": dict(name="exists", n=2, mm10db="True", inputs="single.fa")}
CONFIG_FILES = ["single.fa", "genome.fa", "index.issl", "model.txt", "in/b.fa", "in/a.fa", "in/c.txt", "out/exists-guides.txt"]
CONFIG_DRIVER = """import json, sys
from crackling.ConfigManager import ConfigManager
messages = []
cm = ConfigManager(sys.argv[1], messages.append)
out = dict(configured=bool(cm.isConfigured()), messages=messages, files=[], name=cm['general']['name'])
if cm.isConfigured():
    out['files'] = list(cm.getIterFilesToProcess())
    out.update(output=cm['output']['file'], rnafold_input=cm['rnafold']['input'], rnafold_output=cm['rnafold']['output'],
               config_name=cm.getConfigName())
print(json.dumps(out))
"""


def make_configs(reference):
    import os
    import subprocess
    out = OUT / "configs"
    out.mkdir()
    expected = {}
    for case, keys in CONFIG_CASES.items():
        template = CONFIG_INI.format(**keys)
        (out / f"{case}.ini").write_text(template)
        with tempfile.TemporaryDirectory() as work:
            work = pathlib.Path(work)
            for f in CONFIG_FILES:
                (work / f).parent.mkdir(parents=True, exist_ok=True)
                (work / f).write_text(">r\nACGT\n")
            (work / "run.ini").write_text(template.replace("{dir}", str(work)).replace("{python}", sys.executable))
            (work / "driver.py").write_text(CONFIG_DRIVER)
            env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
            r = subprocess.run([sys.executable, str(work / "driver.py"), str(work / "run.ini")], env=env, capture_output=True, text=True,
                               cwd=work, check=True)
            got = json.loads(r.stdout.strip().splitlines()[-1].replace(str(work), "{dir}"))
        if got["configured"] and not keys["name"]:
            stamp = got.pop("config_name")  # the time the recipe ran: kept as what it looks like
            assert re.fullmatch(r"\d{14}", stamp)
            for k in ("output", "rnafold_input", "rnafold_output"):
                got[k] = got[k].replace(stamp, "{time}")
        expected[case] = got
        print(case, got)
    assert expected["plain"]["configured"] and expected["empty_name"]["configured"]
    assert [f.split("/")[-1] for f in expected["directory"]["files"]] == ["c.txt", "b.fa", "a.fa"]
    assert sorted(f.split("/")[-1] for f in expected["glob"]["files"]) == ["a.fa", "b.fa"]
    assert not expected["n_above_tools"]["configured"] and not expected["output_exists"]["configured"]
    (out / "files.json").write_text(json.dumps(CONFIG_FILES) + "\n")
    (out / "expected.json").write_text(json.dumps(expected, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    make_goldens(ap.parse_args().reference)
    make_configs(ap.parse_args().reference)
