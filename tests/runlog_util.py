"""The one normaliser every comparison of logs goes through, and the goldens of tests/golden/runlog
(tools/make_golden_runlog.py): the reference's own log for every run of tests/golden/results and tests/golden/batches and
for the recipe's own runs.

normalise() drops what a log of this package may differ in from the reference's: the timestamp in front of a message, the
'| Calling:' and '| Finished' lines of Helpers.runner and the line 'Batchinator is writing to:' (each with the empty line
behind it), and the figures of the run-time lines.  Everything else must be equal line by line, empty lines included."""
import gzip
import json
import pathlib
import re
import zlib

import bowtie_util as bu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "runlog"
DROPPED = ("| Calling:", "| Finished", "Batchinator is writing to:")
_STAMP = re.compile(r">>> \d{4}-\d\d-\d\d \d\d:\d\d:\d\d:\d{6}:\t")
_BATCH_TIME = re.compile(r"This batch ran in .* \(dd hh:mm:ss\) or .* seconds")
_TOTAL_TIME = re.compile(r"Total run time \(dd hh:mm:ss\) or .* seconds")


def normalise(log):
    """-> the lines that are compared."""
    out, lines, i = [], log.split("\n"), 0
    while i < len(lines):
        line = lines[i]
        m = _STAMP.match(line)
        if m:
            message = line[m.end():]
            if message.startswith(DROPPED):
                assert lines[i + 1] == "", line
                i += 2
                continue
            message = _BATCH_TIME.sub("This batch ran in (dd hh:mm:ss) or seconds", message)
            message = _TOTAL_TIME.sub("Total run time (dd hh:mm:ss) or seconds", message)
            line = ">>> " + message
        out.append(line)
        i += 1
    return out


def same_log(got, want):
    got, want = normalise(got), normalise(want)
    bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, f"line {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r} ({len(bad)} lines differ)"
    assert len(got) == len(want), f"{len(got)} lines for {len(want)}: {(got + want)[min(len(got), len(want))]!r}"


def golden_runs():
    return json.loads((GOLDEN / "runs.json").read_text())


def golden_log(name):
    return gzip.decompress((GOLDEN / f"{name}.log.gz").read_bytes()).decode()


def golden_bytes(run):
    """The reference's output file of the run: the recipe's own, or the one tests/golden/results and batches keep.  Under
    [offtargetscore] page-length 0 the reference scores no guide (its file, kept beside the log, has '?' in the score
    columns); the package scores them as under any other page length: the file of the same run without that key."""
    import batches_util as bt
    import results_util as ru
    if run["own"] and run["offtarget_page_length"] == 0:
        return bt.golden_bytes(run["name"][:-len("_score0")])
    if run["own"]:
        return gzip.decompress((GOLDEN / f"{run['name']}.txt.gz").read_bytes())
    return ru.golden_bytes(run["name"]) if run["name"] == run["base"] else bt.golden_bytes(run["name"])


def golden_inputs(run):
    """[(the input's name as the run's log prints it, its bytes)] in the order the reference reads them: the run's file, or
    the files of its directory in reverse sorted order."""
    import results_util as ru
    if (GOLDEN / run["input"]).is_dir():
        return [(f"{run['input']}/{p.name}", p.read_bytes()) for p in sorted((GOLDEN / run["input"]).iterdir(), reverse=True)]
    if (GOLDEN / run["input"]).exists():
        return [(run["input"], (GOLDEN / run["input"]).read_bytes())]
    return [(run["input"], ru.golden_input(run))]


def golden_genome(run):
    """The FASTA bytes of the genome the run's Bowtie step works on: its own, or the one of tests/golden/bowtie."""
    return (GOLDEN / run["genome"] if run.get("genome") else bu.GOLDEN / "genome.fa").read_bytes()


def golden_source(run):
    """The directory the run's input is named from."""
    import results_util as ru
    if (GOLDEN / run["input"]).exists():
        return GOLDEN
    return ru.GOLDEN if run["input"].startswith("headers") else bu.GOLDEN


def golden_fold_text(run):
    """What RNAfold's stand-in printed for (a superset of) the guides of the run; where the run's stand-in left answers out
    (rnafold_answers false), without the pairs it left out: those whose line has a CRC-32 that 5 divides."""
    import results_util as ru
    kept = GOLDEN / f"{run['name']}_fold.txt.gz"
    if kept.exists():
        return gzip.decompress(kept.read_bytes()).decode()
    text = ru.golden_fold_text(dict(run, name=run["base"]))
    if run["rnafold_answers"]:
        return text
    lines = text.splitlines()
    # (the stand-in echoes its input line; the recipe's rule looks at that line)
    return "".join(a + "\n" + b + "\n" for a, b in zip(lines[0::2], lines[1::2]) if zlib.crc32(a.encode()) % 5)


def golden_keywords(run):
    """The keywords of crackling_amd.pipeline.run's config for a run of runs.json, with the page lengths a RunLog reads."""
    import batches_util as bt
    kw = bt.golden_keywords(run)
    if run["offtarget_page_length"] is not None:
        kw["offtarget_page_length"] = run["offtarget_page_length"]
    return kw


assert bu.GOLDEN.exists()
