"""GPU: `python -m crackling_amd -c <ini>` in a fresh child process for two golden runs (medium_page7_batch17_fold5 and the
directory run): the output file's bytes, the log under the normaliser of tests/runlog_util.py, an empty .errlog, RNAfold's
exchange files removed; a second invocation is refused because the output file exists and changes nothing.  RNAfold is a
replay stand-in the test writes: it answers every input line with the two lines recorded for it in the golden fold text
and writes RNAfold_output.fold into its working directory."""
import os
import pathlib
import subprocess
import sys

import pytest

import consensus_util as cu
import bowtie_util as bu
import runlog_util as rl

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
RUNS = {r["name"]: r for r in rl.golden_runs()}
STAND_IN = """#!{python} -IS
import sys
answers = {{}}
lines = open({fold!r}).read().splitlines()
for first, second in zip(lines[0::2], lines[1::2]):
    answers[first.rstrip().replace("U", "T")] = (first, second)
with open(sys.argv[sys.argv.index("-i") + 1]) as asked, open("RNAfold_output.fold", "w") as out:
    for line in asked:
        pair = answers.get(line.rstrip("\\n").replace("U", "T"))
        if pair:
            out.write(pair[0] + "\\n" + pair[1] + "\\n")
"""
INI = """[general]
name = golden
optimisation = {optimisation}
[consensus]
n = {n}
mm10db = {mm10db}
sgrnascorer2 = {sgrnascorer2}
chopchop = {chopchop}
[input]
exon-sequences = {input}
offtarget-sites = {issl}
gff-annotation = unused
bowtie2-index = {genome}
batch-size = {batch_size}
[output]
dir = {outdir}
filename = guides.txt
delimiter = {delimiter}
[offtargetscore]
enabled = {enabled}
binary = not-run
method = {method}
threads = 1
page-length = {offtarget_page}
score-threshold = {score_threshold}
max-distance = {max_distance}
[sgrnascorer2]
model = {model}
score-threshold = {sgrna_threshold}
[bowtie2]
binary = not-run
threads = 1
page-length = {page_length}
[rnafold]
binary = {rnafold}
threads = 1
page-length = {rnafold_page}
low_energy_threshold = {low_energy}
high_energy_threshold = {high_energy}
"""


def invoke(ini, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "crackling_amd", "-c", str(ini)], cwd=cwd, env=env,
                          capture_output=True, text=True, stdin=subprocess.DEVNULL)


@pytest.mark.parametrize("name", ["medium_page7_batch17_fold5", "multi"])
def test_command_line_run_leaves_the_reference_files(tmp_path, name):
    run = RUNS[name]
    fold = tmp_path / "fold.txt"
    fold.write_text(rl.golden_fold_text(run))
    rnafold = tmp_path / "rnafold_replay"
    rnafold.write_text(STAND_IN.format(python=sys.executable, fold=str(fold)))
    rnafold.chmod(0o755)
    out = tmp_path / "out"
    out.mkdir()
    keys = {k: run[k] for k in ("optimisation", "n", "mm10db", "sgrnascorer2", "chopchop", "batch_size", "delimiter", "enabled", "method",
                                "score_threshold", "max_distance", "sgrna_threshold", "page_length", "low_energy", "high_energy")}
    ini = tmp_path / "golden.ini"
    ini.write_text(INI.format(input=run["input"], issl=bu.GOLDEN / "index.issl", genome=bu.GOLDEN / "genome.fa", outdir=out,
                              model=cu.GOLDEN / "model.npz", rnafold=rnafold,
                              offtarget_page=5000000 if run["offtarget_page_length"] is None else run["offtarget_page_length"],
                              rnafold_page=5000000 if run["rnafold_page_length"] is None else run["rnafold_page_length"], **keys))
    r = invoke(ini, rl.golden_source(run))
    assert r.returncode == 0, r.stdout + r.stderr + (out / "golden-golden.errlog").read_text()
    assert (out / "golden-guides.txt").read_bytes() == rl.golden_bytes(run)
    rl.same_log((out / "golden-golden.log").read_text(), rl.golden_log(name))
    assert (out / "golden-golden.errlog").read_text() == ""
    assert sorted(p.name for p in out.iterdir()) == ["golden-golden.errlog", "golden-golden.log", "golden-guides.txt"]
    # once more: refused, because the output file exists, and nothing changes
    before = {p.name: p.read_bytes() for p in out.iterdir()}
    r = invoke(ini, rl.golden_source(run))
    assert r.returncode == 0 and f"configMngr says: The output file already exists: {out}/golden-guides.txt" in r.stdout
    assert "Something went wrong with reading the configuration." in r.stdout
    assert {p.name: p.read_bytes() for p in out.iterdir()} == before


def test_an_input_without_a_match_is_refused_by_name(tmp_path):
    """The reference divides by zero at Crackling.py:254 before it has written anything: the run fails, the error log names
    the file, and no output file is left."""
    run = RUNS["medium_page0"]
    (tmp_path / "inputs").mkdir()
    (tmp_path / "inputs" / "b_guides.fa").write_bytes((bu.GOLDEN / "input.fa").read_bytes())
    (tmp_path / "inputs" / "a_none.fa").write_text(">nothing here\nATATATATATATATATATATATATATATATATAT\n")
    out = tmp_path / "out"
    out.mkdir()
    keys = {k: run[k] for k in ("optimisation", "n", "mm10db", "sgrnascorer2", "chopchop", "batch_size", "delimiter", "enabled", "method",
                                "score_threshold", "max_distance", "sgrna_threshold", "page_length", "low_energy", "high_energy")}
    ini = tmp_path / "golden.ini"
    ini.write_text(INI.format(input=tmp_path / "inputs", issl=bu.GOLDEN / "index.issl", genome=bu.GOLDEN / "genome.fa", outdir=out,
                              model=cu.GOLDEN / "model.npz", rnafold=sys.executable, offtarget_page=5000000, rnafold_page=5000000, **keys))
    r = invoke(ini, tmp_path)
    assert r.returncode == 1
    errlog = (out / "golden-golden.errlog").read_text()
    assert "Traceback" in errlog and "a_none.fa" in errlog
    assert sorted(p.name for p in out.iterdir()) == ["golden-golden.errlog", "golden-golden.log"]
