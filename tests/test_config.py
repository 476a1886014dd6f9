"""CPU: crackling_amd.config.load against what the reference's own ConfigManager derived from the INI files of
tests/golden/runlog/configs (expected.json, tools/make_golden_runlog.py): the name, the output file, RNAfold's exchange
files, the list of inputs, configured or refused and the messages; then the rules the package adds (the log's name, the
v1.0.0 refusal, [input] genome / bowtie2-index, the one binary that is checked) and the mapping for the pipeline."""
import json
import pathlib
import re
import sys

import pytest

from crackling_amd import config

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "runlog" / "configs"
EXPECTED = json.loads((GOLDEN / "expected.json").read_text())
FILES = json.loads((GOLDEN / "files.json").read_text())


def lay_out(tmp_path, case, edit=lambda text: text):
    """The files the recipe laid out, and the INI file with its directory and an executable filled in."""
    for f in FILES:
        (tmp_path / f).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / f).write_text(">r\nACGT\n")
    text = (GOLDEN / f"{case}.ini").read_text().replace("{dir}", str(tmp_path)).replace("{python}", sys.executable)
    (tmp_path / "run.ini").write_text(edit(text))
    return tmp_path / "run.ini"


def there(tmp_path, value, stamp=""):
    return value.replace("{dir}", str(tmp_path)).replace("{time}", stamp)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_load_against_the_reference(tmp_path, case):
    want = EXPECTED[case]
    ini = lay_out(tmp_path, case)
    before = sorted(str(p) for p in tmp_path.rglob("*"))
    cfg = config.load(ini)
    assert cfg.ok == want["configured"]
    assert cfg.messages == [there(tmp_path, m) for m in want["messages"]]
    stamp = ""
    if want["name"] == "":
        assert re.fullmatch(r"\d{14}", cfg.name)
        stamp = cfg.name
    else:
        assert cfg.name == want["name"]
    if want["configured"]:
        assert cfg.output_file == there(tmp_path, want["output"], stamp)
        assert cfg.rnafold_input == there(tmp_path, want["rnafold_input"], stamp)
        assert cfg.rnafold_output == there(tmp_path, want["rnafold_output"], stamp)
        files = [there(tmp_path, f) for f in want["files"]]
        # (glob.glob gives the order of the file system)
        assert (sorted(cfg.files) == sorted(files)) if case == "glob" else (cfg.files == files)
        out = str(tmp_path / "out")
        assert cfg.log_file == f"{out}/{want['name']}-{cfg.name}.log" and cfg.errlog_file == f"{out}/{want['name']}-{cfg.name}.errlog"
        assert cfg.pipeline["batch_size"] == 5000000 and cfg.pipeline["offtarget_page_length"] == 5000000
        assert cfg.pipeline["page_length"] == 0 and cfg.pipeline["rnafold_page_length"] == 5000000
        assert cfg.pipeline["optimisation"] == "medium" and cfg.pipeline["n"] == 2 and cfg.pipeline["method"] == "and"
        assert cfg.pipeline["mm10db"] is True and cfg.pipeline["offtargetscore"] is True and cfg.pipeline["delimiter"] == ","
        assert cfg.genome == [str(tmp_path / "genome.fa")] and cfg.index == str(tmp_path / "index.issl")
    else:
        assert cfg.pipeline == {} and cfg.files == []
    assert sorted(str(p) for p in tmp_path.rglob("*")) == before, "load writes nothing"


def test_v1_0_0_dictionary_is_refused(tmp_path):
    (tmp_path / "settings").write_text("CONFIG = {}\n")
    cfg = config.load(tmp_path / "settings")
    assert not cfg.ok and len(cfg.messages) == 1 and "v1.0.0" in cfg.messages[0]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["settings"], "nothing is converted"


def test_genome_key_and_bowtie2_index_rule(tmp_path):
    no_fasta = lambda text: text.replace(f"bowtie2-index = {tmp_path}/genome.fa", f"bowtie2-index = {tmp_path}/bt2/genome")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", no_fasta))
    assert not cfg.ok and len(cfg.messages) == 1 and "[input] bowtie2-index" in cfg.messages[0] and "[input] genome" in cfg.messages[0]
    with_key = lambda text: no_fasta(text).replace("batch-size", f"genome = {tmp_path}/in/*.fa\nbatch-size")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", with_key))
    assert cfg.ok and cfg.genome == [str(tmp_path / "in" / "a.fa"), str(tmp_path / "in" / "b.fa")]
    as_dir = lambda text: text.replace(f"bowtie2-index = {tmp_path}/genome.fa", f"bowtie2-index = {tmp_path}/in")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", as_dir))
    assert cfg.ok and cfg.genome == [str(tmp_path / "in")]
    bad_key = lambda text: text.replace("batch-size", f"genome = {tmp_path}/nothing*\nbatch-size")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", bad_key))
    assert not cfg.ok and "[input] genome" in cfg.messages[0]
    # without the specificity stage no genome is asked for
    off = lambda text: no_fasta(text).replace("enabled = True", "enabled = False")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", off))
    assert cfg.ok and cfg.genome == [] and cfg.pipeline["offtargetscore"] is False


def test_only_rnafold_must_be_executable(tmp_path):
    others = lambda text: text.replace(  # noqa: E731
        f"[bowtie2]\nbinary = {sys.executable}", "[bowtie2]\nbinary = /nonexistent/bowtie2").replace(
        f"[offtargetscore]\nenabled = True\nbinary = {sys.executable}", "[offtargetscore]\nenabled = True\nbinary = /nonexistent/scorer")
    cfg = config.load(lay_out(tmp_path, "plain", others))
    assert cfg.ok and cfg.messages == []
    rnafold = lambda text: text.replace(f"[rnafold]\nbinary = {sys.executable}", "[rnafold]\nbinary = /nonexistent/RNAfold")  # noqa: E731
    cfg = config.load(lay_out(tmp_path, "plain", rnafold))
    assert not cfg.ok and cfg.messages == ["This binary cannot be executed: /nonexistent/RNAfold"]


def test_a_missing_key_refuses_the_configuration(tmp_path):
    cfg = config.load(lay_out(tmp_path, "plain", lambda text: text.replace("batch-size = 5000000\n", "")))
    assert not cfg.ok and cfg.messages == ["The configuration lacks 'batch-size'."] and cfg.pipeline == {} and cfg.files == []
    cfg = config.load(lay_out(tmp_path, "plain", lambda text: text.replace("[bowtie2]", "[bowtie]")))
    assert not cfg.ok and cfg.messages == ["The configuration lacks 'bowtie2'."]


def test_tools_are_counted_by_the_literal_true(tmp_path):
    """'true' switches mm10db on for getboolean and does not count for n: the reference's rule, kept."""
    cfg = config.load(lay_out(tmp_path, "n_above_tools", lambda text: text.replace("n = 3", "n = 2")))
    assert cfg.ok and cfg.pipeline["mm10db"] is True and cfg.pipeline["n"] == 2
