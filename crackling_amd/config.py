"""The reference's configuration file: `load(path) -> RunConfig` applies the rules of ConfigManager.py for INI files
(configparser without interpolation) and builds the mapping crackling_amd.pipeline.batches takes.

What is derived, as the reference derives it: the run's name ([general] name, or the time as %Y%m%d%H%M%S when it is
empty); the output file <dir>/<name>-<filename>; the log <dir>/<general name>-<name>.log and the error log with .errlog
(the first part is [general] name as written, so an empty name gives '-<time>.log'); RNAfold's exchange files
<dir>/<name>-rnafold-input.txt and -output.txt; the list of input files -- a file stands for itself, a directory for its
top-level files in reverse sorted order (as GuideSet.extract takes a directory), anything else is a glob; and the two
refusals of _validateConfig with its messages: [consensus] n above the number of tools switched on (counted by the
literal string 'True', as getNumberToolsInConsensus does) and an output file that exists already.  A refused
configuration has ok == False and its messages; nothing is written.

Deliberate differences:
  * the v1.0.0 configuration, a Python dictionary in a file named without its extension, is refused with a message; it is
    not converted
  * only [rnafold] binary must be executable (shutil.which): it is the one program that is run.  [offtargetscore] binary
    and [bowtie2] binary are never run and not checked
  * the Bowtie step needs the genome's text, not a Bowtie2 index: the optional key [input] genome names a FASTA file, a
    directory or a glob; without it [input] bowtie2-index itself must name a FASTA file or a directory; otherwise the
    configuration is refused with a message that names the key
  * [input] offtarget-sites is opened as an .issl index
  * [sgrnascorer2] model may also name an .npz file with the arrays sv [n_sv, 80], coef [n_sv] and intercept: the model
    without the pickle around it
  * [offtargetscore] page-length reaches the log only: no byte of the output file depends on it (under 0 the reference
    scores no guide at all: Paginator.py:29-30)
"""
import configparser
import glob
import os
import shutil
import time


class RunConfig:
    """ok, messages, name, output_file, log_file, errlog_file, rnafold_input, rnafold_output, files (the inputs, in the order
    they are read), genome (FASTA paths of the genome's text), index (the .issl file), rnafold_binary, rnafold_threads,
    parser (the ConfigParser) and, when ok, `pipeline`: the mapping of crackling_amd.pipeline.batches without its model,
    which `pipeline_config()` adds (it reads the sgRNAScorer2 model file)."""

    def __init__(self):
        self.ok = False
        self.messages = []
        self.parser = None
        self.name = self.output_file = self.log_file = self.errlog_file = self.rnafold_input = self.rnafold_output = None
        self.files, self.genome = [], []
        self.index = self.rnafold_binary = self.model_path = None
        self.rnafold_threads = "1"
        self.pipeline = {}

    def pipeline_config(self):
        """`pipeline` with the sgRNAScorer2 model loaded when the tool is switched on: the reference's joblib file
        (consensus.load_sgrnascorer2), or, for a path that ends in .npz, the arrays sv, coef and intercept themselves."""
        from .consensus import load_sgrnascorer2
        config = dict(self.pipeline)
        if config["sgrnascorer2"]:
            if str(self.model_path).endswith(".npz"):
                import numpy as np
                z = np.load(self.model_path)
                config["model"] = (z["sv"], z["coef"], float(z["intercept"]))
            else:
                config["model"] = load_sgrnascorer2(self.model_path)
        return config


def _files(path):
    """ConfigManager._createListOfFilesToAnalyse, top level only for a directory."""
    if os.path.isdir(path):
        return [os.path.join(path, f) for f in sorted(os.listdir(path), reverse=True) if os.path.isfile(os.path.join(path, f))]
    if os.path.isfile(path):
        return [path]
    return glob.glob(path)


def load(path):
    cfg = RunConfig()
    say = cfg.messages.append
    path = os.fspath(path)
    if os.path.splitext(path)[1] == "":
        say("A configuration without a file extension is the v1.0.0 Python-dictionary format, which is not read here. "
            "Convert it to the INI format of v1.1.0 (see the sample config.ini of Crackling).")
        return cfg
    c = cfg.parser = configparser.ConfigParser(interpolation=None)
    try:
        with open(path, "r") as fp:
            c.read_file(fp)
    except Exception as e:  # (as the reference: whatever stops the read is printed and the configuration refused)
        say(str(e))
        return cfg
    try:
        return _derive(cfg, c)
    except KeyError as e:  # a section or a key the run needs
        cfg.ok, cfg.pipeline, cfg.files = False, {}, []
        say(f"The configuration lacks {e}.")
        return cfg


def _derive(cfg, c):
    say = cfg.messages.append
    passed = True
    if not shutil.which(c["rnafold"]["binary"]):
        passed = False
        say(f"This binary cannot be executed: {c['rnafold']['binary']}")
    tools = sum(c["consensus"][k] == "True" for k in ("mm10db", "sgrnascorer2", "chopchop"))
    n = int(c["consensus"]["n"])
    if n > tools:
        passed = False
        say(f"The consensus approach is incorrectly set. You have specified {tools} to be ran but the n-value is {n}. "
            f"Change n to be <= {tools}.")
    general = c["general"]["name"]
    cfg.name = name = general or time.strftime("%Y%m%d%H%M%S", time.localtime())
    out = c["output"]["dir"]
    cfg.output_file = os.path.join(out, f"{name}-{c['output']['filename']}")
    if os.path.exists(cfg.output_file):
        passed = False
        say(f"The output file already exists: {cfg.output_file}")
        say("To avoid loosing data, please rename your output file.")
    cfg.log_file = os.path.join(out, f"{general}-{name}.log")
    cfg.errlog_file = os.path.join(out, f"{general}-{name}.errlog")
    cfg.rnafold_input = os.path.join(out, f"{name}-rnafold-input.txt")
    cfg.rnafold_output = os.path.join(out, f"{name}-rnafold-output.txt")
    cfg.rnafold_binary, cfg.rnafold_threads = c["rnafold"]["binary"], c["rnafold"]["threads"]
    cfg.index = c["input"]["offtarget-sites"]
    cfg.model_path = c["sgrnascorer2"]["model"]
    enabled = c["offtargetscore"].getboolean("enabled")
    if enabled:
        key = "genome" if c["input"].get("genome") else "bowtie2-index"
        where = c["input"][key]
        if os.path.isdir(where):
            cfg.genome = [where] if os.listdir(where) else []  # (Genome.open reads a directory by its own rule)
        elif os.path.isfile(where):
            cfg.genome = [where]
        else:
            cfg.genome = sorted(glob.glob(where)) if key == "genome" else []
        if not cfg.genome:
            passed = False
            say(f"[input] {key} = {where} names no FASTA file: the Bowtie step reads the genome's text, not a Bowtie2 index. "
                "Name a FASTA file, a directory or a glob under [input] genome.")
    if passed:
        cfg.files = _files(c["input"]["exon-sequences"])
        delimiter = c["output"]["delimiter"]
        cfg.pipeline = dict(
            optimisation=c["general"]["optimisation"], n=n, mm10db=c["consensus"].getboolean("mm10db"),
            chopchop=c["consensus"].getboolean("chopchop"), sgrnascorer2=c["consensus"].getboolean("sgrnascorer2"),
            sgrna_threshold=float(c["sgrnascorer2"]["score-threshold"]), low_energy=float(c["rnafold"]["low_energy_threshold"]),
            high_energy=float(c["rnafold"]["high_energy_threshold"]), offtargetscore=bool(enabled),
            method=c["offtargetscore"]["method"], score_threshold=float(c["offtargetscore"]["score-threshold"]),
            max_distance=int(c["offtargetscore"]["max-distance"]), batch_size=int(c["input"]["batch-size"]),
            page_length=int(c["bowtie2"]["page-length"]), rnafold_page_length=int(c["rnafold"]["page-length"]),
            offtarget_page_length=int(c["offtargetscore"]["page-length"]), delimiter=delimiter)
    cfg.ok = passed
    return cfg
