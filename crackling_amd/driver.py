"""A Crackling run from its configuration file: `python -m crackling_amd -c config.ini` (Crackling_cli.py) and
`driver.run(path)` in process.  The configuration is read by crackling_amd.config; the genome and the index are opened,
pipeline.run_to_file writes the reference's output file, and a crackling_amd.RunLog writes the reference's log beside it,
with an error log (.errlog) that is empty after a clean run and holds the traceback after a failed one.

RNAfold is the one program that is run, as the reference runs it: `<binary> --noPS -j<threads> -i <input> -o`, once per
page, each time in a fresh child process.  Its input is written from the device to the configured path
(issl_folds_input_write); the child works in a temporary directory of the run, and the RNAfold_output.fold it leaves there
is moved to the configured output path and read from it (issl_folds_read_file).  Both files are removed at the end, as
Crackling.py:857-869 does.
"""
import argparse
import os
import shlex
import shutil
import subprocess
import sys
import tempfile
import traceback

from . import config as config_module


class RNAfold:
    """The RNAfold exchange of one run (pipeline: an object with fold_page is handed the Folds and a page of it)."""

    def __init__(self, cfg, log):
        self.cfg, self.log = cfg, log
        self.work = tempfile.TemporaryDirectory(prefix="crackling-rnafold-")

    def fold_page(self, folds, first, n):
        cfg = self.cfg
        if os.path.exists(cfg.rnafold_output):
            os.remove(cfg.rnafold_output)
        folds.write_input(cfg.rnafold_input, first, n)
        command = shlex.split(cfg.rnafold_binary) + ["--noPS", f"-j{cfg.rnafold_threads}", "-i", os.path.abspath(cfg.rnafold_input), "-o"]
        self.log.say(f"| Calling: {command}")
        subprocess.run(command, check=True, cwd=self.work.name, stdin=subprocess.DEVNULL)
        self.log.say("| Finished")
        shutil.move(os.path.join(self.work.name, "RNAfold_output.fold"), cfg.rnafold_output)
        folds.read_file(cfg.rnafold_output, first, n)

    def __call__(self, text):
        raise TypeError("the driver's RNAfold works on the Folds of the run (rnafold_reader 'device')")

    def close(self):
        self.work.cleanup()
        for path in (self.cfg.rnafold_input, self.cfg.rnafold_output):
            try:
                os.remove(path)
            except OSError:
                pass


def run(path, say=print, device=0):
    """-> 0 after a clean run; 0 too for a refused configuration, as the reference exits (its messages through `say`, nothing
    written); 1 when the run failed: the traceback is in the error log."""
    from . import Genome, IsslIndex, RunLog, pipeline
    cfg = config_module.load(path)
    for message in cfg.messages:
        say(f"configMngr says: {message}")
    if not cfg.ok:
        say("Something went wrong with reading the configuration.")
        return 0
    with open(cfg.log_file, "w+") as log_fp, open(cfg.errlog_file, "w+") as err_fp:
        log = RunLog(cfg.pipeline, out=log_fp)
        rnafold = RNAfold(cfg, log)
        genome = index = None
        try:
            config = dict(cfg.pipeline_config(), device=device)
            if config["offtargetscore"]:
                genome = Genome.open(cfg.genome, device)
                index = IsslIndex.open(cfg.index).upload(device)
            pipeline.run_to_file(cfg.output_file, cfg.files, genome, index, config, rnafold, log=log)
            return 0
        except BaseException:
            traceback.print_exc(file=err_fp)
            err_fp.flush()
            return 1
        finally:
            rnafold.close()
            if index is not None:
                index.close()
            if genome is not None:
                genome.close()


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m crackling_amd")
    parser.add_argument("-c", "--config", required=True, metavar="INI", help="the run's configuration in the reference's INI format")
    args = parser.parse_args(argv)
    return run(args.config)


if __name__ == "__main__":
    sys.exit(main())
