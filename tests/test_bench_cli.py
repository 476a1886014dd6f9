"""bench.py's own options on the GPU box, at a small size: a plain run times exactly --steps steps and measures nothing
beyond its headline figure; --dump-outputs writes the scores of the last timed step (float64, input order), the same on
every run with the same arguments and the same as --dump-scores'; --full adds the stage breakdown and the extras."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--sites", "3000000", "--guides", "30000", "--spinup-ms", "0"]


def _bench(*extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *ARGS, *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"), "--dump-scores", str(tmp_path / "a.npz"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "guides/s" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(30000 * 1e3 / line["ms_per_step"])
        assert line["config"]["full"] is False
        assert line["kernel_ms"] is None and line["extras"] is None and "cpu_baseline" not in line
        assert line["ms_per_step_without_event_pairs"] is None and line["roofline"]["avg_launch_ms"] > 0
    ref = np.load(tmp_path / "a.npz")
    for name in ("mit", "cfd"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == (30000,)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        assert np.array_equal(x.view(np.uint64), ref[name].view(np.uint64))
    assert (ref["mit"] < 100).any()


def test_full_run_adds_the_breakdown_and_extras():
    line = _bench("--full", "--no-cpu-baseline", "--no-cli")
    assert line["config"]["full"] is True and line["steps"] == 3
    assert set(line["kernel_ms"]) == {"bin", "scan", "verify", "group", "replay", "pipeline"}
    assert line["roofline"]["avg_launch_ms_alone"] > 0 and line["ms_per_step_without_event_pairs"] > 0
    assert {"north_star_10k_guides", "hbm_regime_64_guides", "whole_bucket_scan", "host_pointer_entry"} <= set(line["extras"])
