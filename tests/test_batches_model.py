"""CPU: the host model of a batched run (tests/batches_util.py) pinned byte for byte to the reference's own output files for
several [input] batch-size and [rnafold] page-length (tests/golden/batches, tools/make_golden_batches.py), and the
model's boundaries checked against a count done the slow way."""
import csv

import numpy as np
import pytest

import batches_util as bt
import results_util as ru

RUNS = bt.golden_runs()
IDS = [r["name"] for r in RUNS]


def test_the_runs_the_recipe_keeps():
    assert IDS == ["medium_page0_batch64", "medium_page0_batch50", "medium_page0_batch17", "medium_page0_batch5000000_fold0",
                   "high_page0_batch64", "medium_page7_batch17_fold5", "ultralow_page7_batch17", "headers_batch64_fold3",
                   "headers_batch1_fold3", "headers_batch203_fold3", "noscore_batch50"]
    for run in RUNS:
        assert run["base"] in [r["name"] for r in ru.golden_runs()] and run["batch_size"] > 0
    # the batches matter in these files and cannot in that one
    for name in ("medium_page0_batch64", "medium_page0_batch50", "medium_page0_batch17"):
        assert bt.golden_bytes(name) != ru.golden_bytes("medium_page0")
    assert bt.golden_bytes("high_page0_batch64") != ru.golden_bytes("high_page0")
    assert bt.golden_bytes("headers_batch203_fold3") == ru.golden_bytes("headers")
    rows = list(csv.DictReader(bt.golden_bytes("medium_page0_batch5000000_fold0").decode().splitlines(keepends=True)))
    assert len(rows) == 203 and all(r["passedSecondaryStructure"] == "?" and r["ssL1"] == "?" for r in rows)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_model_writes_the_reference_file(run):
    stages, calls = bt.host_stages(run, bt.golden_fold_text(run))
    got, offsets = ru.model_table(**stages)
    want = bt.golden_bytes(run["name"])
    assert got == want
    assert offsets.tolist() == np.cumsum([len(x) for x in want.splitlines(keepends=True)]).tolist()
    if run["rnafold_page_length"] == 0:
        assert calls == 0
    elif run["rnafold_page_length"] is None:
        assert calls == (1 if len(stages["fold_rows"]) else 0)
    else:
        assert calls >= len(stages["fold_rows"]) / run["rnafold_page_length"]


def slow_starts(listed, n, batch_size, page_length):
    """Row by row: a page ends when it is full or when the next listed row lies in another batch."""
    starts, in_page, batch = [], 0, None
    for k, j in enumerate(listed):
        b = int(j) // batch_size if batch_size else 0
        if b != batch or (page_length and in_page == page_length):
            starts.append(k)
            in_page, batch = 0, b
        in_page += 1
    return starts + [len(listed)] if len(listed) else [0]


def test_page_starts_against_a_row_by_row_count():
    rng = np.random.default_rng(5)
    for n in (0, 1, 40):
        for density in (0.0, 0.3, 1.0):
            listed = np.nonzero(rng.random(n) < density)[0] if density < 1 else np.arange(n)
            for batch_size in (0, 1, 7, max(n - 1, 1), n, n + 1):
                for page_length in (0, 1, 3, 5000000):
                    got = bt.page_starts(listed, n, batch_size, page_length).tolist()
                    assert got == slow_starts(listed, n, batch_size, page_length), (n, density, batch_size, page_length)
                    assert got[0] == 0 and got[-1] == len(listed) and all(a < b for a, b in zip(got, got[1:]))
    assert bt.uniform_starts(10, 4).tolist() == [0, 4, 8, 10] and bt.uniform_starts(10, 0).tolist() == [0, 10]
    assert bt.uniform_starts(0, 3).tolist() == [0]


def test_paged_rows_equal_the_model_for_uniform_pages():
    _, model, _, sigs = __import__("bowtie_util").adversarial()
    sigs = sigs[:600]
    for page_length in (0, 1, 7, len(sigs)):
        got = bt.paged_rows(model, sigs, bt.uniform_starts(len(sigs), page_length))
        assert got.tobytes() == model.rows(sigs, page_length).tobytes()
    with_empty = bt.paged_rows(model, sigs, [0, 0, 7, 7, 7, 14, len(sigs), len(sigs)])
    assert with_empty.tobytes() == bt.paged_rows(model, sigs, [0, 7, 14, len(sigs)]).tobytes()
