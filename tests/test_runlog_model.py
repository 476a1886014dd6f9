"""CPU: the host model of the log's figures (tests/runlog_model.py) through crackling_amd.RunLog against the reference's own
logs (tests/golden/runlog, tools/make_golden_runlog.py): every message of every batch, line by line, under the one
normaliser of tests/runlog_util.py.  This pins the text rules of RunLog -- the order of the blocks, which of them a
configuration prints, the page lines of Paginator.py, the two page-length-0 quirks -- and the model the GPU tests lean on."""
import numpy as np
import pytest

import crackling_amd as ca
import batches_util as bt
import bowtie_util as bu
import runlog_model as rm
import runlog_util as rl

RUNS = rl.golden_runs()
IDS = [r["name"] for r in RUNS]
_models = {}


def model_of(run):
    """Runs that differ only in [offtargetscore] page-length share their stages."""
    key = (run["base"], run["batch_size"], run["rnafold_page_length"], run["rnafold_answers"])
    if key not in _models:
        _models[key] = rm.Run(run, rl.golden_fold_text(run))
    m = _models[key]
    m.run = run
    return m


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_model_through_runlog_is_the_reference_log(run):
    log = model_of(run).feed(ca.RunLog(rl.golden_keywords(run)))
    rl.same_log(log.text(), rl.golden_log(run["name"]))


def test_goldens_hold_what_the_counts_can_get_wrong():
    """The conditions of the recipe, seen from the model: rows that erred, rows RNAfold did not answer, an empty selection
    under both kinds of page length, empty fold lists, several off-target pages in a batch, and a batch whose Bowtie
    `failed` differs from its rejected rows (the events run, on a genome of its own)."""
    seen = set()
    for run in RUNS:
        m = model_of(run)
        batches, page_failed, not_found = m.counts()
        events = m.batch_events(batches)
        assert sum(events) == sum(m.events)
        for b, e in zip(batches, events):
            if run["enabled"] and e != b["bowtie_rejected"]:
                assert run["name"] == "events" and e == b["bowtie_rejected"] + 1
                seen.add("events differ from rejected rows")
            if b["ss_erred"]:
                seen.add("erred")
            if b["ss_not_found"] and run["rnafold_page_length"] != 0:
                seen.add("not found")
            if run["enabled"] and b["selected_first"] == b["selected_end"]:
                seen.add("empty selection, page length %s 0" % ("above" if run["page_length"] else "of"))
            if run["mm10db"] and b["fold_first"] == b["fold_end"]:
                seen.add("empty fold list")
            if b["page_end"] - b["page_first"] > 1:
                seen.add("several off-target pages")
        assert len(not_found) == sum(int(b["ss_not_found"]) for b in batches)
    assert seen == {"events differ from rejected rows", "erred", "not found", "empty selection, page length above 0",
                    "empty selection, page length of 0", "empty fold list", "several off-target pages"}, seen


def test_bowtie_events_count_every_change_to_rejected():
    """A site named reject, accept, reject counts twice and ends rejected; named reject, accept it counts once and ends
    accepted (runlog_model.constructed_page)."""
    genome, guides, a = rm.constructed_page()
    model = bu.Model([genome])
    own = model.counts(np.array([bu.sig(g[:20]) for g in guides], dtype=np.uint64))
    assert own["nb"].tolist() == [2, 1, 2] and own["strand"].tolist()[0] == 1
    events, codes = rm.bowtie_events(model, [g[:20] for g in guides], [0, 3])
    assert events == [2] and codes.tolist() == [2, 0, 2]
    events, codes = rm.bowtie_events(model, [g[:20] for g in guides[:2]], [0, 2])
    assert events == [1] and codes.tolist() == [2, 1]
    # in pages of their own nobody names the window's strand-0 guide but itself
    events, codes = rm.bowtie_events(model, [g[:20] for g in guides], [0, 1, 2, 3])
    assert events == [1, 0, 1] and codes.tolist() == [0, 1, 0]
    rows = bt.paged_rows(model, np.array([bu.sig(g[:20]) for g in guides], dtype=np.uint64), [0, 3])
    assert rows["code"].tolist() == [2, 0, 2] and rows["source"].tolist()[a] == 2


def test_normaliser_drops_only_what_it_names():
    text = (">>> 2026-01-02 03:04:05:000006:\tAnalysing files...\n\n>>> 2026-01-02 03:04:05:000007:\tBatchinator is writing to: /tmp/x\n\n"
            ">>> 2026-01-02 03:04:05:000008:\t| Calling: ('RNAfold --noPS',)\n\n>>> 2026-01-02 03:04:05:000009:\t| Finished\n\n"
            "Could not find: ACGTACGTACGTACGTACGT\n>>> 2026-01-02 03:04:05:000010:\tThis batch ran in 01 00:00:01 (dd hh:mm:ss) or 1.5 seconds\n\n"
            ">>> 2026-01-02 03:04:05:000011:\tTotal run time (dd hh:mm:ss) or 01 00:00:02 seconds\n\n")
    assert rl.normalise(text) == [">>> Analysing files...", "", "Could not find: ACGTACGTACGTACGTACGT",
                                  ">>> This batch ran in (dd hh:mm:ss) or seconds", "", ">>> Total run time (dd hh:mm:ss) or seconds", "", ""]
    with pytest.raises(AssertionError):
        rl.same_log(text, text.replace("Analysing", "Analyzing"))
    with pytest.raises(AssertionError):
        rl.same_log(text, text + "\n")


def test_file_counts_walk():
    """Guides repeated inside a file and across files; a third occurrence is a duplicate but no new repeated guide."""
    g1, g2 = b"ACGTACGTACGTAAGCTAGCTGG", b"GATTACAGATTACAGATTACAGG"
    pad = b"ATATATATAT"
    a = b">a\n" + pad + g1 + pad + g2 + pad + g1 + b"\n"
    b = b">b\n" + pad + g1 + pad + b"\n>c\n" + pad + g2 + pad + b"\n"
    counts = rm.file_counts([a, b])
    assert counts[0][0] >= 3 and counts[0][1] >= 1 and counts[1][1] >= 2
    assert counts[1][2] >= 2 and counts[1][3] == counts[0][3]
    # the same through one dictionary over all inputs
    seen = {}
    for _, seq in __import__("guides_util").parse([a, b]):
        for _, _, guide in __import__("guides_util").matches(seq):
            seen[guide] = seen.get(guide, 0) + 1
    assert counts[1][2] == sum(v > 1 for v in seen.values()) and counts[1][3] == len(seen)
    assert sum(c[0] for c in counts) == sum(seen.values())
    assert np.all(np.diff([c[3] for c in counts]) >= 0)
