"""The fixtures of tests/test_many_records_gpu.py, checked on the CPU alone: for every size of many_records_util.sizes()
the seeded genome has what the GPU tests rely on -- records on both sides of the switch kLdsRecords, hits at record K and at
both ends of the last record, every verdict code, both strands, and, for the largest size, more than a thousand rows whose
record lies at or above the switch.  A failure here is a fixture regression, not a kernel's."""
import numpy as np
import pytest

import bowtie_util as bu
import locate_util as lu
import many_records_util as mr

K = mr.switch()
SIZES = mr.sizes()


def test_the_switch_is_the_sources():
    assert SIZES == [K - 1, K, K + 1, 2 * K + 808] and K >= 1024
    for name in mr.SWITCH_SOURCES:
        text = (mr.ROOT / "crackling_amd" / "csrc" / name).read_text()
        assert "n_records <= kLdsRecords" in text and "tab[kLds ? kLdsRecords : 1]" in text, name


@pytest.mark.parametrize("n_records", SIZES)
def test_the_genome_has_what_the_gpu_tests_compare(n_records):
    c = mr.case(n_records)
    p, records, truth, model = c["planted"], c["records"], c["truth"], c["model"]
    last = n_records - 1
    assert len(records) == n_records == len(model.records) and p["L"] == last
    assert [n for n, _ in records] == [mr.name_of(r, last).encode() for r in range(n_records)]
    assert b" " in records[last][0] and sum(b" " in n for n, _ in records[K - 8:]) > 1 and max(len(s) for _, s in records) < 60
    assert records[last - 3][1] == b"" and len(records[last - 2][1]) == 22 and records[last - 1][1] == p["both"].encode()
    # the two ends of the last record, in the brute force of locate and in the occurrences of the Bowtie model
    end = len(records[last][1]) - 23
    at_last = truth[truth["record"] == last]
    assert {(0, 0), (end, 0)} <= set(zip(at_last["pos"].tolist(), at_last["strand"].tolist()))
    assert model.occ[p["first"]] == [(last, 0, 0)] and model.occ[p["last"]] == [(last, end, 0)]
    assert int(truth["record"].max()) == last
    # the read of 22 bases that the next record's first base would complete
    glued = (records[last - 2][1] + records[last - 1][1]).decode()
    assert bu.rc(p["past"]) == glued[:23] and p["past"] not in model.occ
    assert bu.sig(p["past"][:20]) not in set(truth["site"].tolist())
    # one window, two occurrences
    both = model.occ[p["both"]]
    assert both == [(last - 1, 0, 0)] and model.occ[bu.rc(p["both"])[:20] + "AGG"] == [(last - 1, 0, 1)]
    # aligned and repeated bits from two records, the first occurrence in the low one
    assert model.occ[p["dup"] + "AGG"] == [(mr.LOW_DUP, 31, 0), (last - 5, 5, 0)]
    assert [r for r, _, _ in model.occ[p["dup"] + "TGG"]] == [mr.LOW_DUP, last - 5]
    dup = model.counts([bu.sig(p["dup"])])[0]
    assert (dup["nb"], dup["aligned"], dup["repeated"], dup["record"], dup["pos"], dup["n_perfect"]) == (4, 9, 9, mr.LOW_DUP, 31, 4)
    rej = model.counts([bu.sig(p["rej"])])[0]
    assert (rej["nb"], rej["aligned"], rej["repeated"], rej["record"], rej["pos"]) == (2, 9, 0, last - 6, 0) and p["rej"][19] == "G"
    if n_records > K:
        assert last >= K and (truth["record"] == K).any()
    if n_records > K + 3:
        size = len(records[K - 1][1])
        assert model.occ[p["straddle"]] == [(K - 1, size - 23, 0), (K, 0, 0)] and records[K + 1][1] == b""
        assert model.occ[p["strands"]] == [(mr.LOW_STRANDS, 7, 0), (K + 2, 0, 1)]
        by = lu.expected_by_site(truth)[bu.sig(p["strands"][3:])]
        assert (by["record"].tolist(), by["pos"].tolist(), by["strand"].tolist()) == ([mr.LOW_STRANDS, K + 2], [10, 0], [0, 1])
    # the queries: every code and both strands under both page lengths, rows from both sides of the switch
    q = c["queries"]
    assert len(q) <= mr.QUERY_CAP and len(q) > 5000
    for page_length in (0, 7):
        rows = model.rows(q, page_length)
        placed = rows[rows["record"] != bu.NONE]
        assert {0, 1, 2} <= set(rows["code"].tolist()) and {0, 1} == set(placed["strand"].tolist())
        assert int(placed["record"].max()) == last and int(placed["record"].min()) < 10
        at = int(np.nonzero(q == np.uint64(bu.sig(p["dup"])))[0][-1]) if page_length == 0 else 1
        assert (rows["owner"][at], rows["code"][at], rows["record"][at], rows["pos"][at]) == (1, 0, mr.LOW_DUP, 31)
        if page_length:  # the four in front share a page: an unnamed copy, and a verdict filed under the other guide
            assert rows["code"][:4].tolist() == [2, 0, 1, 2] and rows["source"][:4].tolist() == [bu.NONE, 1, 3, bu.NONE]
            assert (rows["record"][2], rows["strand"][2]) == (last - 1, 1)
        if n_records > K:
            assert (placed["record"] >= K).any()
        if n_records == SIZES[-1]:
            assert int((placed["record"] >= K).sum()) > 1000 and int((placed["record"] == K).sum()) >= 1
    # locate's side of the same queries
    hit = truth[np.isin(truth["site"], q)]
    if n_records > K:
        assert (hit["record"] >= K).any()
    asked = set(zip(hit["record"].tolist(), hit["pos"].tolist(), hit["strand"].tolist()))
    assert {(last, 0, 0), (last, end, 0), (last - 1, 0, 0), (last - 1, 0, 1), (mr.LOW_STRANDS, 10, 0)} <= asked
    if n_records == SIZES[-1]:
        assert int((hit["record"] >= K).sum()) > 1000 and (hit["record"] == K).any() and (hit["record"] == last).any()
        assert {(K - 1, len(records[K - 1][1]) - 23, 0), (K, 0, 0), (K + 2, 0, 1)} <= asked


def test_the_sizes_share_their_low_records():
    """The three sizes around the switch draw the same records below 10 and plant the same reads there."""
    cases = [mr.case(n) for n in SIZES[:3]]
    assert len({tuple(c["records"][:10]) for c in cases}) == 1
    assert len({(c["planted"]["dup"], c["planted"]["strands"]) for c in cases}) == 1
