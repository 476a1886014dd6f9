"""CPU: the brute force of tests/bulge_util.py -- the expected rows of every bulge test -- pinned to a second oracle written
differently (explicit alignment strings per (b, i), compared character by character) and to rows written out by hand."""
import numpy as np
import pytest

import bulge_util as bu
import search_util as su

NGG9 = "NNNNNNNGG"  # a 6-base guide and NGG: small enough to align by hand


def random_text(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def explicit_oracle(records, pattern, queries, span, max_dist, max_dna, max_rna):
    """For every window, strand, b and break point: the query and the site as two rows of an alignment, '-' where a base has
    no partner, the pattern written under the query.  -> {(query, record, pos, strand, b): (dist, at, site, mism)}"""
    g0, G = span
    L = len(pattern)
    found = {}
    for rec, (_, seq) in enumerate(records):
        seq = seq.decode()
        for b in range(-max_rna, max_dna + 1):
            W = L + b
            for pos in range(len(seq) - W + 1):
                w = seq[pos:pos + W]
                if set(w) - set("ACGT"):
                    continue
                for strand, t in ((0, w), (1, su.revcomp(w))):
                    for k, query in enumerate(queries):
                        best = None
                        for i in ([0] if b == 0 else range(1, G) if b > 0 else range(1, G + b)):
                            cut = g0 + i
                            if b >= 0:  # the site has b bases more: gaps in the query (and in the pattern)
                                top = [(j, query[j], pattern[j]) for j in range(cut)] + [(None, "-", "N")] * b + \
                                      [(j, query[j], pattern[j]) for j in range(cut, L)]
                                bottom = list(t)
                            else:       # the query has -b bases more: gaps in the site
                                top = [(j, query[j], pattern[j]) for j in range(L)]
                                bottom = list(t[:cut]) + ["-"] * -b + list(t[cut:])
                            assert len(top) == len(bottom)
                            admitted, dist, mism = True, 0, 0
                            for (j, qc, pc), sc in zip(top, bottom):
                                if sc == "-":
                                    assert pc == "N"  # the rule on the span's interior
                                    continue
                                admitted = admitted and sc in su.IUPAC[pc]
                                if qc not in "-N" and qc != sc:
                                    dist += 1
                                    mism |= 1 << j
                            if admitted and dist <= max_dist and (best is None or dist < best[0]):
                                best = (dist, i, sum("ACGT".index(c) << (2 * s) for s, c in enumerate(t)), mism)
                        if best:
                            found[(k, rec, pos, strand, b)] = best
    return found


def as_dict(rows):
    return {(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["bulge"])):
            (int(r["dist"]), int(r["at"]), int(r["site"]), int(r["mism"])) for r in rows}


def check_against_oracle(records, pattern, queries, span, max_dist, D, R):
    offsets, rows, profile = bu.brute_force(records, pattern, queries, span, max_dist, D, R)
    want = explicit_oracle(records, pattern, queries, span, max_dist, D, R)
    assert as_dict(rows) == want and len(rows) == len(want)
    keys = [(int(r["query"]), int(r["record"]), int(r["pos"]), int(r["strand"]), int(r["bulge"])) for r in rows]
    assert keys == sorted(keys)  # (query, record, pos, strand, bulge as a signed number)
    assert offsets.tolist() == [sum(1 for k in keys if k[0] < q) for q in range(len(queries) + 1)]
    counted = np.zeros_like(profile)
    np.add.at(counted, (rows["query"], rows["bulge"].astype(np.int64) + R, rows["dist"]), 1)
    assert np.array_equal(counted, profile) and profile.shape == (len(queries), R + D + 1, max_dist + 1)
    return rows


def test_brute_force_equals_explicit_alignments_three_prime_pam():
    rng = np.random.default_rng(1)
    pattern, span = "N" * 10 + "NGG", (0, 10)
    guide = "ACGTTGCAAG"
    text = list(random_text(rng, 300))
    plants = {20: guide + "TGG", 50: guide[:4] + "C" + guide[4:] + "AGG", 80: guide[:6] + guide[7:] + "CGG",
              110: su.revcomp(guide[:3] + "TT" + guide[3:] + "GGG"), 140: su.revcomp(guide[:5] + guide[7:] + "TGG"),
              170: "AAAAAAAAAAAAAAGG"}
    for at, s in plants.items():
        text[at:at + len(s)] = s
    records = [(b"one", "".join(text[:200]).encode()), (b"two", "".join(text[200:]).encode() + b"NACGTTGCAAGTGG")]
    queries = [guide + "NNN", "A" * 10 + "NNN", guide[:4] + "N" + guide[5:] + "NNN", "N" * 13, random_text(rng, 10) + "NNN"]
    rows = check_against_oracle(records, pattern, queries, span, 2, 2, 2)
    assert set(rows["bulge"].tolist()) == {-2, -1, 0, 1, 2} and {0, 1} == set(rows["strand"].tolist())
    assert (rows["dist"][rows["bulge"] != 0] > 0).any() and (rows["at"] > 1).any()


def test_brute_force_equals_explicit_alignments_five_prime_pam_and_codes_at_the_span_ends():
    rng = np.random.default_rng(2)
    text = list(random_text(rng, 260))
    guide = "GATTACAGCT"
    for at, s in {30: "TTTC" + guide, 60: "TTTA" + guide[:5] + "G" + guide[5:], 90: su.revcomp("TTTG" + guide[:2] + guide[3:])}.items():
        text[at:at + len(s)] = s
    records = [(b"r", "".join(text).encode())]
    check_against_oracle(records, "TTTV" + "N" * 10, ["NNNN" + guide, "N" * 14], (4, 10), 1, 1, 1)
    # a code at the span's first and last position, the span not at an end of the pattern
    check_against_oracle(records, "NV" + "N" * 6 + "RGN", ["NN" + guide[:8] + "N", "N" * 11], (1, 8), 2, 2, 1)
    # nothing bulges: the rows of the mismatch search, any code inside the span
    offsets, rows, _ = bu.brute_force(records, "NNRNNNNGG", ["GATTACNNN", "N" * 9], (0, 6), 2, 0, 0)
    want_off, want_rows, _ = su.brute_force(records, "NNRNNNNGG", ["GATTACNNN", "N" * 9], 2)
    assert offsets.tolist() == want_off.tolist() and len(rows) > 0 and not rows["bulge"].any() and not rows["at"].any()
    for f in ("site", "pos", "record", "query", "mism", "strand", "dist"):
        assert np.array_equal(rows[f], want_rows[f]), f


@pytest.fixture(scope="module")
def hand_case():
    """Six windows planted in random text, each aligned by hand in the comments of HAND_ROWS."""
    rng = np.random.default_rng(3)
    text = list(random_text(rng, 300))
    plants = {20: "ACGATCATGG", 60: "ACGGTCATGG", 100: "ACGCATGG", 140: su.revcomp("GATCTAGAGG")}
    for at, s in plants.items():
        text[at:at + len(s)] = s
    records = [(b"hand", "".join(text).encode())]
    queries = ["ACGTCANNN", "GATTACNNN", "ACNTCANNN"]
    return records, bu.as_tuples(bu.brute_force(records, NGG9, queries, (0, 6), 1, 1, 1)[1], 9)


HAND_ROWS = [
    # a DNA bulge: ACG-TCA against ACGATCA, the A at site position 3 has no partner.  Break point 2 pairs GTCA with ATCA
    # (1 mismatch), break point 4 pairs ACGT with ACGA (1): 3 alone gives 0
    (0, 0, 20, 0, 0, 1, 3, "ACGATCATGG", 0),
    # a tie in a homopolymer run: ACGTCA against ACGGTCA.  Break point 2 (AC|GTCA against AC.GTCA) and break point 3
    # (ACG|TCA against ACG.TCA) both give 0; break point 1 pairs CGTCA with GGTCA (1).  The smaller one is reported
    (0, 0, 60, 0, 0, 1, 2, "ACGGTCATGG", 0),
    # an RNA bulge: ACGTCA against ACGCA, the query's T at position 3 has no partner.  Break point 2 pairs TCA with GCA
    # (1), break point 4 pairs ACGT with ACGC (1)
    (0, 0, 100, 0, 0, -1, 3, "ACGCATGG", 0),
    # strand 1, a DNA bulge and a mismatch: the text holds the reverse complement of GATCTAGAGG; GAT-TAC against GATCTAG
    # differs at query position 5 (C against G).  Break point 2: TTAC against CTAG (2); break point 4: GATT against GATC
    # and AC against AG (2)
    (1, 0, 140, 1, 1, 1, 3, "GATCTAGAGG", 1 << 5),
    # N inside the span: ACNTCA against ACGATCA.  Break point 3 pairs ACN with ACG (0), break point 2 pairs NTCA with ATCA
    # (0 as well: the N is not compared); break point 1 pairs CNTCA with GATCA (1).  The smaller of the two is reported
    (2, 0, 20, 0, 0, 1, 2, "ACGATCATGG", 0),
]  # (the sixth, a 5' PAM with span (4, 20), has a text of its own below)


def test_rows_written_out_by_hand(hand_case):
    _, got = hand_case
    for row in HAND_ROWS:
        assert row in got, row
    # the window at 20 is no row at all without a bulge: its positions 7 and 8 are T G, which NGG does not admit
    assert not [r for r in got if r[2] == 20 and r[3] == 0 and r[5] == 0]


def test_a_row_written_out_by_hand_with_a_five_prime_pam_and_span_4_20():
    guide = "ACGTTGCAAGCTTGACCTGA"
    rng = np.random.default_rng(4)
    text = list(random_text(rng, 120))
    site = "TTTA" + guide[:10] + "A" + guide[10:]  # an A between the guide's G at 9 and C at 10: it equals neither
    text[40:40 + len(site)] = site
    records = [(b"cas12a", "".join(text).encode())]
    _, rows, _ = bu.brute_force(records, "TTTV" + "N" * 20, ["NNNN" + guide], (4, 20), 0, 1, 0)
    # break point 9 pairs the guide's G at 9 with the extra A, break point 11 its C at 10: 10 alone gives 0.  mism and at are
    # counted from the span's start, positions from the pattern's
    assert (0, 0, 40, 0, 0, 1, 10, site, 0) in bu.as_tuples(rows, 24)
    q, s = bu.aligned("NNNN" + guide, rows[[r[2] == 40 and r[5] == 1 for r in bu.as_tuples(rows, 24)]][0], (4, 20))
    assert (q, s) == ("NNNN" + guide[:10] + "-" + guide[10:], site)


def test_formatter_lines():
    rows = np.zeros(3, dtype=bu.BULGE_HIT_DTYPE)
    pack = lambda s: sum("ACGT".index(c) << (2 * i) for i, c in enumerate(s))
    rows[0] = (pack("ACGTACGTACTTGCAACGTACGGG"), 1234567890123, 0, 0, (1 << 0) | (1 << 10), 1, 2, 1, 10)
    rows[1] = (pack("ACGTACGTACTTGCAACGTAC"), 7, 0, 1, (1 << 2) | (1 << 5) | (1 << 22), 0, 3, -2, 3)
    rows[2] = (pack("ACGTACGTACTTGCAACGTACGG"), 0, 0, 0, 1 << 22, 0, 1, 0, 0)
    queries = ["CCGTACGTACTGCAACGTACNGG", "TTTACGTACGTACTTGCAACGTA"]
    assert bu.format_rows([(b"chr", b"")], queries, rows[:1], (0, 20)) == \
        b"CCGTACGTAC-TGCAACGTACNGG\tchr\t1234567890123\t-\t2\tD1\taCGTACGTACTtGCAACGTACGGG\n"
    assert bu.format_rows([(b"chr", b"")], queries, rows[1:2], (4, 19)) == \
        b"TTTACGTACGTACTTGCAACGTA\tchr\t7\t+\t3\tR2\tACgTAcG--TACTTGCAACGTAc\n"
    assert bu.format_rows([(b"chr", b"")], queries, rows[2:], (0, 20)) == \
        b"CCGTACGTACTGCAACGTACNGG\tchr\t0\t+\t1\t0\tACGTACGTACTTGCAACGTACGg\n"
    profile = np.arange(12, dtype=np.uint64).reshape(2, 3, 2)
    assert bu.format_profile(queries, profile) == (queries[0].encode() + b"\t0\t1\t2\t3\t4\t5\n" +
                                                   queries[1].encode() + b"\t6\t7\t8\t9\t10\t11\n")
