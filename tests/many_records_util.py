"""A seeded genome of many short records, for the one size switch of the locate and Bowtie stages: k_guide_finish,
k_locate_finish and k_occur_verdict turn a position of the resident text into (record, offset) by a binary search in the
table of record starts, which they keep in LDS up to kLdsRecords records and read from global memory above.  fasta() makes
the input, sizes() the record counts on both sides of the switch, queries() the 20-mers asked of it.  Nothing of the
library runs here: tests/test_many_records_model.py pins the brute force of locate_util and the model of bowtie_util to
this input on the CPU before tests/test_many_records_gpu.py compares the device with them."""
import pathlib
import re

import numpy as np

import bowtie_util as bu

ROOT = pathlib.Path(__file__).resolve().parent.parent
SWITCH_SOURCES = ("issl_guides.hip", "issl_locate.hip", "issl_occur.hip")
SEED = 20261019
LOW_DUP, LOW_STRANDS = 3, 6   # the records below index 10 that hold planted reads
QUERY_CAP = 60_000


def switch():
    """kLdsRecords as the three sources state it: the largest number of records whose starts the kernels keep in LDS."""
    found = []
    for name in SWITCH_SOURCES:
        text = (ROOT / "crackling_amd" / "csrc" / name).read_text()
        values = re.findall(r"constexpr uint32_t kLdsRecords = (\d+);", text)
        assert len(values) == 1, (name, values)
        found.append(int(values[0]))
    assert len(set(found)) == 1, dict(zip(SWITCH_SOURCES, found))
    return found[0]


def sizes():
    """Record counts: one below the switch, the switch itself (the largest table of the LDS fill loop), the first count
    that takes the global path, and one with thousands of records beyond it."""
    k = switch()
    return [k - 1, k, k + 1, 2 * k + 808]


def name_of(r, last):
    """Header text of record r: some with text behind a blank, which bowtieChr cuts off; the last record among them."""
    return "r%d x%d" % (r, r % 7) if r % 4 == 1 or r == last else "r%d" % r


def fasta(n_records, seed=SEED):
    """One FASTA input of n_records records of 0 to 59 random bases (most too short or barely long enough for a window of
    23; a workgroup of the text scan spans about 100 of them), a few of them overwritten.  With L the last index:
      L       a forward read (20-mer + AGG) at offset 0 and another (... TGG) that ends on the record's last base
      L-1     exactly the 23 bases CCT + 17 + AGG: a forward and a reverse occurrence in one window
      L-2     the first 22 bases of a window CC + 20 + C whose last base opens record L-1: its read must not occur
      L-3     empty: a header line only (it shares its start in the text with record L-2)
      L-5     `dup` + AGG and `dup` + TGG, and both once more in record LOW_DUP: aligned and repeated bits from records on
              both sides of the switch, the first occurrence of read 0 in the low one
      L-6     `rej` + AGG and `rej` + TGG: two guides that are unique as 23-mers, end their 20-mer on G (accepted by the G20
              rule) and are rejected by the Bowtie step (two reads align): rows a run drops ahead of scoring
    and, for more than K + 3 records (K = switch()):
      K-1, K  the read `straddle` on the last 23 bases of record K-1 and on the first 23 of record K, which ends on
              another read 0 (... AGG) of its own: a row of the Bowtie step that names record K itself
      K+1     empty
      K+2     starts with the reverse complement of the read `strands` of record LOW_STRANDS: one occurrence per strand,
              the one on strand 1 above the switch.  (For locate, whose site on strand 1 is the reverse complement of the
              window's FIRST 20 characters, the site with one location per strand is strands[3:23]: TGG follows the read
              in the low record.)
    -> (FASTA bytes, planted: the reads by name (str) and the record indices "L", "K", "n")."""
    k, last = switch(), n_records - 1
    assert n_records >= 16
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    read = lambda pam: "ACG"[rng.integers(3)] + rand(19) + pam           # noqa: E731
    # the reads and the two low records first: every size with this seed plants the same ones
    window = "CC" + rand(20) + "C"
    p = dict(first=read("AGG"), last=read("TGG"), both="CCT" + rand(17) + "AGG", past=bu.rc(window), dup=read("")[:20],
             straddle=read("AGG"), strands=read("")[:3] + read("")[:17] + "CGG", rej=read("")[:19] + "G", L=last, K=k, n=n_records)
    low_dup = rand(2) + p["dup"] + "TGG" + rand(6) + p["dup"] + "AGG" + rand(1)
    low_strands = rand(7) + p["strands"] + "TGG" + rand(6)
    seqs = [rand(int(rng.integers(0, 60))) for _ in range(n_records)]
    seqs[LOW_DUP], seqs[LOW_STRANDS] = low_dup, low_strands
    seqs[last] = p["first"] + rand(10) + p["last"]
    seqs[last - 1] = p["both"]
    seqs[last - 2] = window[:22]
    assert window[22] == p["both"][0]
    seqs[last - 3] = ""
    seqs[last - 5] = rand(5) + p["dup"] + "AGG" + rand(3) + p["dup"] + "TGG"
    seqs[last - 6] = p["rej"] + "AGG" + rand(3) + p["rej"] + "TGG"
    if n_records > k + 3:
        assert last - 6 > k + 2
        seqs[k - 1] = rand(12) + p["straddle"]
        seqs[k] = p["straddle"] + rand(8) + "AGG"
        seqs[k + 1] = ""
        seqs[k + 2] = bu.rc(p["strands"]) + rand(20)
    assert all(len(s) < 60 for s in seqs)
    text = "".join(">%s\n%s" % (name_of(r, last), s + "\n" if s else "") for r, s in enumerate(seqs))
    return text.encode(), p


def _mers(seq):
    return [seq[i:i + 20] for i in range(len(seq) - 19)]


def queries(model, planted, cap=QUERY_CAP, seed=11):
    """Packed 20-mers to ask of the genome of fasta(): every planted 20-mer and its reverse complement, twice; all 20-mers
    of the last 200 records and of records K-3 .. K+3; every 20-mer of the text whose read 0 occurs first in a record at or
    above K (what makes the rows and locations beyond the switch many, not a sample's share of them); and a seeded sample
    of bowtie_util.adversarial_queries(model) that fills the list up to `cap`.  Shuffled, behind four that stay in front so
    that a page of any length from 4 on holds them together: `dup` twice (the first copy is named by no group: code 2, the
    second is rejected: code 0) and the two guides of the CCT ... AGG window (the group of the one on strand 1 names the
    other).  -> uint64 signatures"""
    k, n = planted["K"], len(model.records)
    rng = np.random.default_rng(seed)
    mers = []
    for name in ("first", "last", "both", "past", "dup", "straddle", "strands", "rej"):
        mers += [planted[name][:20], bu.rc(planted[name])[:20], bu.rc(planted[name][:20])] * 2
    mers.append(planted["strands"][3:])  # locate's site with a location on either strand
    for r in sorted(set(range(max(0, n - 200), n)) | set(range(max(0, k - 3), min(n, k + 4)))):
        mers += _mers(model.records[r][1])
    own = np.array([bu.sig(m) for m in mers], dtype=np.uint64)
    beyond = model.keys[(model.stats["record"] != bu.NONE) & (model.stats["record"] >= k)]
    rest = bu.adversarial_queries(model, seed)
    take = max(0, cap - len(own) - len(beyond))
    if len(rest) > take:
        rest = rest[np.sort(rng.choice(len(rest), take, replace=False))]
    sigs = np.concatenate([own, beyond, rest])
    rng.shuffle(sigs)
    head = [planted["dup"], planted["dup"], planted["both"][:20], bu.rc(planted["both"])[:20]]
    return np.concatenate([np.array([bu.sig(m) for m in head], dtype=np.uint64), sigs[:cap - len(head)]])


_cases = {}


def case(n_records):
    """-> dict(blob, planted, records (bytes, as locate_util.parse), truth (locate_util.brute_force), model
    (bowtie_util.Model), queries) for one size, built once."""
    if n_records not in _cases:
        import locate_util as lu
        blob, planted = fasta(n_records)
        records = lu.parse([blob])
        model = bu.Model([blob])
        _cases[n_records] = dict(blob=blob, planted=planted, records=records, truth=lu.brute_force(records), model=model,
                                 queries=queries(model, planted))
    return _cases[n_records]
