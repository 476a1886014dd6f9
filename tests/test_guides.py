"""GPU: crackling_amd.GuideSet / issl_guides_* / bin/cracklingGuides against the reference's own rows
(tests/golden/guides/) and against a brute-force pass in Python over the same records (tests/guides_util.py;
tests/test_guides_abi.py pins that brute force to the reference rows)."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
import guides_util as gu
import many_records_util as mr

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "cracklingGuides")
CASES = gu.golden_cases()
POS_PER_BLOCK = 4096  # kPosPerBlock of issl_match.hpp: text positions per workgroup of the scan

# 23-character words that match exactly once each way they are meant to, wherever they stand in a background of "AT":
# no "GG" but at the end, no "CC" but at the start
FWD = b"ACGTTGCAACGTTGCAACGTAGG"   # forward pattern only
REV = b"CCAACGTTGCAACGTTGCAACAT"   # reverse pattern only
BOTH = b"CCGTTGCAACGTTGCAACGTAGG"  # both patterns at one start
WORDS = {FWD: [0], REV: [1], BOTH: [0, 1]}


def _extract_checked(inputs, blobs):
    """Extract, and compare everything with parse() / brute_force() of the same bytes.  -> (records, expected rows)"""
    records = gu.parse(blobs)
    want = gu.brute_force(records)
    with ca.GuideSet.extract(inputs) as gs:
        gu.check_set(gs, records, want)
    return records, want


def _background(n):
    return (b"AT" * (n // 2 + 1))[:n]


def _place(length, placements):
    buf = bytearray(_background(length))
    for at, word in placements:
        buf[at:at + len(word)] = word
    return bytes(buf)


def _places(rows):
    return [(int(g["record"]), int(g["start"]), int(g["strand"])) for g in rows]


# ---- the reference's own rows -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,paths,as_dir,reference,rows", CASES, ids=[c[0] for c in CASES])
def test_golden_cases(case, paths, as_dir, reference, rows, tmp_path):
    blobs = [p.read_bytes() for p in paths]
    for p in paths:  # the case's inputs in a directory of their own
        shutil.copy(p, tmp_path / p.name)
    ways = [blobs, [str(p) for p in paths], [tmp_path]]
    if reference == "raises IndexError":
        for inputs in ways:
            with pytest.raises(ca.IsslError) as e:
                ca.GuideSet.extract(inputs)
            assert e.value.code == -3 and "line 4" in e.value.message
        return
    records = gu.parse(blobs)
    want = gu.brute_force(records)
    for inputs in ways:
        with ca.GuideSet.extract(inputs) as gs:
            gu.check_set(gs, records, want)
            got = np.zeros(len(gs), dtype=gu.ROW_DTYPE)
            got["guide23"] = [s.encode() for s in gs.strings()]
            for f in ("record", "start", "strand", "seen"):
                got[f] = gs.guides[f]
            assert gu.reference_rows([(n, None) for n, _ in gs.records], got) == rows
            if not rows:
                assert gs.n_guides == 0 and gs.n_matches == 0 and gs.sigs_tensor().numel() == 0
                assert gs.score(None)[0].size == 0  # nothing to score: the index is not touched


# ---- the edges of the grid ----------------------------------------------------------------------------------------------

def test_the_construction_words():
    for word, strands in WORDS.items():
        for flank in (b"", b"ATATATATATATATATATATATAT"):
            got = gu.matches(flank + word + flank)
            assert sorted((p, s) for p, s, _ in got) == [(len(flank), s) for s in strands]
    assert gu.matches(_background(500)) == []


@pytest.mark.parametrize("word", list(WORDS), ids=["fwd", "rev", "both"])
def test_block_boundary_of_the_grid(word):
    for at in range(POS_PER_BLOCK - 23, POS_PER_BLOCK + 2):
        seq = _place(2 * POS_PER_BLOCK + 700, [(at, word), (2 * POS_PER_BLOCK + 100, FWD)])
        _, want = _extract_checked([b">r\n" + seq + b"\n"], [b">r\n" + seq + b"\n"])
        far = (0, 2 * POS_PER_BLOCK + 100, 0)  # FWD once more, two workgroups on: another guide, or the same seen twice
        assert _places(want) == ([(0, at, 0)] if word == FWD else sorted([(0, at, s) for s in WORDS[word]] + [far], key=lambda t: (t[2], t[1])))
        assert want["seen"].tolist() == ([2] if word == FWD else [1] * len(want))


def test_the_end_of_the_text():
    for length in (23, 24, 60, POS_PER_BLOCK, POS_PER_BLOCK + 22, POS_PER_BLOCK + 23):
        for word in WORDS:
            fits = _place(length, [(length - 23, word)])       # the last 23 characters of the text
            short = fits[:-1]                                     # 22 of them: no match
            fasta = b">r\n" + fits + b"\n"
            _, want = _extract_checked([fasta], [fasta])
            assert sorted(_places(want)) == [(0, length - 23, s) for s in WORDS[word]]
            _, want = _extract_checked([b">r\n" + short], [b">r\n" + short])
            assert len(want) == 0


def test_short_texts_and_a_record_of_exactly_23():
    for fasta in (b">a\nACGT\n", b"ACGTACGTACGTACGTACGTGG", b">a\n>b\n>c", b">only a header"):
        records, want = _extract_checked([fasta], [fasta])
        assert len(want) == 0 and len(records) >= 1
    with ca.GuideSet.extract([b""]) as gs:  # nothing at all: no record, no guide
        assert gs.records == [] and len(gs) == 0 and len(gs.guides) == 0 and gs.strings() == []
    for word in WORDS:
        _, want = _extract_checked([b">w\n" + word], [b">w\n" + word])
        assert _places(want) == [(0, 0, s) for s in WORDS[word]]
    with ca.GuideSet.extract([b">w\n" + BOTH]) as gs:
        assert gs.strings() == [BOTH.decode(), BOTH.decode()[::-1].translate(str.maketrans("ACGT", "TGCA"))]


def test_record_ends_and_separators():
    a = _place(60, [(60 - 23, FWD)])   # ends on the last character of record 0
    b = _place(60, [(0, REV)])         # starts on the first of record 1
    # a match that would span the separator if the records were glued: first 12 characters end c1, last 11 start c2
    c1, c2 = _place(40, [(28, BOTH[:12])]), _place(40, [(0, BOTH[12:])])
    assert len(gu.matches(c1 + c2)) == 2
    fasta = b">a\n" + a + b"\n>b\n" + b + b"\n>c1\n" + c1 + b"\n>c2\n" + c2 + b"\n"
    _, want = _extract_checked([fasta], [fasta])
    assert _places(want) == [(0, 37, 0), (1, 0, 1)]
    # wrapped lines are joined: the same coordinates
    wrapped = b">a\n" + a[:30] + b"\n" + a[30:] + b"\r\n>b\n" + b[:7] + b"\r\n" + b[7:] + b"\n"
    _, want = _extract_checked([wrapped], [wrapped])
    assert _places(want) == [(0, 37, 0), (1, 0, 1)]


def test_forward_before_reverse_and_first_seen_across_records():
    rc = lambda s: s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))  # noqa: E731
    # record 0: a reverse match at 5, then FWD at 40 -- the forward one is met first; record 1: FWD again (seen 2), and
    # the reverse complement of REV's guide as a forward word: the same guide as record 0's reverse match
    r0 = _place(80, [(5, REV), (40, FWD)])
    r1 = _place(90, [(10, FWD), (50, rc(REV))])
    fasta = b">r0\n" + r0 + b"\n>r1\n" + r1 + b"\n"
    _, want = _extract_checked([fasta], [fasta])
    assert _places(want) == [(0, 40, 0), (0, 5, 1)] and want["seen"].tolist() == [2, 2]
    assert want["guide23"].tolist() == [FWD, rc(REV)]


def test_more_records_than_the_start_table_in_lds():
    rnd = np.random.default_rng(4300)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts = []
    for r in range(4300):  # k_guide_finish keeps up to 4096 starts in LDS; most workgroups of the scan span ~100 records
        seq = acgt[rnd.integers(0, 4, size=int(rnd.integers(0, 60)))].tobytes()
        parts.append(b">r%d\n" % r + (seq + b"\n" if seq else b""))
    fasta = b"".join(parts)
    records, want = _extract_checked([fasta], [fasta])
    assert len(records) == 4300 and len(want) > 2000 and int(want["record"].max()) > 4200
    k = mr.switch()  # and at the switch itself: k records are the largest table of the LDS fill loop, k + 1 the first in global memory
    assert k < 4300
    for n_records in (k, k + 1):
        fasta, planted = mr.fasta(n_records)
        records, want = _extract_checked([fasta], [fasta])
        assert len(records) == n_records and len(want) > 2000 and int(want["record"].max()) == n_records - 1
        ends = want[want["record"] == n_records - 1]
        assert {planted["first"].encode(), planted["last"].encode()} <= set(ends["guide23"].tolist())
        assert {0, len(records[-1][1]) - 23} <= set(ends["start"].tolist())


# ---- a random genome ------------------------------------------------------------------------------------------------------

def _genome(seed=20261017, total=300_000, n_records=12):
    rnd = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = acgt[rnd.integers(0, 4, size=total)].copy()
    for at in rnd.integers(0, total - 400, size=40):       # soft-masked stretches
        s[at:at + 400] |= 0x20
    for at in rnd.integers(0, total - 200, size=30):       # N stretches
        s[at:at + int(rnd.integers(1, 200))] = ord("N")
    unit = np.frombuffer(b"GATTACAGATTACAGATTACCGG", dtype=np.uint8)
    s[100_000:100_000 + 23 * 1001] = np.tile(unit, 1001)  # every 23-mer of the tiling 1000 times or more
    twice, thrice = acgt[rnd.integers(0, 4, size=21)].tobytes() + b"GG", b"CC" + acgt[rnd.integers(0, 4, size=21)].tobytes()
    for word, places in ((twice, (5_000, 250_000)), (thrice, (30_000, 170_000, 290_000))):
        for at in places:
            s[at:at + 23] = np.frombuffer(word, dtype=np.uint8)
    cuts = [0] + sorted(rnd.choice(np.arange(1000, total - 1000), size=n_records - 1, replace=False).tolist()) + [total]
    recs = []
    for r in range(n_records):
        seq = s[cuts[r]:cuts[r + 1]].tobytes()
        width = int(rnd.integers(50, 90))
        recs.append(b">chr%d seed %d\n" % (r, seed) + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)))
    return recs


@pytest.fixture(scope="module")
def genome():
    recs = _genome()
    records = gu.parse([b"".join(recs)])
    return recs, records, gu.brute_force(records)


def test_random_genome(genome):
    recs, records, want = genome
    assert len(records) == 12 and sum(len(s) for _, s in records) == 300_000
    seen = set(want["seen"].tolist())
    assert {1, 2, 3} <= seen and max(seen) >= 1000 and len(want) > 30_000
    fasta = b"".join(recs)
    with ca.GuideSet.extract([fasta]) as gs, ca.GuideSet.extract([fasta]) as again:
        gu.check_set(gs, records, want)
        assert gs.guides.tobytes() == again.guides.tobytes()  # deterministic: the same bytes on every run
        assert gs.sigs_tensor().cpu().numpy().tobytes() == again.sigs_tensor().cpu().numpy().tobytes()
        sigs = gs.sigs_tensor()
        assert sigs.is_cuda and sigs.dtype.is_floating_point is False and sigs.numel() == len(want)
        assert np.array_equal(sigs.cpu().numpy().view(np.uint64), gs.guides["guide23"] & np.uint64((1 << 40) - 1))
        assert np.array_equal(sigs.cpu().numpy().view(np.uint64), ca.encode_guides([s[:20] for s in gs.strings()]))
        assert np.array_equal(gs.guides_tensor().cpu().numpy().view(np.uint8).reshape(-1), gs.guides.view(np.uint8))
        # three files: the same records under indexes that run on over the files
        files = [b"".join(recs[:5]), b"".join(recs[5:6]), b"".join(recs[6:])]
        assert gu.parse(files) == records
        with ca.GuideSet.extract(files) as split:
            gu.check_set(split, records, want)
            assert split.guides.tobytes() == gs.guides.tobytes()


def test_a_record_name_shared_across_files(genome):
    recs = genome[0]
    # chr1 comes again in the second file, in mid-file: skipped there; as the last record of the third file: kept
    files = [b"".join(recs[:3]), recs[3] + recs[1] + recs[4], recs[5] + recs[1]]
    records = gu.parse(files)
    assert [n[:4] for n, _ in records] == [b"chr0", b"chr1", b"chr2", b"chr3", b"chr4", b"chr5", b"chr1"]
    _extract_checked(files, files)


# ---- hand-off to the scorer -----------------------------------------------------------------------------------------------

def test_score_without_leaving_the_device(genome, golden_uniform):
    fasta = b"".join(genome[0][:2]) + [c for c in CASES if c[0] == "multi"][0][1][0].read_bytes()
    ix = ca.IsslIndex.open(golden_uniform.issl).upload(0)
    try:
        with ca.GuideSet.extract([fasta]) as gs:
            strings, seen = gs.strings(), gs.guides["seen"]
            assert (seen > 1).any() and len(strings) > 1000
            idx, mit, cfd = gs.score(ix)
            assert np.array_equal(idx, np.flatnonzero(seen == 1))
            want_mit, want_cfd = ix.score([strings[i][:20] for i in idx], 4, 75.0, "and")
            assert np.array_equal(mit.view(np.uint64), want_mit.view(np.uint64))
            assert np.array_equal(cfd.view(np.uint64), want_cfd.view(np.uint64))
            idx, mit, cfd = gs.score(ix, max_dist=3, threshold=0.0, method="mit", only_unique=False)
            assert np.array_equal(idx, np.arange(len(strings)))
            want_mit, want_cfd = ix.score([s[:20] for s in strings], 3, 0.0, "mit")
            assert np.array_equal(mit.view(np.uint64), want_mit.view(np.uint64))
            assert np.array_equal(cfd.view(np.uint64), want_cfd.view(np.uint64))
    finally:
        ix.close()


# ---- bin/cracklingGuides ----------------------------------------------------------------------------------------------------

def _text(rows):
    return "".join("\t".join(r) + "\n" for r in rows).encode()


@pytest.mark.parametrize("case", ["multi", "dir3"])
def test_cli_prints_the_reference_rows(case, tmp_path):
    _, paths, as_dir, _, rows = [c for c in CASES if c[0] == case][0]
    args = [str(paths[0].parent)] if as_dir else [str(p) for p in paths]
    r = subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, ISSL_GUIDES_TIMING="1"))
    assert r.returncode == 0 and r.stdout == _text(rows)
    line = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("[issl guides]")]
    assert len(line) == 1 and all(f" {st} " in line[0] for st in ("parse", "upload", "count", "emit", "sort", "runs", "order", "finish"))
    assert f"guides {len(rows)} unique {sum(x[5] == '1' for x in rows)}" in line[0]
    r = subprocess.run([EXE, "--unique"] + args, capture_output=True)
    assert r.returncode == 0 and r.stdout == _text([x for x in rows if x[5] == "1"]) and r.stderr == b""
    if as_dir:  # the files named one by one are read in the order given
        r = subprocess.run([EXE] + [str(p) for p in sorted(paths)], capture_output=True)
        assert r.returncode == 0 and r.stdout != _text(rows) and len(r.stdout.splitlines()) > 10


def test_cli_errors(tmp_path):
    blank = [c for c in CASES if c[0] == "blankline"][0][1][0]
    for args in ([str(tmp_path / "missing.fa")], [str(blank)], ["--unique", str(blank)]):
        r = subprocess.run([EXE] + args, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr
    assert b"line 4" in r.stderr and str(blank).encode() in r.stderr
