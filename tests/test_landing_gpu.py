"""GPU: off-target landings (IsslIndex.landings / landing_profile, issl_offtarget_landings*) against the numpy join of
tests/landing_util.py -- the records of IsslIndex.offtargets, the brute force over the FASTA and the transcript model.  Every
comparison is exact."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import landing_util as mu
import locate_util as lu
import transcripts_util as tu

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = str(ROOT / "bin" / "isslLandOfftargets")


def _same(a, b, fields):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in fields)


class Case:
    """An index, a genome and an annotation on the device with the model's view of them."""

    def __init__(self, index_fasta, gff=None, genome_fasta=None):
        genome_fasta = index_fasta if genome_fasta is None else genome_fasta
        self.fasta, self.gff = genome_fasta, gff
        self.ix = ca.IsslIndex.build_from_fasta([index_fasta])
        self.genome = ca.Genome.open([genome_fasta])
        self.ann = ca.Annotation.open(gff) if gff is not None else None
        self.records = lu.parse([genome_fasta])
        self.truth = lu.brute_force(self.records)
        self.hits = mu.location_hits(self.records, self.truth, tu.Model(gff)) if gff is not None else None

    def model(self, guides, max_dist, annotated=True):
        """-> (offsets, rows, profile) of the model, from this index's own record list."""
        guides = np.asarray(guides, dtype=np.uint64)
        offs, recs = self.ix.offtargets(guides, max_dist=max_dist)
        offsets, rows, cnt = mu.join(len(guides), offs, recs, self.truth, self.hits if annotated else None)
        return offsets, rows, mu.profile(len(guides), recs, cnt, rows)

    def check(self, guides, max_dist, annotated=True):
        """landings and landing_profile against the model, byte for byte.  -> (offsets, rows, profile)"""
        guides = np.asarray(guides, dtype=np.uint64)
        ann = self.ann if annotated else None
        want_off, want, want_prof = self.model(guides, max_dist, annotated)
        offsets, rows = self.ix.landings(guides, self.genome, ann, max_dist=max_dist)
        assert offsets.dtype == np.uint64 and rows.dtype == ca.LANDING_DTYPE
        assert np.array_equal(offsets, want_off)
        assert len(rows) == len(want) and rows.tobytes() == want.tobytes()
        prof = self.ix.landing_profile(guides, self.genome, ann, max_dist=max_dist)
        assert prof.tobytes() == want_prof.tobytes()
        return offsets, rows, prof

    def close(self):
        if self.ann is not None:
            self.ann.close()
        self.genome.close()
        self.ix.close()


@pytest.fixture(scope="module")
def repeat():
    fasta, records, truth, gff, hits, guides = mu.repeat_case()
    case = Case(fasta, gff)
    assert np.array_equal(case.truth, truth)
    yield case, guides
    case.close()


def _runs_gff():
    """One exon whose bounds are two pos + 1 values inside the 70 000-copy run (copies 1000 .. 50 000 of it start inside), a
    second gene over copies 40 000 .. 45 000 (status 2 there), and a transcript without an mRNA line on run1 (status 3)."""
    s6 = mu.run_starts()[6]
    at = lambda copy: s6 + 23 * copy + 1
    return b"".join([
        tu.gff_line("run0", "mRNA", 1, 10, "ID=t1;Parent=g1"), tu.gff_line("run0", "exon", at(1000), at(50_000), "ID=e1;Parent=t1"),
        tu.gff_line("run0", "mRNA", 1, 10, "ID=t2;Parent=g2"), tu.gff_line("run0", "exon", at(40_000), at(45_000), "ID=e2;Parent=t2"),
        tu.gff_line("run1", "exon", 1, 10_000_000, "ID=e3;Parent=orphan"),
    ])


@pytest.fixture(scope="module")
def runs():
    fasta, words = mu.runs_genome()
    case = Case(fasta, _runs_gff())
    yield case, ca.encode_guides([w[:20] for w in words])
    case.close()


def test_repeat_genome(repeat):
    case, guides = repeat
    offsets, rows, prof = case.check(guides, 4)
    assert set(rows["hits"]["status"].tolist()) == {0, 2, 3}
    assert np.any(rows["hits"]["hit"] > 0) and np.any(rows["hits"]["hit"] == 0)
    assert int(prof["in_exon"].sum()) == int((rows["hits"]["hit"] > 0).sum()) > 0
    sites, occurrences = case.ix.offtarget_profile(guides, max_dist=4)
    assert np.array_equal(prof["located"], occurrences) and not prof["absent"].any() and not prof["pad"].any()
    assert np.all(np.diff(offsets.astype(np.int64)) == occurrences.sum(axis=1))
    # without the annotation: untested rows, nothing in an exon
    _, bare, bare_prof = case.check(guides, 4, annotated=False)
    assert np.all(bare["hits"]["status"] == 1) and np.all(bare["hits"]["first"] == 0xFFFFFFFF) and not bare["hits"]["hit"].any()
    assert not bare_prof["in_exon"].any() and np.array_equal(bare_prof["located"], occurrences)
    assert not rows["pad"].any()


def test_runs_genome(runs):
    """Runs of 1, 63, 64, 65, 4096, 4097 and 70 000 copies.  At max_dist 0 a guide owns its own run: the profile's lane, wave
    and workgroup walks each side of their switches.  At max_dist 2 every guide owns all seven: one record whose landings
    span hundreds of workgroups of the join, under seven guides."""
    case, guides = runs
    counts = mu.RUN_COUNTS
    offsets, rows, prof = case.check(guides, 0)
    assert np.diff(offsets.astype(np.int64)).tolist() == counts and prof["located"][:, 0].tolist() == counts
    assert prof["in_exon"][:, 0].tolist() == [0, 63, 0, 0, 4096, 0, 49_001]  # run1 holds runs 1 and 4; copies 1000 .. 50 000 of run 6
    offsets, rows, prof = case.check(guides, 2)
    assert np.diff(offsets.astype(np.int64)).tolist() == [sum(counts)] * 7
    assert prof["located"].sum(axis=1).tolist() == [sum(counts)] * 7 and prof["in_exon"].sum(axis=1).tolist() == [63 + 4096 + 49_001] * 7
    mine = rows[(rows["guide"] == 3) & (rows["site"] == guides[6])]
    assert len(mine) == 70_000 and np.array_equal(np.diff(mine["pos"].astype(np.int64)), np.full(69_999, 23))
    assert int((mine["hits"]["hit"] > 0).sum()) == 49_001 and int((mine["hits"]["status"] == 2).sum()) == 5_001
    assert int((rows["hits"]["status"] == 3).sum()) == 7 * (63 + 4096)


def test_shapes(runs):
    case, guides = runs
    ix, genome, ann = case.ix, case.genome, case.ann
    offsets, rows = ix.landings(np.zeros(0, dtype=np.uint64), genome, ann)        # n = 0
    assert offsets.tolist() == [0] and len(rows) == 0
    assert len(ix.landing_profile(np.zeros(0, dtype=np.uint64), genome, ann)) == 0
    nobody = ca.encode_guides(["GATTACAGATTACAGATTAC"])                           # a guide without an off-target
    offsets, rows, prof = case.check(nobody, 0)
    assert offsets.tolist() == [0, 0] and len(rows) == 0 and not prof["located"].any() and not prof["absent"].any()
    offsets, rows, _ = case.check(guides[[2, 1, 2]], 0)                            # a guide listed twice
    assert offsets.tolist() == [0, 64, 127, 191]
    assert _same(rows[:64], rows[127:], ("site", "pos", "record", "strand", "rank", "hits"))
    assert rows["guide"].tolist() == [0] * 64 + [1] * 63 + [2] * 64
    for total, pick in ((0, nobody), (1, guides[[0]]), (255, guides[[1, 2, 2, 2]]), (256, guides[[1, 2, 2, 3]]), (257, guides[[2, 2, 2, 3]])):
        offsets, rows, _ = case.check(np.concatenate([nobody, pick, nobody]) if total else pick, 0)
        assert len(rows) == total == int(offsets[-1])


def test_offtargets_that_do_not_occur_in_this_genome():
    """The index from the whole runs FASTA, the genome without its record run1 (runs 1 and 4): empty off-targets first, last
    and side by side, inside a guide and across guides."""
    whole, words = mu.runs_genome()
    part, _ = mu.runs_genome(skip={1})
    case = Case(whole, _runs_gff(), genome_fasta=part)
    try:
        guides = ca.encode_guides([w[:20] for w in words])
        assert [n for n, _ in case.genome.records] == [b"run0", b"run2"]
        order = guides[[1, 0, 1, 4, 2, 4]]                                        # at max_dist 0 a guide is one off-target
        offsets, rows, prof = case.check(order, 0)
        assert np.diff(offsets.astype(np.int64)).tolist() == [0, 1, 0, 0, 64, 0]
        assert prof["absent"][:, 0].tolist() == [1, 0, 1, 1, 0, 1] and prof["located"][:, 0].tolist() == [0, 1, 0, 0, 64, 0]
        offsets, rows, prof = case.check(guides, 2)                               # every guide: five runs present, two absent
        sites, occurrences = case.ix.offtarget_profile(guides, max_dist=2)
        assert prof["absent"].sum(axis=1).tolist() == [2] * 7 and np.all(prof["located"].sum(axis=1) == occurrences.sum(axis=1) - 63 - 4096)
        assert not np.isin(rows["site"], guides[[1, 4]]).any() and set(rows["record"].tolist()) == {0, 1}
        assert np.all(rows["hits"]["hit"][rows["record"] == 1] == 0)               # run2 is not annotated
    finally:
        case.close()


def test_record_names():
    """Text ahead of the first header (a record with an empty name), a header with leading blanks, a dotted name -- which
    never matches the annotation's `_`."""
    fasta, words = mu.runs_genome(counts=[5, 6, 7], names=(b"", b" lead x", b"dot.ted"))
    fasta = fasta[len(b">\n"):]
    gff = b"".join([tu.gff_line("", "mRNA", 1, 10, "ID=a;Parent=ga"), tu.gff_line("", "exon", 1, 60, "ID=ea;Parent=a"),
                    tu.gff_line("lead", "mRNA", 1, 10, "ID=b;Parent=gb"), tu.gff_line("lead", "exon", 1, 60, "ID=eb;Parent=b"),
                    tu.gff_line("dot.ted", "mRNA", 1, 10, "ID=c;Parent=gc"), tu.gff_line("dot.ted", "exon", 1, 60, "ID=ec;Parent=c")])
    case = Case(fasta, gff)
    try:
        assert [n for n, _ in case.genome.records] == [b"", b" lead x", b"dot.ted"] == [n for n, _ in case.records]
        assert case.ann.seqs == [b"", b"lead", b"dot_ted"]
        guides = ca.encode_guides([w[:20] for w in words])
        offsets, rows, prof = case.check(guides, 0)
        assert np.diff(offsets.astype(np.int64)).tolist() == [5, 6, 7]
        assert [int((rows["hits"]["hit"][rows["record"] == r] > 0).sum()) for r in range(3)] == [2, 2, 0]  # pos + 1 = 18, 41 <= 60
    finally:
        case.close()


@pytest.mark.parametrize("beyond", [0, 1])
def test_many_records(beyond):
    """The join keeps the table of record starts in LDS up to kLdsRecords records and reads it from global memory above:
    the largest genome of the one path and the smallest of the other, landings in their last records."""
    import many_records_util as mr
    n = mr.switch() + beyond
    fasta, planted = mr.fasta(n)
    gff = b"".join(tu.gff_line("r%d" % r, "mRNA", 1, 10, "ID=t%d;Parent=g%d" % (r, r)) + tu.gff_line("r%d" % r, "exon", 1, 30, "ID=e%d;Parent=t%d" % (r, r))
                   for r in (3, 6, n - 7, n - 6, n - 2, n - 1))
    case = Case(fasta, gff)
    try:
        assert len(case.genome.records) == n
        sites = np.unique(case.truth["site"])
        late = case.truth["site"][case.truth["record"] >= n - 7]
        guides = np.concatenate([sites[np.linspace(0, len(sites) - 1, 56).astype(np.int64)], late[np.linspace(0, len(late) - 1, 8).astype(np.int64)]])
        offsets, rows, prof = case.check(guides, 1)
        assert int(rows["record"].max()) == n - 1 and np.any(rows["hits"]["hit"][rows["record"] >= n - 7] > 0)
    finally:
        case.close()


def test_capacity_determinism_and_device_entries(repeat):
    import torch
    case, guides = repeat
    lib = _lib.lib
    guides = np.ascontiguousarray(guides[:12])
    want_off, want, want_prof = case.model(guides, 3)
    total = len(want)
    assert total > 12
    h = (case.ix._h, case.genome._h, case.ann._h)
    # one row short: nothing is written, offsets and total are complete
    buf = np.full(64 * total, 0xAB, dtype=np.uint8)
    offs = np.zeros(len(guides) + 1, dtype=np.uint64)
    n = C.c_size_t()
    _lib.check(lib.issl_offtarget_landings(*h, guides.ctypes.data, len(guides), 3, offs.ctypes.data, buf.ctypes.data, total - 1, C.byref(n)))
    assert n.value == total and np.array_equal(offs, want_off) and np.all(buf == 0xAB)
    _lib.check(lib.issl_offtarget_landings(*h, guides.ctypes.data, len(guides), 3, offs.ctypes.data, buf.ctypes.data, total, C.byref(n)))
    assert n.value == total and buf.tobytes() == want.tobytes()
    # two calls, equal bytes
    again_off, again = case.ix.landings(guides, case.genome, case.ann, max_dist=3)
    assert again.tobytes() == want.tobytes() and again_off.tobytes() == want_off.tobytes()
    # the device entries, on a side stream, a guard row behind the last one
    stream = torch.cuda.Stream()
    d_guides = torch.from_numpy(guides.view(np.int64)).cuda()
    d_offs = torch.zeros(len(guides) + 1, dtype=torch.int64, device="cuda")
    assert case.ix.landings_device(d_guides, case.genome, d_offs, None, case.ann, max_dist=3, stream=stream.cuda_stream) == total
    assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
    d_rows = torch.full((64 * (total - 1),), 0xAB, dtype=torch.uint8, device="cuda")
    d_offs.zero_()
    assert case.ix.landings_device(d_guides, case.genome, d_offs, d_rows, case.ann, max_dist=3, stream=stream.cuda_stream) == total
    assert bool((d_rows == 0xAB).all()) and d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
    d_rows = torch.full((64 * (total + 1),), 0xAB, dtype=torch.uint8, device="cuda")
    assert case.ix.landings_device(d_guides, case.genome, d_offs, d_rows, case.ann, max_dist=3, stream=stream.cuda_stream) == total
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy()
    assert got[:64 * total].tobytes() == want.tobytes() and np.all(got[64 * total:] == 0xAB)
    d_prof = torch.full((144 * (len(guides) + 1),), 0xAB, dtype=torch.uint8, device="cuda")
    case.ix.landing_profile_device(d_guides, case.genome, d_prof, case.ann, max_dist=3, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    got = d_prof.cpu().numpy()
    assert got[:144 * len(guides)].tobytes() == want_prof.tobytes() and np.all(got[144 * len(guides):] == 0xAB)
    # ... without an annotation too
    bare_off, bare, bare_prof = case.model(guides, 3, annotated=False)
    assert case.ix.landings_device(d_guides, case.genome, d_offs, d_rows, None, max_dist=3, stream=stream.cuda_stream) == total
    torch.cuda.synchronize()
    assert d_rows.cpu().numpy()[:64 * total].tobytes() == bare.tobytes()
    # outputs that are too small are refused, as Annotation.hits_device refuses them
    with pytest.raises(ValueError):
        case.ix.landings_device(d_guides, case.genome, d_offs[:-1], None, case.ann, max_dist=3)
    with pytest.raises(ValueError):
        case.ix.landing_profile_device(d_guides, case.genome, d_prof[:144 * len(guides) - 1], case.ann, max_dist=3)


def test_pieces(repeat):
    """More than 2^22 records (the scan runs in pieces) from more than 2^15 guides (the host call cuts the batch): the rows'
    (guide, rank, record, pos, strand) and the offsets against IsslIndex.offtargets + Genome.locate."""
    case, guides = repeat
    offs32, recs32 = case.ix.offtargets(guides, max_dist=2)
    copies = ((1 << 22) + len(recs32)) // len(recs32)
    copies = max(copies, ((1 << 15) + 32) // 32)
    many = np.tile(guides, copies)
    offs, recs = case.ix.offtargets(many, max_dist=2)
    assert len(recs) > (1 << 22) and len(many) > (1 << 15)
    loc_off, locs = case.genome.locate(recs["site"])
    cnt = np.diff(loc_off.astype(np.int64))
    offsets, rows = case.ix.landings(many, case.genome, case.ann, max_dist=2)
    assert np.array_equal(offsets, loc_off[offs.astype(np.int64)])
    assert len(rows) == len(locs)
    rank = np.arange(len(recs), dtype=np.int64) - offs.astype(np.int64)[recs["guide"]]
    assert np.array_equal(rows["guide"], np.repeat(recs["guide"], cnt)) and np.array_equal(rows["rank"], np.repeat(rank, cnt).astype(np.uint32))
    for f in ("record", "pos", "strand"):
        assert np.array_equal(rows[f], locs[f]), f
    # every copy of the 32 guides has the first copy's rows, and those are the model's
    first = int(offsets[32])
    want_off, want, want_prof = case.model(guides, 2)
    assert rows[:first].tobytes() == want.tobytes()
    assert _same(rows[-first:], want, ("site", "pos", "record", "strand", "rank", "id", "occ", "dist", "slice", "pad", "hits"))
    prof = case.ix.landing_profile(many, case.genome, case.ann, max_dist=2)
    assert prof.tobytes() == np.tile(want_prof, copies).tobytes()
    # the device entries take the guides as one batch: its records are scanned in two pieces, counted first and scanned
    # again to write, and the guide whose records straddle the cut gets its profile from both
    import torch
    d_guides = torch.from_numpy(many.view(np.int64)).cuda()
    d_offs = torch.zeros(len(many) + 1, dtype=torch.int64, device="cuda")
    d_rows = torch.full((64 * (len(rows) + 1),), 0xAB, dtype=torch.uint8, device="cuda")
    assert case.ix.landings_device(d_guides, case.genome, d_offs, d_rows, case.ann, max_dist=2) == len(rows)
    torch.cuda.synchronize()
    assert d_offs.cpu().numpy().view(np.uint64).tobytes() == offsets.tobytes()
    got = d_rows.cpu().numpy()
    assert got[:64 * len(rows)].tobytes() == rows.tobytes() and np.all(got[64 * len(rows):] == 0xAB)
    del d_rows, got
    d_prof = torch.empty(144 * len(many), dtype=torch.uint8, device="cuda")
    case.ix.landing_profile_device(d_guides, case.genome, d_prof, case.ann, max_dist=2)
    torch.cuda.synchronize()
    assert d_prof.cpu().numpy().tobytes() == prof.tobytes()


def test_executable(repeat, tmp_path):
    case, guides = repeat
    guides = guides[[0, 9, 17, 25, 0]]
    fa, gff, issl, q = tmp_path / "g.fa", tmp_path / "genes.gff3", tmp_path / "g.issl", tmp_path / "q.txt"
    fa.write_bytes(case.fasta)
    gff.write_bytes(case.gff)
    case.ix.write(issl)
    q.write_bytes(b"".join(t + b"\n" for t in lu.sig_text(guides)))
    for annotated in (True, False):
        _, rows, prof = case.model(guides, 3, annotated)
        opt = ["--annotation", str(gff)] if annotated else []
        r = subprocess.run([EXE] + opt + [str(issl), str(q), "3", str(fa)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == mu.records_text(guides, rows, case.records, annotated)
        r = subprocess.run([EXE, "--profile"] + opt + [str(issl), str(q), "3", str(fa)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == mu.profile_text(guides, prof, 3)


def test_handles_on_different_devices(repeat):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    case, guides = repeat
    with ca.Genome.open([case.fasta], device=1) as other:
        with pytest.raises(ca.IsslError) as e:
            case.ix.landings(guides[:2], other, None)
        assert e.value.code == -1 and "device 0" in e.value.message and "device 1" in e.value.message
        with pytest.raises(ca.IsslError):
            case.ix.landing_profile(guides[:2], other, case.ann)
