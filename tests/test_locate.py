"""GPU: crackling_amd.Genome / issl_genome_locate* against a brute-force pass in Python over the same record text
(tests/locate_util.py; tests/test_locate_abi.py pins that brute force to the reference-made site lists)."""
import ctypes as C
import json
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import crackling_amd as ca
from crackling_amd import _lib
import locate_util as lu

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
EXTRACT = ROOT / "tests" / "golden" / "extract"
MiB = 1 << 20
ABSENT = ["AAAAAAAAAAAAAAAAAAAA", "ACACACACACACACACACAC", "TTTTTTTTTTTTTTTTTTTG", "GATTACAGATTACAGATTAC", "CCCCCCCCCCGGGGGGGGGG"]


def _locate_checked(blobs, extra_sites=(), paths=None):
    """Open, locate every distinct site of the brute force plus extra_sites, check the whole contract.  -> (truth, locs)"""
    records = lu.parse(blobs)
    truth = lu.brute_force(records)
    with ca.Genome.open(paths if paths is not None else blobs) as g:
        assert g.records == [(n, len(s)) for n, s in records]
        assert g.n_bases == sum(len(s) for _, s in records)
        sites = np.concatenate([np.unique(truth["site"]), ca.encode_guides(list(extra_sites))]).astype(np.uint64)
        offsets, locs = g.locate(sites)
        lu.check_locate(g.records, offsets, locs, sites, truth)
        assert len(locs) == len(truth) + sum(int((truth["site"] == s).sum()) for s in ca.encode_guides(list(extra_sites)))
    return truth, locs


def _fixtures():
    out = [("multi", [EXTRACT / "multi.fa"], EXTRACT / "multi.sites.txt", "list"),
           ("repeat", [EXTRACT / "repeat.fa"], EXTRACT / "repeat.sites.txt", "list")]
    for c in json.loads((EXTRACT / "cases" / "cases.json").read_text()):
        d = EXTRACT / "cases" / c["case"]
        if (d / "sites.txt").exists():
            out.append((c["case"], sorted(d / i for i in c["inputs"] if not i.startswith(".")), d / "sites.txt", c["as"]))
    return out


@pytest.mark.parametrize("name,inputs,sites_txt,how", _fixtures(), ids=[f[0] for f in _fixtures()])
def test_reference_fixtures(name, inputs, sites_txt, how, tmp_path):
    blobs = [p.read_bytes() for p in inputs]
    lines = sites_txt.read_bytes().split()
    absent = [s for s in ABSENT if s.encode() not in set(lines)]
    paths = [str(p) for p in inputs]
    if how == "dir":  # the case's inputs, the hidden one included, in a directory of their own
        for p in inputs[0].parent.iterdir():
            if p.name != "sites.txt":
                shutil.copy(p, tmp_path / p.name)
        paths = [tmp_path]
    truth, _ = _locate_checked(blobs, absent, paths=paths)
    _locate_checked(blobs, absent)  # the same from memory
    # per site, as many locations as the reference wrote lines
    want = {}
    for s in lines:
        want[s] = want.get(s, 0) + 1
    texts = lu.sig_text(truth["site"])
    got = {}
    for s in texts:
        got[s] = got.get(s, 0) + 1
    assert got == want


# ---- constructed genomes: 23-character matches at known places in a background that matches nothing -----------------

FWD = b"ACGTTGCAACGTTGCAACGTAGG"     # forward pattern only: site ACGTTGCAACGTTGCAACGT
REV = b"CCAACGTTGCAACGTTGCAACAT"     # reverse pattern only
BOTH = b"CCGTTGCAACGTTGCAACGTAGG"    # both patterns at one position


def _patterns(s):
    t = lu.brute_force([(b"", s)])
    return sorted((int(p), int(st)) for p, st in zip(t["pos"], t["strand"]))


def _background(n):
    return b"T" * n  # no G: no forward match; no C: no reverse match


def _place(length, placements):
    buf = bytearray(_background(length))
    for at, word in placements:
        buf[at:at + len(word)] = word
    return bytes(buf)


def test_the_construction_words():
    assert _patterns(FWD) == [(0, 0)]
    assert _patterns(REV) == [(0, 1)]
    assert _patterns(BOTH) == [(0, 0), (0, 1)]


def test_block_boundary_of_the_grid():
    for at in range(4095 - 22, 4096 + 2):
        for word in (FWD, REV, BOTH):
            seq = _place(9000, [(at, word)])
            truth, locs = _locate_checked([b">r\n" + seq + b"\n"])
            assert sorted(zip(locs["pos"].tolist(), locs["strand"].tolist())) == [(at + p, s) for p, s in _patterns(word)]


def test_record_ends_and_separators():
    a = _place(60, [(60 - 23, FWD)])           # ends on the last character of record 0
    b = _place(60, [(0, REV)])              # starts on the first of record 1
    # a match that would span the separator if the records were glued: first 12 characters end a, last 11 start c
    c1, c2 = _place(40, [(28, FWD[:12])]), _place(40, [(0, FWD[12:])])
    fasta = b">a\n" + a + b"\n>b\n" + b + b"\n>c1\n" + c1 + b"\n>c2\n" + c2 + b"\n"
    truth, locs = _locate_checked([fasta])
    assert [(int(l["record"]), int(l["pos"]), int(l["strand"])) for l in np.sort(locs, order=["record", "pos", "strand"])] == \
        [(0, 37, 0), (1, 0, 1)]
    # wrapped lines are joined: the same coordinates
    wrapped = b">a\n" + a[:30] + b"\n" + a[30:] + b"\n>b\n" + b[:7] + b"\r\n" + b[7:] + b"\n"
    _, locs2 = _locate_checked([wrapped])
    assert sorted(zip(locs2["record"].tolist(), locs2["pos"].tolist())) == [(0, 37), (1, 0)]


def test_both_patterns_at_one_position_and_both_strands_of_one_site():
    site20 = b"ACGTTGCAACGTTGCAACGG"
    # a reverse match whose site is site20: its first 20 matched characters are the reverse complement of the site
    fwd_word, rev_word = site20 + b"AGG", _revcomp(site20) + b"AAT"
    assert _patterns(fwd_word) == [(0, 0)] and _patterns(rev_word) == [(0, 1)]
    seq = _place(400, [(10, BOTH), (100, fwd_word), (200, rev_word)])
    truth, locs = _locate_checked([b">x\n" + seq + b"\n"])
    by = lu.expected_by_site(truth)
    at10 = sorted((int(g["strand"][k]), site) for site, g in by.items() for k in range(len(g)) if int(g["pos"][k]) == 10)
    assert [st for st, _ in at10] == [0, 1] and at10[0][1] != at10[1][1]  # two locations, same pos, two sites
    site = int(ca.encode_guides([site20])[0])  # (BOTH's reverse site as well)
    assert [(int(p), int(st)) for p, st in zip(by[site]["pos"], by[site]["strand"])] == [(10, 1), (100, 0), (200, 1)]
    assert len(locs) == 4


def test_tiny_genomes():
    for blob, n_rec in ((b">a\nACGTTGCAACGTTGCAACGTAG\n", 1), (b">only\n", 1), (b">a\n>b\n" + FWD + b"\n>c\n", 3), (b"", 0), (b"\n\n", 0)):
        with ca.Genome.open([blob]) as g:
            assert len(g.records) == n_rec
            offsets, locs = g.locate([FWD[:20].decode(), "A" * 20])
            want = 1 if FWD in blob else 0
            assert offsets.tolist() == [0, want, want] and len(locs) == want
            if want:
                assert (int(locs[0]["record"]), int(locs[0]["pos"]), int(locs[0]["strand"])) == (1, 0, 0)
                assert g.records == [(b"a", 0), (b"b", 23), (b"c", 0)]
    with ca.Genome.open([b">h1\n", b">h2\n" + FWD + b"\n", b""]) as g:  # a header-only file among others: per-file rules
        assert g.records == [(b"h1", 0), (b"h2", 23)]
        assert g.locate([FWD[:20].decode()])[1].tolist() == [(0, 1, 0)]


@pytest.fixture(scope="module")
def runs_genome():
    """One 23-mer per run length, copies back to back (so they straddle emit blocks and sort workgroups), the runs spread
    over three records.  Site k is a counter in base 4 behind a fixed head, so the expected lists are known by construction."""
    counts = [1, 63, 64, 65, 4096, 4097, 70000]
    words = []
    for k in range(len(counts)):
        tail = "".join("ACGT"[(k >> (2 * d)) & 3] for d in range(4))
        words.append(("ACGTTGCAACGTTGCA" + tail + "AGG").encode())
    recs = [b"", b"", b""]
    for k, (w, c) in enumerate(zip(words, counts)):
        recs[k % 3] += _background(17 + k) + w * c
    fasta = b"".join(b">run%d\n" % r + s + b"\n" for r, s in enumerate(recs))
    records = lu.parse([fasta])
    return fasta, records, lu.brute_force(records), words, counts


def test_runs_of_one_site(runs_genome):
    fasta, records, truth, words, counts = runs_genome
    with ca.Genome.open([fasta]) as g:
        sites = ca.encode_guides([w[:20] for w in words])
        offsets, locs = g.locate(sites)
        assert np.diff(offsets.astype(np.int64)).tolist() == counts
        lu.check_locate(g.records, offsets, locs, sites, truth)
        for k, c in enumerate(counts):  # back to back copies: positions 23 apart
            mine = locs[int(offsets[k]):int(offsets[k + 1])]
            assert np.all(mine["record"] == k % 3) and np.all(mine["strand"] == 0)
            assert np.array_equal(np.diff(mine["pos"].astype(np.int64)), np.full(c - 1, 23))
        every = np.unique(truth["site"])
        offsets, locs = g.locate(every)
        lu.check_locate(g.records, offsets, locs, every, truth)
        assert len(locs) == len(truth)


def test_query_shapes_capacity_determinism_and_device_entry(runs_genome):
    import torch
    fasta, records, truth, words, counts = runs_genome
    lib = _lib.lib
    with ca.Genome.open([fasta]) as g:
        offsets, locs = g.locate(np.zeros(0, dtype=np.uint64))                # n = 0
        assert offsets.tolist() == [0] and len(locs) == 0
        one = ca.encode_guides([words[2][:20]])
        offsets, locs = g.locate(one)                                         # n = 1
        assert offsets.tolist() == [0, 64]
        lu.check_locate(g.records, offsets, locs, one, truth)
        thrice = np.concatenate([one, ca.encode_guides([words[1][:20], "A" * 20]), one, one])
        offsets, locs3 = g.locate(thrice)                                     # a site named three times
        lu.check_locate(g.records, offsets, locs3, thrice, truth)
        assert np.diff(offsets.astype(np.int64)).tolist() == [64, 63, 0, 64, 64]
        assert locs3[0:64].tobytes() == locs3[127:191].tobytes() == locs3[191:255].tobytes() == locs.tobytes()
        # capacity: one short writes nothing, offsets and total complete
        sites = np.concatenate([thrice, ca.encode_guides([words[5][:20]])])
        want_off, want = g.locate(sites)
        total = len(want)
        assert total == 64 * 3 + 63 + 4097
        buf = np.full(total, 0xAB, dtype=np.uint8).repeat(16).view(ca.LOCATION_DTYPE)
        offs = np.zeros(len(sites) + 1, dtype=np.uint64)
        n = C.c_size_t()
        _lib.check(lib.issl_genome_locate(g._h, sites.ctypes.data, len(sites), offs.ctypes.data, buf.ctypes.data, total - 1, C.byref(n)))
        assert n.value == total and np.array_equal(offs, want_off) and np.all(buf.view(np.uint8) == 0xAB)
        _lib.check(lib.issl_genome_locate(g._h, sites.ctypes.data, len(sites), offs.ctypes.data, buf.ctypes.data, total, C.byref(n)))
        assert n.value == total and buf.tobytes() == want.tobytes()
        # determinism
        again_off, again = g.locate(sites)
        assert again.tobytes() == want.tobytes() and again_off.tobytes() == want_off.tobytes()
        # device entry point: same bytes; the capacity rule there too
        d_sites = torch.from_numpy(sites.view(np.int64)).cuda()
        d_offs = torch.zeros(len(sites) + 1, dtype=torch.int64, device="cuda")
        assert g.locate_device(d_sites, d_offs, None) == total
        assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()
        d_locs = torch.full((16 * (total - 1),), 0xAB, dtype=torch.uint8, device="cuda")
        assert g.locate_device(d_sites, d_offs, d_locs) == total
        assert bool((d_locs == 0xAB).all())
        d_locs = torch.full((16 * total,), 0xAB, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        assert g.locate_device(d_sites, d_offs, d_locs, stream=stream.cuda_stream) == total
        torch.cuda.synchronize()
        assert d_locs.cpu().numpy().tobytes() == want.tobytes()
        assert d_offs.cpu().numpy().view(np.uint64).tobytes() == want_off.tobytes()


def test_large_random_query(runs_genome):
    """300 000 random 20-mers around a known few that occur: the filter's false positives and the exact search."""
    fasta, records, truth, words, counts = runs_genome
    rng = np.random.default_rng(7)
    sites = rng.integers(0, 1 << 40, size=300_000, dtype=np.uint64)
    known = ca.encode_guides([w[:20] for w in words[:5]])
    at = np.array([0, 1, 150_000, 299_998, 299_999])
    sites[at] = known
    with ca.Genome.open([fasta]) as g:
        offsets, locs = g.locate(sites)
    present = np.isin(sites, truth["site"])
    cnt = np.diff(offsets.astype(np.int64))
    assert np.all(cnt[~present] == 0)
    by = lu.expected_by_site(truth)
    for k in np.flatnonzero(present):
        want = by[int(sites[k])]
        got = locs[int(offsets[k]):int(offsets[k + 1])]
        assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["record"], want["record"]) and \
            np.array_equal(got["strand"], want["strand"])
    assert set(at.tolist()) <= set(np.flatnonzero(present).tolist())


def test_query_cut_into_pieces(runs_genome):
    """More than 2^22 sites: the query is cut, the offsets run on across the pieces, and a site gets its list in whichever
    piece it is named."""
    fasta, records, truth, words, counts = runs_genome
    n = (1 << 22) + 1000
    rng = np.random.default_rng(8)
    sites = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    known = ca.encode_guides([w[:20] for w in words[:6]])
    at = np.array([5, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, n - 1, 77])
    sites[at] = known
    sites[n - 2] = known[0]  # named in both pieces
    with ca.Genome.open([fasta]) as g:
        offsets, locs = g.locate(sites)
    present = np.flatnonzero(np.isin(sites, truth["site"]))
    cnt = np.diff(offsets.astype(np.int64))
    assert int(cnt.sum()) == len(locs) == int(cnt[present].sum())
    by = lu.expected_by_site(truth)
    for k in present:
        want = by[int(sites[k])]
        got = locs[int(offsets[k]):int(offsets[k + 1])]
        assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["record"], want["record"])
    assert set(at.tolist()) | {n - 2} <= set(present.tolist())


def _repeat_genome(seed, mbp=1.0, records=5):
    """Seeded i.i.d. bases with interspersed copies of a few 300-bp elements, in `records` records of wrapped lines."""
    rng = np.random.default_rng(seed)
    n = int(mbp * 1e6)
    seq = rng.integers(0, 4, size=n, dtype=np.uint8)
    elems = rng.integers(0, 4, size=(8, 300), dtype=np.uint8)
    for at in rng.integers(0, n - 300, size=n // 3000):
        e = elems[rng.integers(0, 8)].copy()
        mut = rng.random(300) < 0.02
        e[mut] = rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)
        seq[at:at + 300] = e
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[seq].tobytes()
    cuts = [0] + sorted(rng.integers(1, n, size=records - 1).tolist()) + [n]
    out = []
    for r in range(records):
        rec = text[cuts[r]:cuts[r + 1]]
        out.append(b">chr%d test\n" % r + b"\n".join(rec[i:i + 70] for i in range(0, len(rec), 70)) + b"\n")
    return b"".join(out)


def _revcomp(s):
    return bytes(b"TGCA"[b"ACGT".index(x)] for x in reversed(s))


def test_end_to_end_offtargets_to_locations(tmp_path):
    fasta = _repeat_genome(21)
    records = lu.parse([fasta])
    ix = ca.IsslIndex.build_from_fasta([fasta])
    rng = np.random.default_rng(22)
    truth_sites = lu.brute_force(records)["site"]
    guides = truth_sites[rng.integers(0, len(truth_sites), size=32)]
    offs, recs = ix.offtargets(guides, max_dist=4)
    assert len(recs) >= 32  # every guide finds itself at least
    sites, first = np.unique(recs["site"], return_index=True)
    occ = recs["occ"][first]
    with ca.Genome.open([fasta]) as g:
        offsets, locs = g.locate(sites)
        assert np.array_equal(np.diff(offsets.astype(np.int64)), occ.astype(np.int64))  # as many locations as occurrences
        texts = lu.sig_text(sites)
        for k in range(len(sites)):
            for l in locs[int(offsets[k]):int(offsets[k + 1])]:
                span = records[int(l["record"])][1][int(l["pos"]):int(l["pos"]) + 20]
                assert (span if l["strand"] == 0 else _revcomp(span)) == texts[k]
        # the executable prints what Genome.locate says, for a plain sites file and for a real report
        names = [n for n, _ in g.records]

        def formatted(order):
            lines = []
            for s in order:
                k = int(np.searchsorted(sites, s))
                for l in locs[int(offsets[k]):int(offsets[k + 1])]:
                    lines.append(texts[k] + b"\t" + names[int(l["record"])] + b"\t%d\t" % int(l["pos"]) + (b"-" if l["strand"] else b"+") + b"\n")
            return b"".join(lines)

        fa = tmp_path / "g.fa"
        fa.write_bytes(fasta)
        plain = tmp_path / "sites.txt"
        order = list(sites[::-1][:200]) + [int(ca.encode_guides(["A" * 20])[0])]
        plain.write_bytes(b"".join(t + b"\n" for t in lu.sig_text(order + order[:3])))
        exe = str(ROOT / "bin" / "isslLocateOfftargets")
        r = subprocess.run([exe, str(plain), str(fa)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == formatted(order[:-1])
        issl = tmp_path / "g.issl"
        ix.write(issl)
        q = tmp_path / "q.txt"
        q.write_bytes(b"".join(t + b"\n" for t in lu.sig_text(guides[:8])))
        rep = subprocess.run([str(ROOT / "bin" / "isslReportOfftargets"), str(issl), str(q), "4"], capture_output=True, timeout=120)
        assert rep.returncode == 0 and rep.stdout, rep.stderr
        tsv = tmp_path / "report.tsv"
        tsv.write_bytes(rep.stdout)
        seen, order = set(), []
        for line in rep.stdout.splitlines():
            s = int(ca.encode_guides([line.split(b"\t")[1]])[0])
            if s not in seen:
                seen.add(s)
                order.append(s)
        r = subprocess.run([exe, "--report", str(tsv), str(fa)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == formatted(order)
    ix.close()


def test_close_returns_the_memory():
    import torch
    fasta = _repeat_genome(23, mbp=0.5)
    free = lambda: torch.cuda.mem_get_info(0)[0]
    with ca.Genome.open([b">warm\n" + FWD + b"\n"]) as g:  # what the first call leaves in the runtime is not the handle's
        g.locate([FWD[:20].decode()])
    torch.cuda.synchronize()
    before = free()
    g = ca.Genome.open([fasta])
    offsets, locs = g.locate(np.unique(lu.brute_force(lu.parse([fasta]))["site"])[:5000])
    assert len(locs) >= 5000
    g.close()
    g.close()  # idempotent
    torch.cuda.synchronize()
    assert abs(free() - before) <= 64 * MiB
