"""Genome FASTA -> uploaded index on the GPU (issl_index_build_from_fasta, bin/isslIndexFromFasta): the same .issl bytes,
scores and errors as the two-step chain extract_offtargets -> build_from_text (isslCreateIndex)."""
import os
import pathlib
import shutil
import subprocess
import threading

import numpy as np
import pytest

import crackling_amd as ca
import oracle_util as ou
from test_extract import CASES, REF_CASES, case_inputs

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "extract"
SETS = ["multi", "repeat"]
WIDTHS = [8, 4, 2]
CLI = ROOT / "bin" / "isslIndexFromFasta"
MiB = 1 << 20


def synth_fasta(seed, n_records, rec_len, p_n=0.002, lower=0.2, width=60, crlf=False, repeat=None):
    """Seeded multi-FASTA: uniform bases, lower case, runs of N, wrapped lines; `repeat` = (23-mer, copies) appends a
    record that holds the 23-mer `copies` times back to back."""
    rng = np.random.default_rng(seed)
    nl = "\r\n" if crlf else "\n"
    parts = []
    for r in range(n_records):
        n = int(rng.integers(rec_len // 2, rec_len + 1))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        starts = np.flatnonzero(rng.random(n) < p_n)
        for a in starts[:64]:
            s[a:a + int(rng.integers(1, 200))] = ord("N")
        m = rng.random(n) < lower
        s[m] += 32
        seq = s.tobytes().decode()
        parts.append(f">rec{r} seed {seed}{nl}")
        parts.append(nl.join(seq[i:i + width] for i in range(0, len(seq), width)) + nl)
    if repeat:
        unit, copies = repeat
        seq = unit * copies
        parts.append(f">repeat{nl}")
        parts.append(nl.join(seq[i:i + 4096] for i in range(0, len(seq), 4096)) + nl)
    return "".join(parts).encode()


def issl_sites(data):
    """Signatures of an .issl image, in id order."""
    h = np.frombuffer(data[:48], dtype=np.uint64)
    off = 48 + 16 * int(h[5])
    return np.frombuffer(data[off:off + 8 * int(h[0])], dtype=np.uint64).copy()


def guides_near(sigs, n, seed):
    """Sites with 0-4 substitutions at random positions."""
    rng = np.random.default_rng(seed)
    g = sigs[rng.integers(0, len(sigs), size=n)].copy()
    for _ in range(4):
        hit = rng.random(n) < 0.8
        pos = rng.integers(0, 20, size=n).astype(np.uint64) * np.uint64(2)
        delta = rng.integers(1, 4, size=n).astype(np.uint64)
        old = (g >> pos) & np.uint64(3)
        new = (old + delta) & np.uint64(3)
        g = np.where(hit, (g & ~(np.uint64(3) << pos)) | (new << pos), g)
    return g


def chain_bytes(blobs, width, tmp_path, tag="chain", text=None):
    if text is None:
        text = ca.extract_offtargets(blobs)
    ix = ca.IsslIndex.build_from_text(text, slice_width=width)
    p = tmp_path / f"{tag}_{width}.issl"
    ix.write(p)
    ix.close()
    return text, p.read_bytes()


def fasta_bytes(blobs, width, tmp_path, tag="fasta", options=None):
    ix = ca.IsslIndex.build_from_fasta(blobs, slice_width=width, options=options)
    p = tmp_path / f"{tag}_{width}.issl"
    ix.write(p)
    return ix, p


def assert_scores_match(ix, path, guides, max_dist=4):
    ref = ca.IsslIndex.open(path).upload(0)
    try:
        for method, thr in (("and", 75.0), ("mit", 0.0), ("cfd", 50.0)):
            mit, cfd = ix.score(guides, max_dist, thr, method)
            rmit, rcfd = ref.score(guides, max_dist, thr, method)
            assert np.array_equal(mit.view(np.uint64), rmit.view(np.uint64)), method
            assert np.array_equal(cfd.view(np.uint64), rcfd.view(np.uint64)), method
    finally:
        ref.close()


# ---- no GPU --------------------------------------------------------------------------------------------------------

def test_build_from_fasta_without_device_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (GOLD / "multi.fa").read_bytes()
    for inputs in ([blob], [GOLD / "multi.fa"]):
        with pytest.raises(ca.IsslError) as e:
            ca.IsslIndex.build_from_fasta(inputs)
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
    out = tmp_path / "o.issl"
    r = subprocess.run([str(CLI), str(out), "8", str(GOLD / "multi.fa")], capture_output=True)
    assert r.returncode == 1 and b"no HIP device" in r.stderr and not out.exists()
    r = subprocess.run([str(CLI), str(out), "8"], capture_output=True)
    assert r.returncode == 2 and b"usage" in r.stderr and not out.exists()
    r = subprocess.run([str(CLI), str(out), "eight", str(GOLD / "multi.fa")], capture_output=True)
    assert r.returncode == 2 and b"usage" in r.stderr and not out.exists()


@pytest.mark.parametrize("width", [0, 1, 3, 5, 6, 7, 9, 16])
def test_other_widths_are_refused_before_any_work(width, tmp_path):
    """Refused with ISSL_E_ARG before the device is looked at (so also on a box without one) and before the input is
    read (a missing file is not reported)."""
    with pytest.raises(ca.IsslError) as e:
        ca.IsslIndex.build_from_fasta([(GOLD / "multi.fa").read_bytes()], slice_width=width)
    assert e.value.code == -1 and "8, 4 or 2" in str(e.value)
    with pytest.raises(ca.IsslError) as e:
        ca.IsslIndex.build_from_fasta([tmp_path / "absent.fa"], slice_width=width)
    assert e.value.code == -1
    out = tmp_path / "o.issl"
    r = subprocess.run([str(CLI), str(out), str(width), str(GOLD / "multi.fa")], capture_output=True)
    assert r.returncode == 1 and b"8, 4 or 2" in r.stderr and not out.exists()


# ---- GPU: fixtures ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", SETS)
def test_fixture_genomes_give_the_chain_bytes(name, width, tmp_path):
    fa = GOLD / f"{name}.fa"
    sites_txt = (GOLD / f"{name}.sites.txt").read_bytes()   # the reference script's own output
    ix = ca.IsslIndex.build_from_text(sites_txt, slice_width=width)
    ix.write(tmp_path / "want.issl")
    ix.close()
    want = (tmp_path / "want.issl").read_bytes()
    if width == 8:
        assert want == ou.build_issl(sites_txt, 20, 8)
    for inputs in ([fa.read_bytes()], [fa], [str(fa)]):
        got, p = fasta_bytes(inputs, width, tmp_path)
        assert p.read_bytes() == want, inputs[0].__class__
        hd = got.header
        assert hd["n_lines"] == sites_txt.count(b"\n") and hd["slice_width"] == width
        if isinstance(inputs[0], bytes):
            sigs = issl_sites(want)
            guides = guides_near(sigs, 500, seed=width)
            assert_scores_match(got, tmp_path / "want.issl", guides)
        got.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", REF_CASES)
def test_input_shapes_give_the_index_of_the_reference_site_list(name, tmp_path):
    """One input or several, odd line ends, repeated headers, ...: the .issl of the reference script's own sites.txt
    (tests/golden/extract/cases), from blobs and from paths at every width, from the executable at width 8 (a
    directory case as the directory)."""
    blobs, sites_txt, args = case_inputs(name, tmp_path)
    case = next(c for c in CASES if c["case"] == name)
    paths = [GOLD / "cases" / name / f for f in case["inputs"] if not (case["as"] == "dir" and f.startswith("."))]
    for width in WIDTHS:
        ix = ca.IsslIndex.build_from_text(sites_txt, slice_width=width)
        ix.write(tmp_path / "want.issl")
        ix.close()
        want = (tmp_path / "want.issl").read_bytes()
        for inputs in (blobs, paths):
            got, p = fasta_bytes(inputs, width, tmp_path)
            assert got.header["n_lines"] == case["lines"]
            got.close()
            assert p.read_bytes() == want, (width, inputs[0].__class__)
        if width == 8:
            out = tmp_path / "cli.issl"
            r = subprocess.run([str(CLI), str(out), "8"] + args, capture_output=True)
            assert r.returncode == 0, r.stderr.decode()
            assert out.read_bytes() == want


@pytest.mark.gpu
def test_errors_match_the_chain(tmp_path):
    for blob in (b">a\nACGTTTTTTTTTTTTTTTTTTTTTTTNNNN\n>b\nAC\n", b"", b">only a header\n"):
        with pytest.raises(ca.IsslError) as chain:
            ca.IsslIndex.build_from_text(ca.extract_offtargets([blob]))
        with pytest.raises(ca.IsslError) as e:
            ca.IsslIndex.build_from_fasta([blob])
        assert (e.value.code, e.value.message) == (chain.value.code, chain.value.message) == (-1, "site list is empty"), blob
    # a bad device: the extraction's own error
    with pytest.raises(ca.IsslError) as want:
        ca.extract_offtargets([(GOLD / "multi.fa").read_bytes()], device=4096)
    with pytest.raises(ca.IsslError) as e:
        ca.IsslIndex.build_from_fasta([(GOLD / "multi.fa").read_bytes()], device=4096)
    assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
    with pytest.raises(ca.IsslError) as e:
        ca.IsslIndex.build_from_fasta([tmp_path / "absent.fa"])
    assert e.value.code == -2
    with pytest.raises(ca.IsslError) as e:
        ca.IsslIndex.build_from_fasta([(GOLD / "multi.fa").read_bytes()], options={"no_such_option": 1})
    assert e.value.code == -1 and "no_such_option" in str(e.value)


# ---- GPU: seeded synthetic genomes -------------------------------------------------------------------------------

REPEAT_UNIT = "GATTACAGATTACAGATTACCGG"   # N20 + NGG: one forward site per copy
REPEAT_COPIES = 200_000


@pytest.mark.gpu
def test_synthetic_genomes_give_the_chain_bytes_and_the_oracle_scores(tmp_path):
    cases = [
        ("many small records, CRLF", [synth_fasta(1, 3000, 400, crlf=True)]),
        ("two files, N runs, lower case", [synth_fasta(2, 5, 200_000, p_n=0.01), synth_fasta(3, 40, 20_000, lower=0.6)]),
        ("a 23-mer 200 000 times", [synth_fasta(4, 3, 100_000, repeat=(REPEAT_UNIT, REPEAT_COPIES))]),
        ("~50 Mbp", [synth_fasta(5, 25, 2_000_000)]),
    ]
    for what, blobs in cases:
        text = ca.extract_offtargets(blobs)
        for width in WIDTHS:
            _, want = chain_bytes(blobs, width, tmp_path, text=text)
            ix, p = fasta_bytes(blobs, width, tmp_path)
            assert p.read_bytes() == want, (what, width)
            assert ix.header["n_lines"] == text.count(b"\n")
            if width != 8:
                ix.close()
                continue
            sigs = issl_sites(want)
            guides = guides_near(sigs, 2000, seed=len(what))
            if what.startswith("a 23-mer"):
                unit = ca.encode_guides([REPEAT_UNIT[:20].encode()])
                hits = ix.dump_hits(unit, 0, 0.0, "and")
                assert len(hits) == 1 and hits[0, 5] >= REPEAT_COPIES, hits   # one site, occ >= 200 000
                guides = np.concatenate([unit, guides])
            oracle = ou.OracleIndex(p)
            mit, cfd = ix.score(guides, 4, 75.0, "and")
            omit, ocfd, ohits = oracle.score(guides, 4, 75.0, "and", want_hits=True)
            assert np.array_equal(mit.view(np.uint64), omit.view(np.uint64)), what
            assert np.array_equal(cfd.view(np.uint64), ocfd.view(np.uint64)), what
            assert np.array_equal(ix.dump_hits(guides, 4, 0.0, "and"), oracle.score(guides, 4, 0.0, "and", want_hits=True)[2]), what
            oracle.close()
            ix.close()


# ---- GPU: options ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_layout_options_keep_the_bytes(tmp_path):
    blobs = [synth_fasta(7, 8, 100_000)]
    for width in WIDTHS:
        _, want = chain_bytes(blobs, width, tmp_path)
        for opts, key in (({"keep_lists": 0}, "lists_absent"), ({"compact": 1}, "is_compact")):
            ix, p = fasta_bytes(blobs, width, tmp_path, options=opts)
            assert ix.get_option(key) == 1, (width, opts)
            assert p.read_bytes() == want, (width, opts)
            guides = guides_near(issl_sites(want), 300, seed=width)
            assert_scores_match(ix, tmp_path / f"fasta_{width}.issl", guides)
            ix.close()


@pytest.mark.gpu
def test_bad_width_leaves_hbm_as_it_was(tmp_path):
    import torch
    blob = (GOLD / "multi.fa").read_bytes()
    ca.IsslIndex.build_from_fasta([blob]).close()   # runtime and code objects loaded
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for width in (1, 5, 9):
        with pytest.raises(ca.IsslError) as e:
            ca.IsslIndex.build_from_fasta([blob], slice_width=width)
        assert e.value.code == -1
        assert torch.cuda.mem_get_info(0)[0] == before, width
    ca.IsslIndex.build_from_fasta([blob]).close()
    # (close() returns the image; 32 MiB of slack for what the runtime keeps of its own)
    assert abs(torch.cuda.mem_get_info(0)[0] - before) <= 32 * MiB


# ---- GPU: memory -------------------------------------------------------------------------------------------------

def _low_water(fn):
    """Run fn() while free HBM is sampled every 5 ms; returns (result, free before, lowest free seen)."""
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    low = [before]
    stop = threading.Event()

    def watch():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            stop.wait(0.005)
    t = threading.Thread(target=watch, daemon=True)
    t.start()
    try:
        out = fn()
    finally:
        stop.set()
        t.join()
    return out, before, low[0]


@pytest.mark.gpu
def test_memory_budget_of_a_200_mbp_genome(tmp_path):
    """Peak = max(sequence + 16 B per raw site (match and sort), 8 B per raw site + 12 B per distinct site (collapse),
    the device-sites builder's own peak + its 12 B per distinct site of inputs), with 64 MiB of slack."""
    import torch
    blob = synth_fasta(200, 67, 4_000_000, p_n=0.0)
    seq_len = len(blob)   # (the parsed sequence is shorter than the file)
    ix, before, low = _low_water(lambda: ca.IsslIndex.build_from_fasta([blob]))
    peak_fasta = before - low
    path = tmp_path / "g.issl"
    ix.write(path)
    hd = ix.header
    n_raw, n_sites = hd["n_lines"], hd["n_sites"]
    image = ix.device_bytes()
    ix.close()
    assert n_raw > 30_000_000
    # the same sites as a device table: signatures from the file, counts from slice 0's entries (occ << 32 | id)
    data = path.read_bytes()
    sigs = issl_sites(data)
    h = np.frombuffer(data[:48], dtype=np.uint64)
    off = 48 + 16 * int(h[5]) + 8 * n_sites + 8 * int(h[4] << h[3])
    ent = np.frombuffer(data[off:off + 8 * n_sites], dtype=np.uint64)
    occ = np.empty(n_sites, dtype=np.uint32)
    occ[(ent & np.uint64(0xFFFFFFFF)).astype(np.int64)] = (ent >> np.uint64(32)).astype(np.uint32)
    assert int(occ.sum(dtype=np.uint64)) == n_raw
    d_sigs = torch.from_numpy(sigs.view(np.int64)).to("cuda:0")
    d_occ = torch.from_numpy(occ.view(np.int32)).to("cuda:0")
    ix2, before2, low2 = _low_water(lambda: ca.IsslIndex.build_from_device_sites(d_sigs, d_occ, n_raw))
    peak_dev = before2 - low2
    ix2.write(tmp_path / "d.issl")
    ix2.close()
    del d_sigs, d_occ
    torch.cuda.empty_cache()
    assert (tmp_path / "d.issl").read_bytes() == data
    budget = max(seq_len + 16 * n_raw, 8 * n_raw + 12 * n_sites, peak_dev + 12 * n_sites)
    print(f"200 Mbp: {n_raw} sites, {n_sites} distinct, image {image / MiB:.0f} MiB, peak {peak_fasta / MiB:.0f} MiB, "
          f"device-sites build {peak_dev / MiB:.0f} MiB, budget {budget / MiB:.0f} MiB")
    assert peak_fasta >= image
    assert peak_fasta <= budget + 64 * MiB


# ---- GPU: executable ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_gives_the_chain_bytes_and_scorer_output(tmp_path):
    fas = [GOLD / "multi.fa", GOLD / "repeat.fa"]
    text, want = chain_bytes([p.read_bytes() for p in fas], 8, tmp_path)
    out = tmp_path / "out.issl"
    r = subprocess.run([str(CLI), str(out), "8"] + [str(p) for p in fas], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert out.read_bytes() == want
    assert str(text.count(b"\n")).encode() in r.stderr and b"5 slices" in r.stderr
    d = tmp_path / "genome"
    d.mkdir()
    for p in fas:
        shutil.copy(p, d / p.name)
    (d / ".hidden.fa").write_bytes(b">x\nGATTACAGATTACAGATTACCGG\n")
    r = subprocess.run([str(CLI), str(tmp_path / "dir.issl"), "8", str(d)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "dir.issl").read_bytes() == want
    (tmp_path / "chain.issl").write_bytes(want)
    sigs = issl_sites(want)
    guides = ca.decode_guides(guides_near(sigs, 400, seed=3))
    scorer = str(ROOT / "bin" / "isslScoreOfftargets")
    got = ca.run_scorer_binary(scorer, str(out), guides, 4, 75, "and", workdir=tmp_path)
    assert got == ca.run_scorer_binary(scorer, str(tmp_path / "chain.issl"), guides, 4, 75, "and", workdir=tmp_path)
    assert got.count("\n") == 400
    # failure: no output file left behind
    r = subprocess.run([str(CLI), str(tmp_path / "none.issl"), "8", str(tmp_path / "absent.fa")], capture_output=True)
    assert r.returncode == 1 and b"absent.fa" in r.stderr and not (tmp_path / "none.issl").exists()
