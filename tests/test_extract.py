"""Off-target site extraction: oracle vs the golden vectors of the reference Python (CPU), GPU
implementation vs goldens and oracle (GPU)."""
import ctypes as C
import json
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "extract"
SETS = ["multi", "repeat"]
# input shapes run through the reference script (oracle/make_golden_extract_cases.py): per case the inputs, whether they
# are given as a list or as a directory, and the reference's line count or the exception it raised
CASES = json.loads((GOLD / "cases" / "cases.json").read_text())
REF_CASES = [c["case"] for c in CASES if "lines" in c]
REJECTED_CASES = [c["case"] for c in CASES if "raises" in c]


def case_inputs(name, tmp_path=None):
    """(blobs the reference read, sites.txt or None, command-line arguments when tmp_path is given).  A directory case
    is copied to a directory of its own; its dot-file is there and is not among the blobs."""
    case = next(c for c in CASES if c["case"] == name)
    d = GOLD / "cases" / name
    seen = [f for f in case["inputs"] if not (case["as"] == "dir" and f.startswith("."))]
    blobs = [(d / f).read_bytes() for f in seen]
    want = (d / "sites.txt").read_bytes() if "lines" in case else None
    args = None
    if tmp_path is not None:
        args = [str(d / f) for f in seen]
        if case["as"] == "dir":
            g = tmp_path / f"{name}_dir"
            g.mkdir()
            for f in case["inputs"]:
                shutil.copy(d / f, g / f)
            args = [str(g)]
    return blobs, want, args


def oracle_extract(blobs):
    so = ROOT / "oracle" / "_build" / "libextract_oracle.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(ROOT / "oracle"), "all"], check=True, capture_output=True)
    lib = C.CDLL(str(so))
    lib.oracle_extract.restype = C.c_void_p
    lib.oracle_extract.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_size_t)]
    lib.oracle_extract_free.argtypes = [C.c_void_p]
    files = (C.c_char_p * len(blobs))(*blobs)
    lens = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    n = C.c_size_t()
    p = lib.oracle_extract(files, lens, len(blobs), C.byref(n))
    out = C.string_at(p, n.value)
    lib.oracle_extract_free(p)
    return out


def random_fasta(seed, n_records, max_len, p_n=0.003, lower=0.2, width=70):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n_records):
        n = int(rng.integers(0, max_len))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        s[rng.random(n) < p_n] = ord("N")
        m = rng.random(n) < lower
        s[m] = s[m] + 32  # lower case
        seq = s.tobytes().decode()
        out.append(f">rec{r} something\n")
        out += [seq[i:i + width] + "\n" for i in range(0, len(seq), width)]
    return "".join(out).encode()


@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_reference_python_golden(name):
    got = oracle_extract([(GOLD / f"{name}.fa").read_bytes()])
    assert got == (GOLD / f"{name}.sites.txt").read_bytes()


@pytest.mark.parametrize("name", REF_CASES)
def test_oracle_matches_reference_python_on_input_shapes(name):
    """One input: the reference's explode rules; several: its per-file rules (repeated headers, leading blanks)."""
    blobs, want, _ = case_inputs(name)
    case = next(c for c in CASES if c["case"] == name)
    assert want.count(b"\n") == case["lines"] > 100
    assert oracle_extract(blobs) == want


@pytest.mark.parametrize("name", REJECTED_CASES)
def test_oracle_on_inputs_the_reference_rejects(name):
    """A blank line (IndexError) or sequence before the first header (AttributeError) in a single input: the reference
    raises, the project carries on; the oracle's output is pinned by its line count."""
    blobs, want, _ = case_inputs(name)
    case = next(c for c in CASES if c["case"] == name)
    assert want is None and len(blobs) == 1 and case["raises"] in ("IndexError", "AttributeError")
    got = oracle_extract(blobs)
    assert got.count(b"\n") == case["oracle_lines"] > 100 and len(got) == 21 * case["oracle_lines"]


def test_input_shape_cases_cover_both_modes():
    assert len(REF_CASES) >= 30 and sorted(REJECTED_CASES) == ["blank_lines_single", "sequence_before_first_header_single"]
    n_inputs = {c["case"]: len([f for f in c["inputs"] if not (c["as"] == "dir" and f.startswith("."))]) for c in CASES}
    assert sum(n == 1 for n in n_inputs.values()) >= 10 and sum(n > 1 for n in n_inputs.values()) >= 15
    assert n_inputs["directory_with_one_file"] == 1 and n_inputs["directory_with_dot_file"] == 2


def test_oracle_known_sites():
    # one forward site (N20 + NGG) and its text; one reverse-pattern match (first 20 chars reverse-complemented)
    out = oracle_extract([b">a\nACGTACGTACGTACGTACGTAGG\n>b\nCCAACGTACGTACGTACGTACGTT\n"]).decode().split()
    assert "ACGTACGTACGTACGTACGT" in out
    rc = str.maketrans("ACGT", "TGCA")
    assert "CCAACGTACGTACGTACGTA".translate(rc)[::-1] in out
    # a T in the first position is not a forward site (pattern starts with [ACG])
    assert oracle_extract([b">a\nTCGTACGTACGTACGTACGTAGG\n"]) == b""


def test_extraction_without_device_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import crackling_amd as ca
    with pytest.raises(ca.IsslError) as e:
        ca.extract_offtargets([(GOLD / "multi.fa").read_bytes()])
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)
    r = subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(tmp_path / "o.txt"), str(GOLD / "multi.fa")],
                       capture_output=True)
    assert r.returncode == 1 and b"no HIP device" in r.stderr and not (tmp_path / "o.txt").exists()
    r = subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(tmp_path / "o.txt")], capture_output=True)
    assert r.returncode == 2 and b"usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gpu_extraction_matches_reference_golden(name):
    import crackling_amd as ca
    got = ca.extract_offtargets([(GOLD / f"{name}.fa").read_bytes()])
    assert got == (GOLD / f"{name}.sites.txt").read_bytes()


@pytest.mark.gpu
def test_gpu_extraction_matches_oracle_on_random_genomes(tmp_path):
    import crackling_amd as ca
    for seed, recs, mx in [(1, 5, 20000), (2, 1, 300000), (3, 40, 3000), (4, 3, 30)]:
        blob = random_fasta(seed, recs, mx)
        assert ca.extract_offtargets([blob]) == oracle_extract([blob]), seed
    blobs = [random_fasta(10 + i, 3, 50000) for i in range(3)]
    want = oracle_extract(blobs)
    assert ca.extract_offtargets(blobs) == want
    lines = want.split(b"\n")[:-1]
    assert lines == sorted(lines) and len(lines) > 1000
    # executable: output file + the builder consumes it
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / f"g{i}.fa"; p.write_bytes(b); paths.append(str(p))
    out = tmp_path / "sites.txt"
    r = subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(out)] + paths + ["--threads", "4"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert out.read_bytes() == want
    r = subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(tmp_path / "o2.txt"), str(tmp_path / "g0.fa")], capture_output=True)
    assert r.returncode == 0 and (tmp_path / "o2.txt").read_bytes() == oracle_extract([blobs[0]])
    issl = tmp_path / "x.issl"
    subprocess.run([str(ROOT / "bin" / "isslCreateIndex"), str(out), "20", "8", str(issl)], check=True, capture_output=True)
    ix = ca.IsslIndex.open(issl)
    assert ix.header["n_lines"] == len(lines) and ix.header["n_sites"] == len(set(lines))
    ix.close()


@pytest.mark.gpu
def test_gpu_extraction_of_inputs_parsed_in_several_pieces():
    """Inputs above 4 MB are parsed by several host threads, cut at line starts and joined with the sequential rule for
    record separators: wrapped and unwrapped records, CRLF line ends, blank lines, padded lines, many short records (so
    that pieces start with headers) -- same bytes as the oracle's single pass.  Given as two inputs, the same bytes go
    by the per-file rules: the second input's CRLF records rec0..rec2 give way to the LF records of the same names
    behind them, and the padded lines keep their leading blanks (2 523 509 lines, against 2 523 816 by the single-file
    rules)."""
    import crackling_amd as ca
    rng = np.random.default_rng(77)
    parts = [random_fasta(21, 6, 1_500_000, width=60)]                        # ~4.5 MB, wrapped
    one = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=5_000_000)].tobytes()
    parts.append(b">unwrapped one line\n" + one + b"\n")                    # a 5 MB line
    parts.append(random_fasta(22, 4000, 1200, width=50).replace(b"\n", b"\r\n"))  # CRLF, thousands of headers
    parts.append(b"\n\n  >padded header\n   acgtacgtacgtacgtacgtagg   \n\n>x\n" + random_fasta(23, 3, 900_000))
    blob = b"".join(parts)
    assert len(blob) > 12_000_000
    want = oracle_extract([blob])
    assert ca.extract_offtargets([blob]) == want
    assert ca.extract_offtargets([blob[:6_000_000], blob[6_000_000:]]) == oracle_extract([blob[:6_000_000], blob[6_000_000:]])
    assert want.count(b"\n") > 1_000_000


@pytest.mark.gpu
def test_gpu_extraction_empty_and_tiny_inputs():
    import crackling_amd as ca
    assert ca.extract_offtargets([b""]) == b""
    assert ca.extract_offtargets([b">x\nACGT\n"]) == b""
    assert ca.extract_offtargets([b">x\nACGTACGTACGTACGTACGTAGG"]) == b"ACGTACGTACGTACGTACGT\n"


# ---- inputs the reference script read: fixtures per input shape ------------------------------------------------------

def run_cli(out, args):
    r = subprocess.run([str(ROOT / "bin" / "extractOfftargets"), str(out)] + args, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return out.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", REF_CASES)
def test_gpu_extraction_matches_reference_on_input_shapes(name, tmp_path):
    """In memory, paths on the command line, and a directory holding the same files (the reference expands a lone
    directory argument to its non-hidden entries, extractOfftargets.py:201-207): the reference's own sites.txt."""
    import crackling_amd as ca
    blobs, want, args = case_inputs(name, tmp_path)
    assert ca.extract_offtargets(blobs) == want
    assert run_cli(tmp_path / "as_given.txt", args) == want
    case = next(c for c in CASES if c["case"] == name)
    d = GOLD / "cases" / name
    if case["as"] == "dir":
        other = [str(d / f) for f in case["inputs"] if not f.startswith(".")]
    else:
        g = tmp_path / "as_dir"
        g.mkdir()
        for f in case["inputs"]:
            shutil.copy(d / f, g / f)
        (g / ".skipped.fa").write_bytes(b">x\nGATTACAGATTACAGATTACCGG\n")
        other = [str(g)]
    assert run_cli(tmp_path / "other_form.txt", other) == want


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJECTED_CASES)
def test_gpu_extraction_of_inputs_the_reference_rejects(name, tmp_path):
    import crackling_amd as ca
    blobs, _, args = case_inputs(name, tmp_path)
    want = oracle_extract(blobs)
    assert ca.extract_offtargets(blobs) == want
    assert run_cli(tmp_path / "o.txt", args) == want


def repeated_header_inputs():
    """Three inputs above 4 MB each, so each is parsed in pieces, with header lines that come again in a later piece of
    the same file (LF and CRLF copies, which text mode makes equal), in another file (both stand), and as the last line
    of a file without a line end (another key)."""
    rng = np.random.default_rng(4242)

    def body(n, width, nl):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()
        return nl.join(s[i:i + width] for i in range(0, len(s), width)) + nl

    many = []                                    # ~2500 records of ~2 kb under 400 names
    for _ in range(2500):
        nl = "\r\n" if rng.random() < 0.3 else "\n"
        many.append(f">chr{int(rng.integers(0, 400))} shared{nl}" + body(int(rng.integers(500, 3500)), 70, nl))
    few = [f">big{nl}" + body(1_500_000, 60, nl) for nl in ("\n", "\r\n", "\n")]   # the same header in three pieces
    few.append(">chr7 shared\n" + body(200_000, 60, "\n") + ">big")                   # ... and at the end, unterminated
    mixed = [body(100_000, 80, "\n")]                                                # no header at first
    for k in range(1500):
        lead = "  " if k % 50 == 0 else ""
        mixed.append(f"{lead}>rec{k % 300}\n" + lead + body(int(rng.integers(1000, 5000)), 50, "\n"))
    blobs = ["".join(many).encode(), "".join(few).encode(), "".join(mixed).encode()]
    assert all(len(b) > 4_200_000 for b in blobs) and sum(map(len, blobs)) > 12_000_000
    return blobs


@pytest.mark.gpu
def test_gpu_extraction_of_repeated_headers_across_pieces(tmp_path):
    import crackling_amd as ca
    blobs = repeated_header_inputs()
    want = oracle_extract(blobs)
    n = want.count(b"\n")
    # superseded records are gone: far fewer sites than the same bytes give when every record stands
    assert 300_000 < n < oracle_extract([b"".join(blobs)]).count(b"\n") - 500_000
    assert ca.extract_offtargets(blobs) == want
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / f"g{i}.fa"; p.write_bytes(b); paths.append(str(p))
    assert run_cli(tmp_path / "o.txt", paths) == want
    ix = ca.IsslIndex.build_from_fasta(paths)
    ix.write(tmp_path / "got.issl")
    ix.close()
    ref = ca.IsslIndex.build_from_text(want)
    ref.write(tmp_path / "want.issl")
    ref.close()
    assert (tmp_path / "got.issl").read_bytes() == (tmp_path / "want.issl").read_bytes()


# ---- kernel edges: inputs whose key multiset is known by construction ------------------------------------------------
# A 23-character record whose first base is A or G and which ends in AGG holds exactly one forward site (its first 20
# characters) and no reverse one.  The parsed text is the records joined by '\n', with one more '\n' at the end.

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_SHIFTS = (np.arange(19, -1, -1) * 2).astype(np.uint64)
W = 4096   # text positions per k_match_* workgroup, keys per radix workgroup (256 * kSortItems) and per collapse workgroup


def mers(keys):
    """(n, 20) characters of 40-bit keys (base 0 in the two most significant bits: numeric order = text order)."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    return _ACGT[((keys[:, None] >> _SHIFTS) & np.uint64(3)).astype(np.int64)]


def key_of(text20):
    k = 0
    for ch in text20:
        k = k << 2 | b"ACGT".index(ch)
    return k


def random_keys(rng, n, distinct=False):
    """Keys whose first base is A or G."""
    if distinct:
        pool = np.unique(rng.integers(0, 1 << 40, size=2 * n + 64, dtype=np.uint64) & ~np.uint64(1 << 38))
        return rng.permutation(pool)[:n]
    return rng.integers(0, 1 << 40, size=n, dtype=np.uint64) & ~np.uint64(1 << 38)


def units(keys):
    return [m.tobytes() + b"AGG" for m in mers(keys)]


def fasta_of(records):
    return b"".join(b">r\n" + r + b"\n" for r in records)


def text_of(keys):
    m = mers(np.sort(np.asarray(keys, dtype=np.uint64)))
    return np.concatenate([m, np.full((len(m), 1), 10, dtype=np.uint8)], axis=1).tobytes()


def runs(rng, counts):
    """Shuffled keys in which the j-th smallest distinct key comes counts[j] times."""
    k = np.sort(random_keys(rng, len(counts), distinct=True))
    return rng.permutation(np.repeat(k, counts))


def _site_at(o):
    def make(rng):
        before = random_keys(rng, (o - 2) // 24)
        at, after = random_keys(rng, 1), random_keys(rng, 3)
        recs = units(before) + [b"N" * (o - 24 * len(before) - 1)] + units(at) + units(after)
        parsed = b"\n".join(recs) + b"\n"
        assert parsed.find(recs[len(before) + 1]) == o or len(set(recs)) < len(recs)
        return recs, np.concatenate([before, at, after])
    return make


def _text_length(n_units, total):
    def make(rng):
        keys = random_keys(rng, n_units + 1)
        recs = units(keys[:-1]) + [b"N" * (total - 24 * n_units - 24 - 1)] + units(keys[-1:])
        assert sum(len(r) + 1 for r in recs) == total
        return recs, keys
    return make


def _poly(base):
    def make(rng):
        keys = random_keys(rng, 40)
        n = 3 * W
        return units(keys[:20]) + [base * n] + units(keys[20:]), np.concatenate([keys, np.full(n - 22, key_of(b"G" * 20), dtype=np.uint64)])
    return make


def _both_patterns(rng):
    """C [CT] [ACGT]{19} [AG] G: the forward and the reverse pattern match at the same position."""
    n = 700
    body = _ACGT[rng.integers(0, 4, size=(n, 23))]
    body[:, 0] = ord("C")
    body[:, 1] = _ACGT[rng.integers(0, 2, size=n) * 2 + 1]
    body[:, 21] = _ACGT[rng.integers(0, 2, size=n) * 2]
    body[:, 22] = ord("G")
    fwd = [key_of(r[:20].tobytes()) for r in body]
    rev = [key_of(bytes(b"TGCA"[b"ACGT".index(c)] for c in r[:20].tobytes()[::-1])) for r in body]
    pad = random_keys(rng, 10)
    return units(pad) + [r.tobytes() for r in body], np.array(fwd + rev + list(pad), dtype=np.uint64)


def _of_keys(make_keys):
    def make(rng):
        keys = np.asarray(make_keys(rng), dtype=np.uint64)
        return units(keys), keys
    return make


_FIXED = key_of(b"GATTACAGATTACAGATTAC")
EDGES = {f"site_at_{o}": _site_at(o) for k in (1, 2) for o in range(W * k - 23, W * k + 2)}
EDGES.update({
    # matching
    "text_of_22": lambda rng: ([b"A" * 18 + b"AGG"], np.empty(0, dtype=np.uint64)),
    "text_of_23": lambda rng: ([b"GATTACAGATTACAGATTAGG"[:19] + b"AGG"], np.empty(0, dtype=np.uint64)),
    "text_of_24": lambda rng: (units([_FIXED]), np.array([_FIXED], dtype=np.uint64)),
    "text_of_two_blocks": _text_length(100, 2 * W),
    "text_of_three_blocks": _text_length(300, 3 * W),
    "poly_g": _poly(b"G"),
    "poly_c": _poly(b"C"),
    "both_patterns": _both_patterns,
    # sort: key counts around one and two radix workgroups, byte patterns, input order
    **{f"n_{n}": _of_keys(lambda rng, n=n: random_keys(rng, n)) for n in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W)},
    "all_equal_5000": _of_keys(lambda rng: np.full(5000, _FIXED)),
    "all_equal_8192": _of_keys(lambda rng: np.full(2 * W, _FIXED)),
    "all_equal_8193": _of_keys(lambda rng: np.full(2 * W + 1, _FIXED)),
    "top_byte_only": _of_keys(lambda rng: (random_keys(rng, 6000) & np.uint64(0xFF << 32)) | np.uint64(_FIXED & 0xFFFFFFFF)),
    "bottom_byte_only": _of_keys(lambda rng: np.uint64(_FIXED & ~0xFF) | (random_keys(rng, 6000) & np.uint64(0xFF))),
    "sorted_input": _of_keys(lambda rng: np.sort(random_keys(rng, 9000))),
    "reverse_sorted_input": _of_keys(lambda rng: np.sort(random_keys(rng, 9000))[::-1]),
    # collapse: where runs of equal keys lie in the sorted array
    "all_distinct_8192": _of_keys(lambda rng: random_keys(rng, 2 * W, distinct=True)),
    "run_across_block_edge": _of_keys(lambda rng: runs(rng, [1] * (W - 1) + [2] + [1] * 100)),
    "run_across_two_block_edges": _of_keys(lambda rng: runs(rng, [1] * (W - 1) + [2] + [1] * (W - 3) + [3] + [1] * 10)),
    "runs_of_1_2_3": _of_keys(lambda rng: runs(rng, [1, 2, 3] * 1500)),
    "runs_of_257": _of_keys(lambda rng: runs(rng, [1] * 10 + [257] + [1] * 3 + [257] * 3 + [1] * 50)),
    "run_over_whole_blocks": _of_keys(lambda rng: runs(rng, [1] * 100 + [5, 2 * W + 900, 7] + [1] * 30)),
    "heads_at_lanes_63_64": _of_keys(lambda rng: runs(rng, [63, 1, 64, 128, 63 + 256, 1, 64, 1])),
})


def edge_case(name):
    """(FASTA bytes, the site text its keys give, the keys)."""
    import zlib
    recs, keys = EDGES[name](np.random.default_rng(zlib.crc32(name.encode())))
    keys = np.asarray(keys, dtype=np.uint64)
    return fasta_of(recs), text_of(keys), keys


def test_edge_cases_have_the_shape_they_claim():
    for name, heads in (("run_across_block_edge", {W - 1}), ("heads_at_lanes_63_64", {0, 63, 64, 128, 256, 575, 576, 640})):
        k = np.sort(edge_case(name)[2])
        got = set(np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]])).tolist())
        assert heads <= got, name
        if name == "run_across_block_edge":
            assert k[W - 1] == k[W] and k[W - 2] != k[W - 1] and k[W] != k[W + 1]
    k = np.sort(edge_case("run_over_whole_blocks")[2])
    assert k[W - 1] == k[W] == k[2 * W] == k[2 * W + 1] and k[0] != k[W]
    assert len(edge_case("n_4095")[2]) == W - 1 and len(edge_case("n_8193")[2]) == 2 * W + 1
    assert len(np.unique(edge_case("top_byte_only")[2] >> np.uint64(32))) > 100
    assert len(np.unique(edge_case("bottom_byte_only")[2])) == 256
    assert len(edge_case("poly_g")[2]) == 3 * W - 22 + 40


@pytest.mark.parametrize("name", list(EDGES))
def test_oracle_gives_the_constructed_sites(name):
    blob, want, keys = edge_case(name)
    assert want.count(b"\n") == len(keys)
    assert oracle_extract([blob]) == want


def index_tables(data):
    """(signatures in id order, occurrence counts in id order) of an .issl image; the counts from slice 0's entries
    (occ << 32 | id)."""
    h = np.frombuffer(data[:48], dtype=np.uint64)
    n_sites = int(h[0])
    off = 48 + 16 * int(h[5])
    sigs = np.frombuffer(data[off:off + 8 * n_sites], dtype=np.uint64)
    off += 8 * n_sites + 8 * int(h[4] << h[3])
    ent = np.frombuffer(data[off:off + 8 * n_sites], dtype=np.uint64)
    occ = np.zeros(n_sites, dtype=np.uint64)
    occ[(ent & np.uint64(0xFFFFFFFF)).astype(np.int64)] = ent >> np.uint64(32)
    return sigs, occ


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGES))
def test_gpu_extraction_and_collapse_at_kernel_edges(name, tmp_path):
    import crackling_amd as ca
    blob, want, keys = edge_case(name)
    assert ca.extract_offtargets([blob]) == want
    if len(keys) == 0:
        with pytest.raises(ca.IsslError) as e:
            ca.IsslIndex.build_from_fasta([blob])
        assert (e.value.code, e.value.message) == (-1, "site list is empty")
        return
    ix = ca.IsslIndex.build_from_fasta([blob])
    ix.write(tmp_path / "got.issl")
    hd = ix.header
    ix.close()
    uniq, counts = np.unique(keys, return_counts=True)
    assert (hd["n_lines"], hd["n_sites"]) == (len(keys), len(uniq))
    data = (tmp_path / "got.issl").read_bytes()
    sigs, occ = index_tables(data)
    # the signature holds base p in bits 2p, 2p + 1 (isslCreateIndex.cpp:39-47)
    want_sigs = np.zeros(len(uniq), dtype=np.uint64)
    for p in range(20):
        want_sigs |= ((uniq >> np.uint64(2 * (19 - p))) & np.uint64(3)) << np.uint64(2 * p)
    assert np.array_equal(sigs, want_sigs)
    assert np.array_equal(occ, counts.astype(np.uint64))
    ref = ca.IsslIndex.build_from_text(want)
    ref.write(tmp_path / "want.issl")
    ref.close()
    assert data == (tmp_path / "want.issl").read_bytes()
