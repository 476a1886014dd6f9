"""CPU: the C ABI of a run in batches (include/issl_hip.h): issl_genome_occurrences_paged[_device],
issl_consensus_selection_pages, issl_results_build_rows and ISSL_RESULTS_NO_HEADER are declared, exported and bound, and
the argument errors that need no device are answered before one is asked for."""
import ctypes as C
import inspect
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "issl_hip.h").read_text()
SYMBOLS = ["issl_genome_occurrences_paged", "issl_genome_occurrences_paged_device", "issl_consensus_selection_pages",
           "issl_results_build_rows"]


def test_four_names_and_the_flag_are_declared_exported_and_bound():
    import crackling_amd as ca
    from crackling_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert f"int {name}(" in HEADER and hasattr(lib, name) and name in _lib.EXPORTS, name
    assert "ISSL_RESULTS_NO_HEADER = 4" in HEADER and ca.results.NO_HEADER == 4
    assert "ISSL_RESULTS_DIRECT = 1" in HEADER and "#define ISSL_ABI_VERSION 6" in HEADER  # additions only
    flat = " ".join(HEADER.split())
    assert re.search(r"issl_genome_occurrences_paged\(issl_genome \*g, const uint64_t \*sites, size_t n, const uint64_t \*page_starts, "
                     r"size_t n_pages, issl_occurrence \*rows\);", flat)
    assert re.search(r"issl_genome_occurrences_paged_device\(issl_genome \*g, const uint64_t \*d_sites, size_t n, "
                     r"const uint64_t \*d_page_starts, size_t n_pages, issl_occurrence \*d_rows, void \*stream\);", flat)
    assert re.search(r"issl_consensus_selection_pages\(issl_consensus \*c, uint64_t batch_size, uint64_t page_length, "
                     r"const uint64_t \*\*d_page_starts, uint64_t \*n_pages\);", flat)
    assert re.search(r"size_t n_scored, uint64_t first_row, uint64_t n_rows, const issl_results_config \*cfg, issl_results \*\*out\);", flat)


def test_the_python_interface():
    import crackling_amd as ca
    sig = inspect.signature
    assert list(sig(ca.Genome.occurrences).parameters)[1:] == ["sites", "page_length", "page_starts"]
    assert sig(ca.Genome.occurrences).parameters["page_starts"].default is None
    assert sig(ca.Genome.occurrences_device).parameters["page_starts"].default is None
    assert list(sig(ca.Consensus.selection_pages).parameters)[1:] == ["batch_size", "page_length"]
    assert list(sig(ca.Consensus.bowtie).parameters)[1:] == ["genome", "page_length", "batch_size"]
    assert sig(ca.Consensus.bowtie).parameters["batch_size"].default == 0
    assert sig(ca.read_bowtie_output).parameters["page_starts"].default is None
    p = sig(ca.ResultTable.__init__).parameters
    assert p["rows"].default is None and p["header"].default is True
    for name in ("run", "batches", "run_to_file"):
        assert callable(getattr(ca.pipeline, name)), name
    assert list(sig(ca.pipeline.batches).parameters) == list(sig(ca.pipeline.run).parameters)
    assert list(sig(ca.pipeline.run_to_file).parameters) == ["path"] + list(sig(ca.pipeline.run).parameters)
    doc = ca.pipeline.batches.__doc__
    for phrase in ("batch_size", "rnafold_page_length", "Paginator.py:29-30", "Crackling.py:420", ":458"):
        assert phrase in doc, phrase


def test_argument_errors_come_before_any_device_call():
    from crackling_amd import _lib
    lib = _lib.lib
    fake = C.c_void_p(0x1000)  # never read: every call below fails on an argument ahead of it
    starts = (C.c_uint64 * 2)(0, 1)
    # the Bowtie step
    assert lib.issl_genome_occurrences_paged(None, fake, 1, starts, 1, fake) == -1 and b"null" in lib.issl_last_error()
    assert lib.issl_genome_occurrences_paged(fake, None, 1, starts, 1, fake) == -1
    assert lib.issl_genome_occurrences_paged(fake, fake, 1, starts, 1, None) == -1
    assert lib.issl_genome_occurrences_paged(fake, fake, 1, None, 1, fake) == -1
    assert lib.issl_genome_occurrences_paged(fake, None, 0, None, 1, None) == -1   # pages without their boundaries
    assert lib.issl_genome_occurrences_paged_device(None, fake, 1, fake, 1, fake, None) == -1
    assert lib.issl_genome_occurrences_paged_device(fake, None, 1, fake, 1, fake, None) == -1
    assert lib.issl_genome_occurrences_paged_device(fake, fake, 1, None, 1, fake, None) == -1
    assert lib.issl_genome_occurrences_paged_device(fake, fake, 1, fake, 1, None, None) == -1
    # the pages
    d, n = C.c_void_p(0x1234), C.c_uint64(7)
    assert lib.issl_consensus_selection_pages(None, 0, 0, C.byref(d), C.byref(n)) == -1
    assert lib.issl_consensus_selection_pages(fake, 0, 0, None, C.byref(n)) == -1
    assert lib.issl_consensus_selection_pages(fake, 0, 0, C.byref(d), None) == -1
    # the row range: the checks of issl_results_build in its order
    cfg = _lib.ResultsConfig(b",", 4, b"and", 75.0)
    h = C.c_void_p(0x1234)
    args = (None, 0, None, 0, None, 0, None, None, None, None, 0, 0, 0)
    assert lib.issl_results_build_rows(None, fake, *args, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    assert lib.issl_results_build_rows(fake, None, *args, C.byref(cfg), C.byref(h)) == -1
    assert lib.issl_results_build_rows(fake, fake, *args, None, C.byref(h)) == -1
    assert lib.issl_results_build_rows(fake, fake, *args, C.byref(cfg), None) == -1
    h = C.c_void_p(0x1234)
    assert lib.issl_results_build_rows(fake, fake, *args, C.byref(_lib.ResultsConfig(b":", 4, b"and", 75.0)), C.byref(h)) == -4
    assert h.value is None and b"delimiter" in lib.issl_last_error()


def test_read_bowtie_output_with_page_starts():
    """The pages of a run in batches, for a caller with a real Bowtie2: explicit boundaries file the reads as the uniform
    ones do, and a cut between two guides of one 20-mer leaves both tested."""
    import crackling_amd as ca
    import bowtie_util as bu
    guides = ["ACGTACGTACGTACGTACGTAGG", "TTGTACGTACGTACGTACGACGG", "ACGTACGTACGTACGTACGTCGG"]
    line = lambda k, read: f"{k}\t4\t*\t0\t0\t*\t*\t0\t0\t{read}\t{'I' * 23}\tYT:Z:UU"  # noqa: E731
    sam = "".join(line(8 * k + v, g[:20] + pam) + "\n" for k, g in enumerate(guides) for v, pam in enumerate(bu.PAMS))
    for page_length in (0, 1, 2):
        uniform = [0] + list(range(page_length, 3, page_length)) + [3] if page_length else [0, 3]
        got = ca.read_bowtie_output(sam, guides, page_starts=uniform)
        assert got.tobytes() == ca.read_bowtie_output(sam, guides, page_length=page_length).tobytes()
    one = ca.read_bowtie_output(sam, guides, page_starts=[0, 3])
    assert one["code"].tolist() == [2, 1, 1] and one["source"].tolist() == [0xFFFFFFFF, 1, 2]
    cut = ca.read_bowtie_output(sam, guides, page_starts=np.array([0, 0, 2, 2, 3], dtype=np.uint64))  # empty pages too
    assert cut["code"].tolist() == [1, 1, 1] and cut["source"].tolist() == [0, 1, 2]
    for bad in ([1, 3], [0, 2], [0, 2, 1, 3], []):
        with pytest.raises(ValueError):
            ca.read_bowtie_output(sam, guides, page_starts=bad)
