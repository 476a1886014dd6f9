"""GPU: the result table (crackling_amd.ResultTable, pipeline.run, repr_f64; issl_results_* of include/issl_hip.h) against
the reference's own output files (tests/golden/results) and, byte for byte and offset for offset, against the csv model of
tests/results_util.py, which tests/test_results_model.py pins to those files."""
import struct

import numpy as np
import pytest

import crackling_amd as ca
import bowtie_util as bu
import consensus_util as cu
import results_util as ru

pytestmark = pytest.mark.gpu
RUNS = ru.golden_runs()
IDS = [r["name"] for r in RUNS]


@pytest.fixture(scope="module")
def golden():
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    index = ca.IsslIndex.open(bu.GOLDEN / "index.issl").upload(0)
    yield genome, index
    index.close()
    genome.close()


# ---- 1. the reference's own files ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_golden_parity(golden, run):
    genome, index = golden
    asked = []

    def rnafold(fold_input):
        asked.append(fold_input)
        return ru.golden_fold_text(run)

    got = ca.pipeline.run([ru.golden_input(run)], genome, index, ru.golden_keywords(run), rnafold)
    assert got == ru.golden_bytes(run["name"])
    assert len(asked) == (1 if run["mm10db"] else 0)


# ---- 2. the model, on crafted input -------------------------------------------------------------------------------------

class Crafted:
    """Guide set, consensus, Bowtie step and scores of one crafted FASTA, and the model's arguments for them."""

    def __init__(self, n_guides, seed, long_header=0):
        import torch
        self.blob = ru.crafted_fasta(n_guides, seed, long_header)
        self.gs = ca.GuideSet.extract([self.blob])
        assert self.gs.n_guides == n_guides
        self.genome = ca.Genome.open([self.blob])
        self.c = ca.Consensus(self.gs, optimisation="ultralow", n=2, model=cu.golden_model())
        rng = np.random.default_rng(seed)
        folds = np.zeros(self.c.n_fold, dtype=ca.FOLD_DTYPE)
        folds["energy"] = rng.choice([-35.0, -30.0, -29.9, -18.0, -17.9, -5.3], self.c.n_fold)
        folds["scaffold"] = rng.integers(0, 2, self.c.n_fold)
        folds["present"] = rng.integers(0, 5, self.c.n_fold) > 0
        self.c.finish(folds if self.c.n_fold else None)
        self.bowtie = self.c.bowtie(self.genome, 7)
        self.scores = ru.crafted_scores(self.c.selected, seed)
        self.d_scores = tuple(torch.from_numpy(np.ascontiguousarray(x).astype(np.int64 if k == 0 else np.float64)).cuda()
                              for k, x in enumerate(self.scores))
        self.seed = seed

    def table(self, delimiter, method="and", threshold=75.0, flags=0, parts=(True, True, True)):
        ft = ru.crafted_fold_texts(self.c.n_fold, self.seed, delimiter)
        t = ca.ResultTable(self.c, ft if parts[0] else None, self.bowtie if parts[1] else None,
                           self.d_scores if parts[2] else None, delimiter, method, threshold, flags)
        kw = dict(guides=self.gs.guides, record_names=[n for n, _ in self.gs.records], rows=self.c.rows, delimiter=delimiter,
                  method=method, threshold=threshold)
        if parts[0]:
            kw.update(fold_rows=self.c.fold_rows, folds_text=ft)
        if parts[1]:
            kw.update(selection=self.c.selected, bowtie_rows=self.bowtie.rows, genome_names=[n for n, _ in self.genome.records])
        if parts[2]:
            kw.update(scores=self.scores)
        return t, ru.model_table(**kw)

    def close(self):
        self.c.close()
        self.genome.close()
        self.gs.close()


def same(table, model):
    want, offsets = model
    got = table.to_bytes()
    assert table.n_bytes == len(want) and table.n_rows == len(offsets) - 1
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else min(len(got), len(want))
        raise AssertionError(f"first difference at byte {at}: {got[max(0, at - 60):at + 60]!r} != {want[max(0, at - 60):at + 60]!r}")
    assert table.text_tensor().cpu().numpy().tobytes() == want
    assert table.row_offsets_tensor().cpu().numpy().astype(np.uint64).tolist() == offsets.tolist()


@pytest.fixture(scope="module")
def big():
    """Several hundred records, one header line of 100 KB: more than one workgroup, rows that fill the staging buffer more
    than once, one row larger than it."""
    c = Crafted(700, 5, long_header=100000)
    yield c
    c.close()


@pytest.mark.parametrize("delimiter", ru.DELIMITERS, ids=["comma", "tab", "semicolon", "pipe", "space"])
def test_model_parity_for_every_delimiter(big, delimiter):
    t, model = big.table(delimiter)
    with t:
        assert t.rows_per_group and big.gs.n_guides > 2 * t.rows_per_group
        same(t, model)
    want = model[0]
    assert want.count(b"\n") == 701 and max(len(x) for x in want.split(b"\n")) > 100000  # the long header is in a row
    assert any(int(g["seen"]) > 1 for g in big.gs.guides) and any(ln == 0 for _, ln in big.gs.records) is False
    assert len({int(r) for r in big.gs.guides["record"]}) < len(big.gs.records)               # a record without a guide


def test_model_parity_with_the_direct_store_path(big):
    t, model = big.table(",", flags=ca.results.DIRECT)
    with t:
        same(t, model)
    t, model = big.table("\t", flags=ca.results.DIRECT, method="mit", threshold=99.0)
    with t:
        same(t, model)


@pytest.mark.parametrize("method,threshold", [("mit", 75.0), ("cfd", 75.0), ("or", 50.0), ("avg", 75.0), ("AND", 75.0), (" Mit ", 1.0),
                                              ("none", 75.0)])
def test_methods_and_thresholds(big, method, threshold):
    t, model = big.table(",", method=method, threshold=threshold)
    with t:
        same(t, model)


@pytest.mark.parametrize("parts", [(False, False, False), (True, False, False), (False, True, False), (False, False, True)])
def test_stages_that_are_left_out_stay_untested(big, parts):
    t, model = big.table(";", parts=parts)
    with t:
        same(t, model)


def test_set_sizes_around_a_workgroup():
    with ca.GuideSet.extract([b">none\nATATATATATATATATATATATATATATATAT\n"]) as gs, ca.Consensus(gs, model=cu.golden_model()) as c:
        assert gs.n_guides == 0
        c.finish()
        with ca.ResultTable(c) as t:
            per_group = t.rows_per_group
            assert t.n_rows == 0 and t.to_bytes() == (",".join(ru.ORDER) + "\n").encode()
            assert t.row_offsets_tensor().cpu().tolist() == [t.n_bytes]
    assert per_group >= 64
    for n in (1, per_group - 1, per_group, per_group + 1):
        crafted = Crafted(n, 11 + n)
        for flags in (0, ca.results.DIRECT):
            t, model = crafted.table(",", flags=flags)
            with t:
                same(t, model)
        crafted.close()


def test_two_builds_give_the_same_bytes(big):
    a, _ = big.table("|")
    b, _ = big.table("|")
    with a, b:
        assert a.to_bytes() == b.to_bytes()
        assert a.row_offsets_tensor().cpu().tolist() == b.row_offsets_tensor().cpu().tolist()


def test_write_and_append(big, tmp_path):
    t, model = big.table(",")
    with t:
        t.write(tmp_path / "out.txt")
        assert (tmp_path / "out.txt").read_bytes() == model[0]
        t.write(tmp_path / "out.txt", append=True)
        assert (tmp_path / "out.txt").read_bytes() == model[0] * 2
        with pytest.raises(ca.IsslError) as e:
            t.write(tmp_path / "no" / "such" / "dir.txt")
        assert e.value.code == -2


def test_errors_of_a_built_table(big):
    import torch
    with ca.Consensus(big.gs, model=cu.golden_model()) as unfinished:
        with pytest.raises(ValueError):
            ca.ResultTable(unfinished)
        from crackling_amd import _lib
        import ctypes as C
        h = C.c_void_p()
        cfg = _lib.ResultsConfig(b",", 0, b"and", 75.0)
        rc = _lib.lib.issl_results_build(big.gs._h, unfinished._h, None, 0, None, 0, None, 0, None, None, None, None, 0, C.byref(cfg), C.byref(h))
        assert rc == -7 and h.value is None
    with pytest.raises(ValueError):
        ca.ResultTable(big.c, folds_text=[None] * (big.c.n_fold + 1))
    with pytest.raises(ca.IsslError) as e:
        ca.ResultTable(big.c, delimiter=":")
    assert e.value.code == -4
    rows = torch.arange(big.gs.n_guides + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ca.IsslError) as e:
        ca.ResultTable(big.c, scores=(rows, rows.double(), rows.double()))
    assert e.value.code == -1


# ---- 3. repr ------------------------------------------------------------------------------------------------------------

def repr_cases():
    rng = np.random.default_rng(2)
    parts = [rng.integers(0, 1 << 64, 150000, dtype=np.uint64).view(np.float64),
             np.array([2.0 ** e for e in range(-1074, 1024)])]
    p10 = np.array([float(f"1e{e}") for e in range(-323, 309)])
    parts += [p10, np.nextafter(p10, np.inf), np.nextafter(p10, -np.inf)]
    edge = np.array([1e-4, 1e16, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308, 2.225073858507201e-308, 0.0, np.inf,
                     9007199254740993.0, 9007199254740992.0, 1e22, 1e23, 0.1, 0.3, 1 / 3, 45.0, 100.0, 5e-6, 123456789012345680.0])
    with np.errstate(over="ignore"):  # (the neighbour above the largest double is inf)
        parts += [edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf)]
    parts.append(rng.integers(1, 1 << 52, 5000, dtype=np.uint64).view(np.float64))           # subnormals
    parts.append(rng.uniform(0, 100, 20000))
    parts.append(np.round(rng.uniform(0, 100, 10000), 6))
    golden = set()
    for run in RUNS:
        for line in ru.golden_bytes(run["name"]).decode().splitlines()[1:]:
            v = line.split(",")[1]
            if v != "?":
                golden.add(float(v))
    parts.append(np.array(sorted(golden)))
    v = np.concatenate(parts)
    return np.concatenate([v, -v])


def test_repr_f64_is_pythons_repr():
    import torch
    v = repr_cases()
    assert 190000 <= len(v) and np.isnan(v).sum() > 10 and (v == 0).sum() >= 2 and np.isinf(v).sum() >= 2
    got = ca.repr_f64(torch.from_numpy(v).cuda())
    want = [repr(x).encode() for x in v.tolist()]
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, (len(bad), bad[:5])
    assert b"nan" in got and b"-0.0" in got and b"-inf" in got and b"5e-324" in got and b"9007199254740992.0" in got
    assert ca.repr_f64(torch.empty(0, dtype=torch.float64, device="cuda")) == []
