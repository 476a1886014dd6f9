"""GPU: RNAfold's exchange on the device (crackling_amd.Folds, issl_folds_* of include/issl_hip.h) against the host model of
tests/folds_util.py -- which tests/test_folds_model.py pins to the package's Python helpers and to the shared rules under
the sanitizers -- against the helpers themselves wherever a text holds none of the bytes they part from the reference on,
and through Consensus.finish, ResultTable and pipeline.run."""
import csv
import io

import numpy as np
import pytest

import crackling_amd as ca
import bowtie_util as bu
import consensus_util as cu
import folds_util as fu
import results_util as ru

pytestmark = pytest.mark.gpu
RUNS = ru.golden_runs()
IDS = [r["name"] for r in RUNS]
SIZES = [0, 1, 255, 256, 257, 1000]


class World:
    """Guide set and an unfinished consensus at ultralow (every guide is folded) over one crafted FASTA."""

    def __init__(self, n_guides, seed=7):
        self.blob = ru.crafted_fasta(n_guides, seed)
        self.gs = ca.GuideSet.extract([self.blob])
        self.c = self.consensus()
        assert self.gs.n_guides == n_guides == self.c.n_fold
        self.guides = self.c.fold_guides()
        seen, self.distinct = set(), []  # one guide per key guide[1:20], for the crafted answers
        for g in self.guides:
            if g[1:20] not in seen:
                seen.add(g[1:20])
                self.distinct.append(g)

    def consensus(self):
        return ca.Consensus(self.gs, optimisation="ultralow", n=2, model=cu.golden_model())

    def close(self):
        self.c.close()
        self.gs.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(n):
        if n not in made:
            made[n] = World(n)
        return made[n]

    yield get
    for w in made.values():
        w.close()


@pytest.fixture(scope="module")
def golden():
    genome = ca.Genome.open([(bu.GOLDEN / "genome.fa").read_bytes()])
    index = ca.IsslIndex.open(bu.GOLDEN / "index.issl").upload(0)
    yield genome, index
    index.close()
    genome.close()


def check_read(w, text, first=0, n=None, code=None):
    """One read of `text` for rows [first, first + n) of w's fold list against the model (and the helpers); a text the model
    refuses must be refused with the same code and row, keep nothing, and leave the page readable."""
    n = len(w.guides) - first if n is None else n
    page = w.guides[first:first + n]
    with w.c.folds() as f:
        try:
            want_folds, want_texts = fu.model(text, page)
        except fu.Refused as refused:
            assert code == refused.code
            with pytest.raises(ca.IsslError) as e:
                f.read(text, first, n)
            assert e.value.code == refused.code and f"row {first + refused.row} " in e.value.message, e.value.message
            assert f.n_read == 0 and f.folds.tobytes() == bytes(16 * len(w.guides)) and f.texts() == [None] * len(w.guides)
            good = fu.pairs_text(fu.default_pairs(page[:50]))
            f.read(good, first, n)  # after a failed read the page reads cleanly
            assert f.folds[first:first + n].tobytes() == fu.model(good, page)[0].tobytes() and f.n_read == n
            return None
        assert code is None
        f.read(text, first, n)
        folds, texts = f.folds, f.texts()
        assert f.n_read == n and f.text_bytes == (len(text) if n else 0)
    assert folds[first:first + n].tobytes() == want_folds.tobytes()
    assert texts[first:first + n] == want_texts
    assert folds[:first].tobytes() == bytes(16 * first) and texts[:first] == [None] * first
    assert not folds[first + n:]["present"].any() and texts[first + n:] == [None] * (len(w.guides) - first - n)
    if not fu.differs(text):
        as_str = text.decode("latin-1")
        assert ca.read_rnafold_output(as_str, page).tobytes() == want_folds.tobytes()
        assert ca.read_rnafold_text(as_str, page) == want_texts
    return folds, texts


# ---- 1. the golden runs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_golden_runs(golden, run):
    genome, index = golden
    text = ru.golden_fold_text(run)
    kw = cu.golden_keywords(run)
    with ca.GuideSet.extract([ru.golden_input(run)]) as gs, ca.Consensus(gs, **kw) as c, ca.Consensus(gs, **kw) as host:
        guides = c.fold_guides()
        with c.folds() as f:
            assert f.input() == c.fold_input().encode() and len(f) == c.n_fold
            f.read(text)
            want = ca.read_rnafold_output(text, guides)
            assert f.folds.tobytes() == want.tobytes() and f.texts() == ca.read_rnafold_text(text, guides)
            assert f.folds.tobytes() == fu.model(text.encode(), guides)[0].tobytes()
            c.finish(f)
            host.finish(want if c.n_fold else None)
            assert c.rows.tobytes() == host.rows.tobytes() and c.selected.tolist() == host.selected.tolist()
            with pytest.raises(ca.IsslError) as e:
                c.finish(f)
            assert e.value.code == -7
            with pytest.raises(ca.IsslError) as e:
                host.finish(f)  # (the folds of another consensus)
            assert e.value.code == -1
    config = ru.golden_keywords(run)
    asked = []

    def rnafold(lines):
        asked.append(lines)
        return text

    def rnafold_bytes(lines):
        asked.append(lines)
        return text.encode()

    by_default = ca.pipeline.run([ru.golden_input(run)], genome, index, config, rnafold)
    by_device = ca.pipeline.run([ru.golden_input(run)], genome, index, dict(config, rnafold_reader="device"), rnafold_bytes)
    by_host = ca.pipeline.run([ru.golden_input(run)], genome, index, dict(config, rnafold_reader="host"), rnafold)
    assert by_default == by_device == by_host == ru.golden_bytes(run["name"])
    assert all(isinstance(a, str) for a in asked) and len(set(asked)) <= 1
    with pytest.raises(ValueError):
        ca.pipeline.run([ru.golden_input(run)], genome, index, dict(config, rnafold_reader="gpu"), rnafold)


# ---- 2. crafted answers against the model ---------------------------------------------------------------------------------

def test_crafted_answers(worlds):
    w = worlds(1000)
    assert len(w.distinct) >= 300
    with w.c.folds() as f:
        group = f.bytes_per_group
    assert group >= 32 and group % 16 == 0
    cases = fu.crafted_cases(w.distinct[:300], group)
    assert len(cases) > 100 and sum(code is not None for _, _, code in cases) > 20
    for name, text, code in cases:
        try:
            check_read(w, text, code=code)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("n", SIZES)
def test_sizes(worlds, n, tmp_path):
    w = worlds(n)
    with w.c.folds() as f:
        want = w.c.fold_input().encode()
        assert f.input() == want and len(want) == 101 * n and f.n_fold == n
        for first, count in ((0, 0), (0, 1), (n // 2, n - n // 2), (n, 0), (max(n - 1, 0), min(n, 1)), (3, 254), (1, 256)):
            if first + count <= n:
                assert f.input(first, count) == want[101 * first:101 * (first + count)], (first, count)
        f.write_input(tmp_path / "in.txt", 0, n)
        assert (tmp_path / "in.txt").read_bytes() == want
        for first, count in ((n + 1, 0), (n, 1), (0, n + 1), (1 << 40, 1), (1, (1 << 64) - 1)):
            with pytest.raises(ca.IsslError) as e:
                f.input(first, count)
            assert e.value.code == -1
            with pytest.raises(ca.IsslError) as e:
                f.read(b"", first, count)
            assert e.value.code == -1
        if n:
            import ctypes as C
            out = C.create_string_buffer(101 * n)
            assert ca.lib.issl_folds_input_copy(f._h, 0, n, out, 101 * n - 1) == -1
    pairs = fu.default_pairs(w.guides, seed=n)
    for text in (fu.pairs_text(pairs), fu.pairs_text(pairs[::2], "\r\n"), fu.pairs_text(pairs[::-1], "\r")[:-1], b"", b"\r"):
        folds, texts = check_read(w, text)
        assert len(folds) == n
    if n:
        answer = tmp_path / "out.txt"
        answer.write_bytes(fu.pairs_text(pairs))
        with w.c.folds() as f:
            f.read_file(answer)
            want_folds, want_texts = fu.model(fu.pairs_text(pairs), w.guides)
            assert f.folds.tobytes() == want_folds.tobytes()
            assert f.text_of(n - 1, 0) == want_texts[n - 1][0].encode() and f.text_of(0, 1) == want_texts[0][1].encode()
            assert f.text_of(0, 2) == want_texts[0][2].encode()
            with pytest.raises(ca.IsslError) as e:
                f.read_file(tmp_path / "absent.txt")
            assert e.value.code == -7  # (read already: the state is looked at ahead of the file)
        with w.c.folds() as f:
            assert f.text_of(0, 2) is None
            with pytest.raises(ca.IsslError) as e:
                f.read_file(tmp_path / "absent.txt")
            assert e.value.code == -2 and f.n_read == 0


# ---- 3. pages ----------------------------------------------------------------------------------------------------------

def test_pages_have_their_own_dictionary(worlds):
    w = worlds(1000)
    g = w.distinct
    row_of = {x: k for k, x in enumerate(w.guides)}
    pages = [(0, 300), (300, 350), (650, 350)]
    own = lambda a, n: [x for x in g if a <= row_of[x] < a + n]
    first, second, third = (own(a, n) for a, n in pages)
    stray = second[0]  # a guide of the second page, answered in the first page's text only
    texts = [fu.pairs_text(fu.default_pairs(first + [stray], seed=1)), fu.pairs_text(fu.default_pairs(second[1:], seed=2)),
             fu.pairs_text(fu.default_pairs(third, seed=3), "\r\n")]
    with w.c.folds() as f, w.consensus() as c, w.consensus() as host:
        f2 = c.folds()
        for k in (0, 2):
            f.read(texts[k], *pages[k])
            f2.read(texts[k], *pages[k])
        want = np.zeros(1000, dtype=ca.FOLD_DTYPE)
        want_texts = [None] * 1000
        for k in (0, 2):
            a, n = pages[k]
            want[a:a + n], want_texts[a:a + n] = fu.model(texts[k], w.guides[a:a + n])
        assert f.n_read == 650 and f.folds.tobytes() == want.tobytes() and f.texts() == want_texts  # the second page: unread
        for a, n in ((0, 300), (0, 1), (299, 2), (600, 100), (0, 1000), (999, 1)):
            with pytest.raises(ca.IsslError) as e:
                f.read(texts[0], a, n)
            assert e.value.code == -7, (a, n)
        assert f.folds.tobytes() == want.tobytes() and f.n_read == 650
        c.finish(f2)
        host.finish(want)
        assert c.rows.tobytes() == host.rows.tobytes() and (c.rows["ss"][300:650] == 2).all() and (c.rows["ss"][:300] != 2).any()
        with ca.ResultTable(c, f2) as t, ca.ResultTable(host, want_texts) as t_host:
            got = t.to_bytes()
            assert got == t_host.to_bytes()
        lines = list(csv.reader(io.StringIO(got.decode("latin-1"), newline="")))[1:]
        assert len(lines) == 1000 and all(l[11:14] == ["?", "?", "?"] for l in lines[300:650]) and lines[0][11] != "?"
        f.read(texts[1], *pages[1])  # the second page, with its own text: the stray pair of the first page is not found
        a, n = pages[1]
        want[a:a + n], want_texts[a:a + n] = fu.model(texts[1], w.guides[a:a + n])
        assert f.n_read == 1000 and f.folds.tobytes() == want.tobytes() and f.texts() == want_texts
        assert want_texts[row_of[stray]] is None and want["present"][row_of[stray]] == 0
        assert f.text_bytes == sum(len(x) for x in texts)
        f2.close()


# ---- 4. the table ------------------------------------------------------------------------------------------------------

def test_tables_with_folds_equal_tables_with_the_helper(worlds):
    w = worlds(1000)
    g = w.distinct
    odd_first = [' in ner', ' "q"', ',c', ';s', '|p', '\tt', ' a,"b";c|d\te f', '""', ' x  y']
    odd_second = ['..".. (-5.30)', '.,.. (-5.30) x', '.;|. x"5,3"x (-5.5)', '..\t.. q|;q (\t-1.0)', '"" x""x (-2)', '.... ,(x']
    pairs = fu.default_pairs(g)
    for k in range(len(pairs)):
        a, b = pairs[k]
        if k % 3 == 0:
            a = a + odd_first[(k // 3) % len(odd_first)]
        if k % 5 == 0:
            b = odd_second[(k // 5) % len(odd_second)]
        pairs[k] = (a, b)
    text = fu.pairs_text([p for k, p in enumerate(pairs) if k % 7])
    assert not fu.differs(text)
    with w.consensus() as c, c.folds() as f:
        f.read(text)
        helper = ca.read_rnafold_text(text.decode(), w.guides)
        assert f.texts() == helper == fu.model(text, w.guides)[1]
        c.finish(f)
        packed = ca.PackedFolds(helper)
        n = w.gs.n_guides
        for delimiter in ru.DELIMITERS:
            for flags in (0, ca.results.DIRECT):
                with ca.ResultTable(c, f, None, None, delimiter, flags=flags) as t, ca.ResultTable(c, packed, None, None, delimiter, flags=flags) as th:
                    want = th.to_bytes()
                    assert t.to_bytes() == want, (delimiter, flags)
                    offsets = th.row_offsets_tensor().cpu().numpy().astype(np.int64)
                    assert t.row_offsets_tensor().cpu().numpy().astype(np.int64).tolist() == offsets.tolist()
                    per_group = t.rows_per_group
                for a, b in ((0, 0), (0, 1), (per_group - 1, per_group + 1), (per_group, 2 * per_group), (n - 3, n), (n, n)):
                    with ca.ResultTable(c, f, None, None, delimiter, flags=flags, rows=(a, b - a), header=False) as t:
                        assert t.to_bytes() == want[offsets[a]:offsets[b]], (delimiter, flags, a, b)
            if delimiter == " ":
                assert b'"G' in want and b' in ner"' in want  # a first line with an inner blank is quoted
            assert b'""' in want
        with w.consensus() as other:
            other.finish(np.zeros(other.n_fold, dtype=ca.FOLD_DTYPE))
            with pytest.raises(ValueError):
                ca.ResultTable(other, f)


# ---- 5. the same bytes on every run --------------------------------------------------------------------------------------

def test_two_reads_give_the_same_bytes(worlds):
    w = worlds(1000)
    pairs = fu.default_pairs(w.distinct)
    dup = pairs + [(a, fu.plain_line("-%d.25" % (k % 50))) for k, (a, _) in enumerate(pairs)] * 3
    text = fu.pairs_text([dup[i] for i in np.random.default_rng(3).permutation(len(dup))])
    seen = set()
    for _ in range(3):
        with w.c.folds() as f:
            f.read(text)
            seen.add((f.folds.tobytes(), f.spans.tobytes(), f.text()))
    assert len(seen) == 1
    folds = np.frombuffer(next(iter(seen))[0], dtype=ca.FOLD_DTYPE)
    assert folds.tobytes() == fu.model(text, w.guides)[0].tobytes()
