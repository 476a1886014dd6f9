"""Host model of a batched run: what [input] batch-size and the two page lengths change in the reference's output file
(Batchinator.py, Paginator.py, Crackling.py:276-305, :406-498, :611-723).  A batch is a run of consecutive rows of the
guide set; the pages of the Bowtie step and of RNAfold start again with every batch, and nothing else of a row depends on
the batch.  Nothing of the library runs here: the boundaries are counted on the host, the Bowtie rows are
bowtie_util.Model.rows per page, RNAfold's answers are read per page, and everything goes through
results_util.model_table.  tests/test_batches_model.py pins this to the reference's own files (tests/golden/batches,
tools/make_golden_batches.py) before tests/test_batches_gpu.py compares the device with it."""
import gzip
import json
import pathlib

import numpy as np

import bowtie_util as bu
import consensus_util as cu
import guides_util as gu
import results_util as ru

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "batches"


# ---- batches and pages ------------------------------------------------------------------------------------------------

def batches(n, batch_size):
    """The batches of a set of n rows: [(first row, end)]; batch_size 0: one batch."""
    if batch_size <= 0:
        return [(0, n)] if n else []
    return [(a, min(n, a + batch_size)) for a in range(0, n, batch_size)]


def page_starts(listed, n, batch_size, page_length):
    """listed: ascending rows of the set (the selection, the fold list).  -> uint64 boundaries in positions of `listed`:
    page p is [starts[p], starts[p + 1]).  Every batch cuts its share of the list into pages of page_length; 0: one page per
    batch that lists any row.  No page is empty; the first entry is 0 and the last len(listed)."""
    listed = np.asarray(listed, dtype=np.int64)
    starts = []
    for a, b in batches(n, batch_size):
        lo, hi = int(np.searchsorted(listed, a)), int(np.searchsorted(listed, b))
        if page_length > 0:
            starts += list(range(lo, hi, page_length))
        elif hi > lo:
            starts.append(lo)
    assert (starts[:1] or [0]) == [0]
    return np.array(starts + [len(listed)], dtype=np.uint64)


def uniform_starts(n, page_length):
    """The boundaries issl_genome_occurrences(page_length) works with."""
    return page_starts(np.arange(n), n, 0, page_length)


def paged_rows(model, sigs, starts):
    """bowtie_util.Model.rows for explicit pages: every page a call of its own with one page, `source` shifted to the
    page's place.  Equal neighbours among the boundaries are an empty page."""
    sigs = np.asarray(sigs, dtype=np.uint64)
    starts = [int(x) for x in starts]
    assert starts[0] == 0 and starts[-1] == len(sigs) and starts == sorted(starts)
    rows = np.zeros(len(sigs), dtype=bu.DTYPE)
    for a, b in zip(starts, starts[1:]):
        if b > a:
            page = model.rows(sigs[a:b], 0)
            page["source"] = np.where(page["source"] == bu.NONE, bu.NONE, page["source"] + np.uint32(a))
            rows[a:b] = page
    return rows


# ---- RNAfold ----------------------------------------------------------------------------------------------------------

def fold_lines(guides):
    """The lines the reference writes for RNAfold (Crackling.py:421)."""
    import crackling_amd as ca
    return [f"G{g[1:20]}{ca.consensus.SCAFFOLD}" for g in guides]


def answer_page(whole_text, asked):
    """What an RNAfold that printed `whole_text` for a superset prints for the lines `asked`: the pairs whose first line is
    an asked line with T read as U (RNAfold prints U, the recipe's stand-in echoes the line), in the order of the whole text."""
    want = {line.replace("T", "U") for line in asked.split()}
    lines = whole_text.splitlines()
    return "".join(a + "\n" + b + "\n" for a, b in zip(lines[0::2], lines[1::2]) if a.rstrip().replace("T", "U") in want)


def fold_answers(whole_text, fold_rows, fold_guides, n, batch_size, rnafold_page_length):
    """-> (FOLD_DTYPE array or None for an empty list, the three texts per row of the list, the number of RNAfold runs).
    rnafold_page_length None: one run and one dict over the whole list; 0: no guide is tested (Paginator.py:29-30 hands
    out the generator, Crackling.py:420 consumes it, :458 sees nothing); P > 0: one run and one dict per page."""
    import crackling_amd as ca
    if not len(fold_guides):
        return None, [], 0
    if rnafold_page_length is None:
        return ca.read_rnafold_output(whole_text, fold_guides), ru.read_rnafold_text(whole_text, fold_guides), 1
    if rnafold_page_length == 0:
        return np.zeros(len(fold_guides), dtype=ca.consensus.FOLD_DTYPE), [None] * len(fold_guides), 0
    starts = [int(x) for x in page_starts(fold_rows, n, batch_size, rnafold_page_length)]
    folds, texts = [], []
    for a, b in zip(starts, starts[1:]):
        text = answer_page(whole_text, "\n".join(fold_lines(fold_guides[a:b])))
        folds.append(ca.read_rnafold_output(text, fold_guides[a:b]))
        texts += ru.read_rnafold_text(text, fold_guides[a:b])
    return np.concatenate(folds), texts, len(starts) - 1


# ---- the goldens ------------------------------------------------------------------------------------------------------

def golden_runs():
    return json.loads((GOLDEN / "runs.json").read_text())


def golden_bytes(name):
    return gzip.decompress((GOLDEN / f"{name}.txt.gz").read_bytes())


def golden_fold_text(run):
    return ru.golden_fold_text(dict(run, name=run["base"]))


def golden_keywords(run):
    """The keywords of crackling_amd.pipeline.run's config for a run of runs.json."""
    kw = ru.golden_keywords(run)
    kw["batch_size"] = run["batch_size"]
    if run["rnafold_page_length"] is not None:
        kw["rnafold_page_length"] = run["rnafold_page_length"]
    return kw


def rnafold_runs(run):
    """How often the reference's loop runs RNAfold and reads its answer in this run (never with [rnafold] page-length 0)."""
    seqs_guides = gu.brute_force(gu.parse([ru.golden_input(run)]))
    seqs = ru.guide_strings(seqs_guides)
    kw = ru.golden_keywords(run)
    m = cu.Model(seqs, seqs_guides["seen"], **{k: kw[k] for k in ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model",
                                                                  "sgrna_threshold", "low_energy", "high_energy")})
    if run["rnafold_page_length"] is None:
        return 1 if len(m.fold_rows) else 0
    if run["rnafold_page_length"] == 0:
        return 0
    return len(page_starts(m.fold_rows, len(seqs), run["batch_size"], run["rnafold_page_length"])) - 1


def host_stages(run, fold_text):
    """results_util.host_stages with the batches of the run: -> (keyword arguments of model_table, RNAfold runs)."""
    import oracle_util as ou
    records = gu.parse([ru.golden_input(run)])
    guides = gu.brute_force(records)
    seqs = ru.guide_strings(guides)
    n = len(seqs)
    kw = ru.golden_keywords(run)
    m = cu.Model(seqs, guides["seen"], **{k: kw[k] for k in ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model",
                                                             "sgrna_threshold", "low_energy", "high_energy")})
    fold_guides = [seqs[j] for j in m.fold_rows]
    folds, folds_text, calls = fold_answers(fold_text, m.fold_rows, fold_guides, n, run["batch_size"], run["rnafold_page_length"])
    m.finish(folds)
    out = dict(guides=guides, record_names=[name for name, _ in records], rows=m.rows, fold_rows=m.fold_rows, folds_text=folds_text,
               delimiter=run["delimiter"], method=run["method"], threshold=float(run["score_threshold"]))
    if run["enabled"]:
        genome = bu.golden_model()
        sel = m.selected
        sigs = np.array([bu.sig(seqs[j][:20]) for j in sel], dtype=np.uint64)
        brows = paged_rows(genome, sigs, page_starts(sel, n, run["batch_size"], run["page_length"]))
        scored = sel if m.level < 2 else sel[brows["code"] != 0]
        oracle = ou.OracleIndex(bu.GOLDEN / "index.issl")
        mit, cfd = oracle.score(np.array([bu.sig(seqs[j][:20]) for j in scored], dtype=np.uint64), run["max_distance"],
                                float(run["score_threshold"]), run["method"])
        oracle.close()
        out.update(selection=sel, bowtie_rows=brows, genome_names=[name.encode() for name, _ in genome.records],
                   scores=(scored, mit, cfd))
    return out, calls
