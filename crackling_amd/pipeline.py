"""Crackling.py from FASTA to its output file over the resident stages: extract -> consensus -> RNAfold -> Bowtie step ->
off-target scores -> result table.  Glue over the package's classes; no configuration file is read, and nothing is written
to disk but by run_to_file.

The reference works through the guides in batches of [input] batch-size -- consecutive distinct guides in first-seen
order, which are consecutive rows of the guide set -- and appends every batch's rows to its file.  The stages here stay
whole-set (the Bowtie step scans the genome once per 2^22 sites, not once per batch); what a batch changes in the file
is data: the pages of the Bowtie step and of RNAfold start again with every batch.  The text leaves the device one
piece at a time (`batches`, `run_to_file`); `run` joins the pieces.
"""
import contextlib

import numpy as np

from .consensus import FOLD_DTYPE, SCAFFOLD, Consensus, read_rnafold_output
from .results import PackedFolds, ResultTable, read_rnafold_text
from .scorer import GuideSet

CONSENSUS_KEYS = ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model", "sgrna_threshold", "low_energy", "high_energy")
SCORE_CHUNK = 1 << 22  # guides per scoring call, and rows of a piece of the file when the run is one batch


def _row_pieces(n, batch_size):
    """The runs of rows the file is written in: the batches, or pieces of SCORE_CHUNK rows of the one batch."""
    step = batch_size if batch_size > 0 else SCORE_CHUNK
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def _fold_pages(fold_rows, n, batch_size, page_length):
    """The non-empty pages of every batch's share of the fold list, as (first, end) in positions of the list."""
    step = batch_size if batch_size > 0 else max(n, 1)
    edges = np.searchsorted(fold_rows, np.arange(0, n + step, step, dtype=np.int64).clip(max=n))
    return [(a, min(a + page_length, int(hi))) for lo, hi in zip(edges, edges[1:]) for a in range(int(lo), int(hi), page_length)]


def _fold(c, config, rnafold):
    """RNAfold's answers for the fold list of c -> (FOLD_DTYPE array, the three texts per row)."""
    guides = c.fold_guides()
    page_length = config.get("rnafold_page_length")
    if page_length is None:
        text = rnafold(c.fold_input())
        return read_rnafold_output(text, guides), read_rnafold_text(text, guides)
    if int(page_length) == 0:
        return np.zeros(len(guides), dtype=FOLD_DTYPE), [None] * len(guides)
    folds, texts = [], []
    for a, b in _fold_pages(c.fold_rows, c.n_guides, int(config.get("batch_size", 0)), int(page_length)):
        text = rnafold("".join(f"G{g[1:20]}{SCAFFOLD}\n" for g in guides[a:b]))
        folds.append(read_rnafold_output(text, guides[a:b]))
        texts += read_rnafold_text(text, guides[a:b])
    return np.concatenate(folds), texts


def _fold_device(c, config, rnafold):
    """The same on the device -> the Folds of c, read: RNAfold's input comes from Folds.input(), its answer goes to
    Folds.read(), one page at a time; the page logic is that of _fold."""
    folds = c.folds()
    try:
        page_length = config.get("rnafold_page_length")
        if page_length is None:
            folds.read(rnafold(folds.input().decode()))
        elif int(page_length) != 0:
            for a, b in _fold_pages(c.fold_rows, c.n_guides, int(config.get("batch_size", 0)), int(page_length)):
                folds.read(rnafold(folds.input(a, b - a).decode()), a, b - a)
    except BaseException:
        folds.close()
        raise
    return folds


def batches(inputs, genome, index, config, rnafold):
    """inputs: the FASTA inputs of GuideSet.extract (bytes blobs or paths); genome: a Genome (the Bowtie step's text) and
    index: an uploaded IsslIndex, both on the device the guides go to, or None when config["offtargetscore"] is false;
    rnafold: a callable that takes RNAfold's input (the lines of Consensus.fold_input(), a str) and returns what RNAfold
    printed, as str or bytes.
    config: a mapping with the keywords of Consensus (CONSENSUS_KEYS) and, all optional,
      offtargetscore  run the Bowtie step and the scoring ([offtargetscore] enabled; default True)
      batch_size      [input] batch-size: the pages of the Bowtie step and of RNAfold start again with every batch of this
                      many guides (absent or 0: one batch)
      page_length     [bowtie2] page-length (0: one page per batch)
      rnafold_page_length   [rnafold] page-length.  Absent: one call of `rnafold` and one table of its answers over the
                      whole fold list.  P > 0: one call per non-empty page of every batch's share of the fold list, with
                      that page's lines, and its answer read with a table of that page alone.  0: the reference's own
                      behaviour, which tests no guide: Paginator.py:29-30 hands out the filter's generator itself, writing
                      RNAfold's input (Crackling.py:420) consumes it, and the loop that reads the answers (:458) sees
                      nothing.  `rnafold` is not called then -- its answer would never be read -- and every row of the
                      fold list keeps '?' in passedSecondaryStructure and the three ss columns
      max_distance, score_threshold, method   [offtargetscore] max-distance (4), score-threshold (75), method ("and")
      rnafold_reader  "device" (the default): RNAfold's input is written and its answers are read on the GPU
                      (crackling_amd.Folds); folds and texts stay there for the consensus and the table.  "host": the Python
                      helpers fold_input, read_rnafold_output and read_rnafold_text.  The two differ in two places.  An answer
                      that holds VT, FF, 0x1c-0x1e or non-ASCII bytes: there the helpers (str.splitlines()) split lines the
                      reference, and the device with it, does not.  And the number in the parentheses: the helpers take
                      what float(x.strip()) takes -- 1e2, inf, 1_0, any count of digits, VT, FF or 0x1c-0x1f around it --
                      where the device takes plain decimals of up to 15 digits with blanks and TABs around them and refuses
                      the rest (IsslError -3 or -4).  RNAfold prints none of these
      delimiter       [output] delimiter (",")
      device          the GPU (0)
    -> a generator of the bytes of the reference's output file for these inputs, in pieces: the header row, then one piece
    per batch (pieces of at most SCORE_CHUNK rows when the run is one batch).  One piece's text is alive at a time, on the
    device and on the host; the stages stay open until the generator is exhausted or closed."""
    import torch
    device = int(config.get("device", 0))
    method = str(config.get("method", "and"))
    threshold = float(config.get("score_threshold", 75.0))
    batch_size = int(config.get("batch_size", 0))
    reader = str(config.get("rnafold_reader", "device"))
    if reader not in ("device", "host"):
        raise ValueError('rnafold_reader: "device" or "host"')
    with GuideSet.extract(inputs, device) as gs, Consensus(gs, **{k: config[k] for k in CONSENSUS_KEYS if k in config}) as c, \
            contextlib.ExitStack() as stack:
        folds_text = device_folds = None
        if c.n_fold and reader == "device":
            device_folds = _fold_device(c, config, rnafold)
            stack.callback(device_folds.close)  # (ahead of the consensus it belongs to)
            c.finish(device_folds)
        elif c.n_fold:
            folds, folds_text = _fold(c, config, rnafold)
            c.finish(folds)
            folds_text = PackedFolds(folds_text)
        else:
            c.finish()
        bowtie = scores = None
        if config.get("offtargetscore", True):
            bowtie = c.bowtie(genome, int(config.get("page_length", 0)), batch_size)
            rows = bowtie.selected_tensor()
            sigs = gs.sigs_tensor()[rows.to(torch.int64)].contiguous()
            mit = torch.empty(sigs.numel(), dtype=torch.float64, device=sigs.device)
            cfd = torch.empty_like(mit)
            stream = torch.cuda.current_stream(sigs.device).cuda_stream
            for a in range(0, sigs.numel(), SCORE_CHUNK):
                b = min(a + SCORE_CHUNK, sigs.numel())
                index.score_device(sigs[a:b], mit[a:b], cfd[a:b], int(config.get("max_distance", 4)), threshold, method, stream=stream)
            scores = (rows, mit, cfd)
        common = (bowtie, scores, config.get("delimiter", ","), method, threshold)
        with ResultTable(c, None, *common, rows=(0, 0)) as table:
            piece = table.to_bytes()
        yield piece
        for a, b in _row_pieces(gs.n_guides, batch_size):
            texts = device_folds
            if folds_text is not None:
                lo, hi = np.searchsorted(c.fold_rows, (a, b))
                texts = folds_text.piece(int(lo), int(hi))
            with ResultTable(c, texts, *common, rows=(a, b - a), header=False) as table:
                piece = table.to_bytes()
            yield piece


def run(inputs, genome, index, config, rnafold):
    """The arguments of `batches` -> the bytes of the reference's output file for these inputs."""
    return b"".join(batches(inputs, genome, index, config, rnafold))


def run_to_file(path, inputs, genome, index, config, rnafold):
    """The same, appended to the file at `path` piece by piece, as the reference, which opens its file with 'a+', adds
    to what is there.  -> the number of bytes written."""
    written = 0
    with open(path, "ab") as out:
        for piece in batches(inputs, genome, index, config, rnafold):
            out.write(piece)
            written += len(piece)
    return written
