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
import os

import numpy as np

from .bowtie import BowtieStep
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
    Folds.read(), one page at a time; the page logic is that of _fold.  An `rnafold` with a method fold_page(folds, first,
    n) is handed the page itself (the driver's: RNAfold's two files are written and read by the library)."""
    folds = c.folds()

    def page(a, n):
        if hasattr(rnafold, "fold_page"):
            rnafold.fold_page(folds, a, n)
        else:
            folds.read(rnafold(folds.input(a, n).decode()), a, n)

    try:
        page_length = config.get("rnafold_page_length")
        if page_length is None:
            page(0, c.n_fold)
        elif int(page_length) != 0:
            for a, b in _fold_pages(c.fold_rows, c.n_guides, int(config.get("batch_size", 0)), int(page_length)):
                page(a, b - a)
    except BaseException:
        folds.close()
        raise
    return folds


def _input_files(inputs):
    """(name, bytes) of every input as GuideSet.extract reads them, for the log: a path stands for itself, a lone
    directory for its top-level files in reverse sorted name order, a blob is 'input <k>'."""
    inputs = list(inputs)
    if not all(isinstance(x, (str, os.PathLike)) for x in inputs):
        return [(f"input {k}", len(x)) for k, x in enumerate(inputs)]
    paths = [os.fspath(x) for x in inputs]
    if len(paths) == 1 and os.path.isdir(paths[0]):
        paths = [os.path.join(paths[0], f) for f in sorted(os.listdir(paths[0]), reverse=True) if os.path.isfile(os.path.join(paths[0], f))]
    return [(p, os.path.getsize(p)) for p in paths]


def _log_inputs(log, gs, inputs):
    """The extraction block of the log (Crackling.py:171-261).  An input without a match stops the reference with a
    ZeroDivisionError at :254, before it has written anything: refused here, by name."""
    files, counts = _input_files(inputs), gs.file_counts
    if len(files) != len(counts):
        raise ValueError(f"{len(files)} inputs, counts of {len(counts)}")
    for (name, _), c in zip(files, counts):
        if int(c[0]) == 0:
            raise ValueError(f"no candidate guide in {name}: the reference stops there (division by zero, Crackling.py:254)")
    log.begin()
    total, done, repeated, distinct = sum(size for _, size in files), 0, 0, 0
    for (name, size), c in zip(files, counts):
        done, repeated, distinct = done + size, repeated + int(c[2]), distinct + int(c[3])
        log.input_file(name, int(c[0]), repeated, int(c[1]), distinct, done / total * 100.0)


def _not_found_guides(c, gs, positions):
    """(position in the fold list, 20-mer) for the positions given, gathered on the device."""
    import ctypes as C
    import torch
    from ._lib import lib, check
    from .scorer import _DeviceArray, decode_guides
    if not len(positions):
        return []
    d_rows, n_fold = C.c_void_p(), C.c_uint64()
    check(lib.issl_consensus_fold_list(c._h, C.byref(d_rows), C.byref(n_fold)))
    fold = torch.as_tensor(_DeviceArray(c, d_rows.value, (n_fold.value,), "<i4"), device=f"cuda:{c.device}")
    at = torch.from_numpy(np.asarray(positions, dtype=np.int64)).to(fold.device)
    sigs = gs.sigs_tensor()[fold[at].to(torch.int64)].cpu().numpy().astype(np.uint64)
    return list(zip((int(p) for p in positions), decode_guides(sigs, 20)))


def batches(inputs, genome, index, config, rnafold, log=None):
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
      offtarget_page_length   [offtargetscore] page-length: read only for `log`, whose off-target block prints one figure per
                      page; no byte of the file depends on it here (absent: 5000000, the reference's own)
    log: None, or a crackling_amd.RunLog: the stages feed it the reference's log -- the extraction block from the counts the
    extraction keeps per input, a batch's blocks from the counts made on the device over the resident rows
    (crackling_amd.runlog.BatchCounts, the Bowtie step's events per page) ahead of the batch's piece.  Needs the device
    reader.  Without it the call does exactly what it did before.
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
    if log is not None and reader != "device":
        raise ValueError("log: needs rnafold_reader 'device'")
    with GuideSet.extract(inputs, device) as gs, Consensus(gs, **{k: config[k] for k in CONSENSUS_KEYS if k in config}) as c, \
            contextlib.ExitStack() as stack:
        if log is not None:
            _log_inputs(log, gs, inputs)
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
            bowtie = BowtieStep(c, genome, int(config.get("page_length", 0)), batch_size, events=log is not None)
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
        counts = None
        if log is not None:
            from .runlog import DEFAULT_PAGE_LENGTH, BatchCounts
            page = config.get("offtarget_page_length")
            counts = BatchCounts(c, device_folds, bowtie, scores, threshold, method, batch_size,
                                 DEFAULT_PAGE_LENGTH if page is None else int(page))
            events = bowtie.batch_events(counts.batches) if bowtie is not None else [0] * len(counts.batches)
            # (under [rnafold] page-length 0 every row is not found and the log prints none of them)
            fold_page = config.get("rnafold_page_length")
            missing = _not_found_guides(c, gs, counts.not_found) if fold_page is None or int(fold_page) > 0 else []
            batch_rows = batch_size if 0 < batch_size < gs.n_guides else 0
        with ResultTable(c, None, *common, rows=(0, 0)) as table:
            piece = table.to_bytes()
        yield piece
        for a, b in _row_pieces(gs.n_guides, batch_size):
            if counts is not None and (batch_rows or a == 0):
                k = a // batch_rows if batch_rows else 0
                row = counts.batches[k]
                log.batch(k, len(counts.batches), row, counts.page_failed[row["page_first"]:row["page_end"]],
                          [m for m in missing if row["fold_first"] <= m[0] < row["fold_end"]], events[k])
            texts = device_folds
            if folds_text is not None:
                lo, hi = np.searchsorted(c.fold_rows, (a, b))
                texts = folds_text.piece(int(lo), int(hi))
            with ResultTable(c, texts, *common, rows=(a, b - a), header=False) as table:
                piece = table.to_bytes()
            yield piece
        if log is not None:
            log.end()


def run(inputs, genome, index, config, rnafold, log=None):
    """The arguments of `batches` -> the bytes of the reference's output file for these inputs."""
    return b"".join(batches(inputs, genome, index, config, rnafold, log=log))


def run_to_file(path, inputs, genome, index, config, rnafold, log=None):
    """The same, appended to the file at `path` piece by piece, as the reference, which opens its file with 'a+', adds
    to what is there.  -> the number of bytes written."""
    written = 0
    with contextlib.ExitStack() as stack:
        # with a log a run can be refused before its first piece (an input without a match) and then leaves no file
        out = None if log is not None else stack.enter_context(open(path, "ab"))
        for piece in batches(inputs, genome, index, config, rnafold, log=log):
            if out is None:
                out = stack.enter_context(open(path, "ab"))
            out.write(piece)
            written += len(piece)
    return written
