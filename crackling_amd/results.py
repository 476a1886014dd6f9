"""Crackling's output file from the resident stages (issl_results_* of include/issl_hip.h): the header row of
Crackling.py:263-268 and one CSV row of the 26 columns of Constants.py:42-70 per candidate guide (:842-852), written on the
GPU from the guide set, the finished consensus, the Bowtie step's rows and the off-target scores where they lie.

`ResultTable(consensus, ...)` builds the text in device memory; `to_bytes()` and `write()` bring it out, `text_tensor()`
and `row_offsets_tensor()` leave it there.  `rows=(first, count)` and `header=False` build a run of rows, so that the text
can leave the device a batch at a time (crackling_amd.pipeline.batches); a row's text does not know its batch -- what
[input] batch-size changes comes in with the Bowtie step's rows and RNAfold's answers.  Five delimiters; no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib, check

COLUMNS = ("seq", "sgrnascorer2score", "header", "start", "end", "strand", "isUnique", "passedG20", "passedTTTT",
           "passedATPercent", "passedSecondaryStructure", "ssL1", "ssStructure", "ssEnergy", "acceptedByMm10db",
           "acceptedBySgRnaScorer", "consensusCount", "passedBowtie", "passedOffTargetScore", "AT", "bowtieChr", "bowtieStart",
           "bowtieEnd", "mitOfftargetscore", "cfdOfftargetscore", "passedAvoidLeadingT")
DELIMITERS = (",", "\t", ";", "|", " ")
TEXT_SPAN_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("reserved", "<u4")])  # issl_text_span
NO_TEXT = 0xFFFFFFFF
DIRECT, NO_SGRNA, NO_HEADER = 1, 2, 4  # ISSL_RESULTS_DIRECT, ISSL_RESULTS_NO_SGRNA, ISSL_RESULTS_NO_HEADER


def read_rnafold_text(text, guides):
    """RNAfold's output as the reference turns it into the columns ssL1, ssStructure and ssEnergy (Crackling.py:439-474)
    -> one entry per guide of `guides` (23-mers or their first 20 characters, in the order of the fold list): None where
    the output has no pair under the guide's key, else (L1, L2.split(' ')[0], L2.split(' ')[1][1:-1]) -- the pair's first
    line, the structure, and what stands between the first and the last character of the word behind it: "( -5.30)"
    splits at its inner blank, so the energy is then the empty string.  Pairs are found as read_rnafold_output finds
    them: filed under characters [1:20] of the first line, U read as T, a later pair replacing an earlier one, a last line
    without partner dropped.  An L2 without a blank raises ValueError (the reference stops with an IndexError there)."""
    pairs = {}
    first = None
    for i, line in enumerate(text.splitlines()):
        if i % 2 == 0:
            first = line.rstrip()
        else:
            pairs[first[1:20].replace("U", "T")] = (first, line.rstrip())
    out = []
    for g in guides:
        pair = pairs.get(g[1:20])
        if pair is None:
            out.append(None)
            continue
        words = pair[1].split(" ")
        if len(words) < 2:
            raise ValueError(f"RNAfold's line for {g[:20]} has no blank between structure and energy: {pair[1]!r}")
        out.append((pair[0], words[0], words[1][1:-1]))
    return out


def _pack_text(folds_text):
    """[(L1, structure, energy) | None] -> (blob bytes, TEXT_SPAN_DTYPE array of three spans per entry)"""
    spans = np.zeros(3 * len(folds_text), dtype=TEXT_SPAN_DTYPE)
    spans["length"] = NO_TEXT
    parts, at = [], 0
    for i, entry in enumerate(folds_text):
        if entry is None:
            continue
        for k, field in enumerate(entry):
            if field is None:
                continue
            b = field if isinstance(field, bytes) else str(field).encode()
            spans[3 * i + k] = (at, len(b), 0)
            parts.append(b)
            at += len(b)
    return b"".join(parts), spans


class PackedFolds:
    """The entries of read_rnafold_text packed once for several tables: ResultTable takes it in place of the list.
    `piece(lo, hi)` keeps the texts of rows [lo, hi) of the fold list only -- the others read as '?', which a table of
    other rows never prints -- so that a table of a run of rows uploads its own texts and no more."""

    def __init__(self, folds_text):
        self.blob, self.spans = _pack_text(folds_text)
        self.n = len(folds_text)

    def __len__(self):
        return self.n

    def piece(self, lo, hi):
        out = PackedFolds.__new__(PackedFolds)
        out.n = self.n
        out.spans = np.zeros(3 * self.n, dtype=TEXT_SPAN_DTYPE)
        out.spans["length"] = NO_TEXT
        part = self.spans[3 * lo:3 * hi].copy()
        have = part["length"] != NO_TEXT
        first = last = 0
        if have.any():  # (the texts lie in the blob in the order of the list)
            first = int(part["offset"][have][0])
            last = int(part["offset"][have][-1]) + int(part["length"][have][-1])
            part["offset"][have] -= np.uint64(first)
        out.spans[3 * lo:3 * hi] = part
        out.blob = self.blob[first:last]
        return out


class ResultTable:
    """The result file of one run, in device memory.
      consensus   a finished Consensus; its guide set gives the rows
      folds_text  read_rnafold_text(text, consensus.fold_guides()): one entry per row of the fold list, or a PackedFolds of
                  them, or the Folds of this consensus, whose texts stay on the device and are quoted there; None: '?'
                  everywhere
      bowtie      the BowtieStep of this consensus, or None: '?' in its four columns
      scores      (rows, mit, cfd) as CUDA tensors: the rows of the guide set that were scored, ascending (int32 or int64),
                  and their float64 scores as the scorer returns them; or None
      delimiter, method, threshold   [output] delimiter, [offtargetscore] method and score-threshold
      rows        None: every row of the set; (first, count): these rows only -- the other arguments stay those of the whole
                  set -- and row k of this table is row first + k of the set
      header      False: the text starts with its first row (row_offsets_tensor()[0] == 0).  The header row, then
                  header=False tables of consecutive runs of rows that cover the set, are the whole table's bytes
    `flags` is for tests and measurements (DIRECT, NO_SGRNA)."""

    def __init__(self, consensus, folds_text=None, bowtie=None, scores=None, delimiter=",", method="and", threshold=75.0, flags=0,
                 rows=None, header=True):
        import torch
        self._h = None
        if not consensus.finished:
            raise ValueError("the consensus is not finished")
        if bowtie is not None and bowtie.consensus is not consensus:
            raise ValueError("the Bowtie step belongs to another consensus")
        if len(delimiter) != 1 or ord(delimiter) > 127:
            raise ValueError("delimiter: one ASCII character")
        gs = consensus.guide_set
        self.device = gs.device
        cfg = _lib.ResultsConfig()
        cfg.delimiter = delimiter.encode()
        cfg.flags = int(flags) | (0 if header else NO_HEADER)
        first_row, n_rows = (0, gs.n_guides) if rows is None else (int(rows[0]), int(rows[1]))
        if first_row < 0 or n_rows < 0:
            raise ValueError("rows: (first, count), neither below 0")
        method_b = str(method).encode()
        cfg.method = method_b
        cfg.threshold = float(threshold)
        blob, spans, n_folds = None, None, 0
        from .folds import Folds
        device_folds = folds_text if isinstance(folds_text, Folds) else None
        if device_folds is not None:
            if device_folds.consensus is not consensus:
                raise ValueError("the folds belong to another consensus")
        elif folds_text is not None:
            if len(folds_text) != consensus.n_fold:
                raise ValueError(f"{len(folds_text)} fold texts for a fold list of {consensus.n_fold}")
            packed = folds_text if isinstance(folds_text, PackedFolds) else PackedFolds(folds_text)
            blob, spans = packed.blob, packed.spans
            n_folds = len(folds_text)
        d_bowtie, n_bowtie, genome = None, 0, None
        if bowtie is not None:
            b_rows = bowtie.rows_tensor()
            d_bowtie, n_bowtie, genome = b_rows.data_ptr() if b_rows.numel() else None, b_rows.shape[0], bowtie.genome._h
            if d_bowtie is None:
                genome = None
        d_scored = d_mit = d_cfd = None
        n_scored = 0
        keep = []
        if scores is not None:
            s_rows, mit, cfd = scores
            s_rows = s_rows.to(device=f"cuda:{self.device}", dtype=torch.int32).contiguous()
            mit = mit.to(device=f"cuda:{self.device}", dtype=torch.float64).contiguous()
            cfd = cfd.to(device=f"cuda:{self.device}", dtype=torch.float64).contiguous()
            if not (s_rows.numel() == mit.numel() == cfd.numel()):
                raise ValueError("scores: rows, mit and cfd of one length")
            keep = [s_rows, mit, cfd]
            n_scored = s_rows.numel()
            if n_scored:
                d_scored, d_mit, d_cfd = s_rows.data_ptr(), mit.data_ptr(), cfd.data_ptr()
        torch.cuda.current_stream(self.device).synchronize()  # the inputs are complete before the library reads them
        h = C.c_void_p()
        args = (gs._h, consensus._h, blob, len(blob) if blob is not None else 0, spans.ctypes.data if spans is not None else None,
                n_folds, d_bowtie, n_bowtie, genome, d_scored, d_mit, d_cfd, n_scored)
        if device_folds is not None:
            check(lib.issl_results_build_rows_folds(gs._h, consensus._h, device_folds._h, *args[6:], first_row, n_rows, C.byref(cfg),
                                                    C.byref(h)))
        elif rows is None and header:
            check(lib.issl_results_build(*args, C.byref(cfg), C.byref(h)))
        else:
            check(lib.issl_results_build_rows(*args, first_row, n_rows, C.byref(cfg), C.byref(h)))
        del keep
        self._h = h
        n_rows, n_bytes, per_group = C.c_uint64(), C.c_uint64(), C.c_uint32()  # (of the table: the rows asked for)
        check(lib.issl_results_info(self._h, C.byref(n_rows), C.byref(n_bytes), C.byref(per_group)))
        self.n_rows, self.n_bytes, self.rows_per_group = n_rows.value, n_bytes.value, per_group.value
        self.first_row = first_row

    def _device(self):
        d_text, d_off = C.c_void_p(), C.c_void_p()
        check(lib.issl_results_device(self._h, C.byref(d_text), C.byref(d_off)))
        return d_text.value, d_off.value

    def text_tensor(self):
        """uint8 CUDA tensor over the text in device memory (n_bytes): no copy; the tensor keeps this object alive."""
        import torch
        from .scorer import _DeviceArray
        return torch.as_tensor(_DeviceArray(self, self._device()[0], (self.n_bytes,), "|u1"), device=f"cuda:{self.device}")

    def row_offsets_tensor(self):
        """int64 CUDA tensor of n_rows + 1 offsets: row k is text[offsets[k]:offsets[k + 1]], offsets[0] is the length of
        the header row (0 without one)."""
        import torch
        from .scorer import _DeviceArray
        return torch.as_tensor(_DeviceArray(self, self._device()[1], (self.n_rows + 1,), "<i8"), device=f"cuda:{self.device}")

    def times(self):
        """Device time of the build's launches in ms (HIP events): {"measure", "scan", "emit"}."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(lib.issl_results_times(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"measure": a.value, "scan": b.value, "emit": c.value}

    def to_bytes(self):
        """The whole file as bytes."""
        out = C.create_string_buffer(max(self.n_bytes, 1))
        check(lib.issl_results_copy(self._h, out, self.n_bytes))
        return out.raw[:self.n_bytes]

    def write(self, path, append=False):
        """Write the file; append=True adds to what is there, as the reference (which opens its file 'a+') does."""
        check(lib.issl_results_write(self._h, os.fsencode(path), 1 if append else 0))

    def close(self):
        if self._h:
            lib.issl_results_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def repr_f64(tensor):
    """repr() of every double of a float64 CUDA tensor, formatted on the device -> list of bytes."""
    import torch
    t = tensor.to(dtype=torch.float64).contiguous().flatten()
    n = t.numel()
    if n == 0:
        return []
    text = torch.empty((n, 32), dtype=torch.uint8, device=t.device)
    lens = torch.empty(n, dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.issl_repr_f64_device(t.data_ptr(), n, text.data_ptr(), lens.data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)))
    raw = text.cpu().numpy().tobytes()
    return [raw[32 * i:32 * i + k] for i, k in enumerate(lens.cpu().numpy().tolist())]
