"""Transcript hit counts (issl_annotation_* of include/issl_hip.h): src/crackling/utils/countHitTranscripts.py.

The reference appends a `hits` column to Crackling's output: of the transcripts of the gene a guide lies in, how many have
an exon that contains the guide's `bowtieStart`.  `Annotation` resolves a GFF3 annotation into one answer per elementary
segment on the GPU when it is opened; `hits` / `hits_device` then answer any (sequence, start), the rows of
`Genome.locate` -- off-target sites -- as well as the guides' own places; `BowtieStep.transcripts(annotation)` answers the
rows of the Bowtie step where they lie, in device memory.
"""
import ctypes as C
import os

import numpy as np

from ._lib import check, lib

TRANSCRIPT_HITS_DTYPE = np.dtype([("hit", "<u4"), ("total", "<u4"), ("status", "<u4"), ("first", "<u4")])
assert TRANSCRIPT_HITS_DTYPE.itemsize == 16
NO_SEQ = 0xFFFFFFFF


def format_hits(rows):
    """TRANSCRIPT_HITS_DTYPE rows -> the reference's `hits` strings: "<hit>/<total>", "?/?" for a status other than 0."""
    return [f"{int(r['hit'])}/{int(r['total'])}" if r["status"] == 0 else "?/?" for r in rows]


class Annotation:
    """A GFF3 annotation resolved on the GPU: the breakpoints of every sequence and one answer per segment."""

    def __init__(self, handle):
        self._h = handle
        n = [C.c_uint64() for _ in range(5)]
        check(lib.issl_annotation_info(self._h, *[C.byref(x) for x in n]))
        self.info = dict(zip(("n_seqs", "n_transcripts", "n_genes", "n_exons", "n_segments"), (x.value for x in n)))
        self.seqs = []
        name, name_len = C.c_void_p(), C.c_size_t()
        for k in range(self.info["n_seqs"]):
            check(lib.issl_annotation_seq(self._h, k, C.byref(name), C.byref(name_len)))
            self.seqs.append(C.string_at(name, name_len.value) if name_len.value else b"")

    @classmethod
    def open(cls, path_or_bytes, device=0):
        """path_or_bytes: the GFF3 text (bytes) or a path to it (str / os.PathLike)."""
        h = C.c_void_p()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            blob = bytes(path_or_bytes)
            check(lib.issl_annotation_open(blob, len(blob), device, C.byref(h)))
        elif isinstance(path_or_bytes, (str, os.PathLike)):
            check(lib.issl_annotation_open_file(os.fsencode(path_or_bytes), device, C.byref(h)))
        else:
            raise TypeError("path_or_bytes: the GFF3 text as bytes, or a path")
        return cls(h)

    def lookup(self, name):
        """Index of the sequence a query names (str or bytes, taken as it stands), NO_SEQ when the annotation lacks it."""
        raw = name.encode() if isinstance(name, str) else bytes(name)
        seq = C.c_uint32()
        check(lib.issl_annotation_lookup(self._h, raw, len(raw), C.byref(seq)))
        return seq.value

    def hits(self, names, starts):
        """names: one sequence name per query (bowtieChr; str or bytes), or a uint32 array of indices from lookup();
        starts: bowtieStart.  -> TRANSCRIPT_HITS_DTYPE array, one row per query."""
        if isinstance(names, np.ndarray) and names.dtype.kind in "ui":
            seq = np.ascontiguousarray(names, dtype=np.uint32)
        else:
            known = {}
            seq = np.fromiter((known[n] if n in known else known.setdefault(n, self.lookup(n)) for n in names), dtype=np.uint32)
        start = np.ascontiguousarray(starts, dtype=np.int64)
        if len(seq) != len(start):
            raise ValueError("names and starts differ in length")
        out = np.zeros(len(seq), dtype=TRANSCRIPT_HITS_DTYPE)
        if len(seq):
            check(lib.issl_annotation_hits(self._h, seq.ctypes.data, start.ctypes.data, len(seq), out.ctypes.data))
        return out

    def hits_device(self, d_seq, d_start, d_out, stream=None):
        """d_seq: int32 CUDA tensor of sequence indices (-1: absent); d_start: int64 CUDA tensor; d_out: uint8 CUDA tensor of
        16 bytes per query (TRANSCRIPT_HITS_DTYPE).  Enqueued on `stream`; the call does not wait."""
        n = d_seq.numel()
        if d_seq.element_size() != 4 or d_start.element_size() != 8 or d_start.numel() != n:
            raise ValueError("d_seq: 32-bit indices, d_start: as many 64-bit starts")
        if d_out.numel() * d_out.element_size() < TRANSCRIPT_HITS_DTYPE.itemsize * n:
            raise ValueError("d_out holds fewer than 16 bytes per query")
        check(lib.issl_annotation_hits_device(self._h, d_seq.data_ptr() if n else None, d_start.data_ptr() if n else None, n,
                                              d_out.data_ptr() if n else None, C.c_void_p(stream) if stream else None))

    def hits_occurrences_device(self, genome, d_rows, d_out, stream=None):
        """d_rows: uint8 CUDA tensor [n, 32] of OCCURRENCE_DTYPE rows on `genome`; d_out: 16 bytes per row."""
        n = d_rows.numel() * d_rows.element_size() // 32
        if d_out.numel() * d_out.element_size() < TRANSCRIPT_HITS_DTYPE.itemsize * n:
            raise ValueError("d_out holds fewer than 16 bytes per row")
        check(lib.issl_annotation_hits_occurrences_device(self._h, genome._h, d_rows.data_ptr() if n else None, n,
                                                          d_out.data_ptr() if n else None, C.c_void_p(stream) if stream else None))

    def close(self):
        if self._h:
            lib.issl_annotation_close(self._h)
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


class TranscriptHits:
    """The answers for the rows of a BowtieStep (BowtieStep.transcripts), left in device memory."""

    def __init__(self, step, annotation):
        import torch
        d_rows = step.rows_tensor()
        self._d_out = torch.empty((d_rows.shape[0], TRANSCRIPT_HITS_DTYPE.itemsize), dtype=torch.uint8, device=d_rows.device)
        annotation.hits_occurrences_device(step.genome, d_rows, self._d_out,
                                           stream=torch.cuda.current_stream(d_rows.device).cuda_stream)
        self._rows = None

    def rows_tensor(self):
        """uint8 CUDA tensor [n_selected, 16]: the answers in device memory."""
        return self._d_out

    @property
    def rows(self):
        if self._rows is None:
            self._rows = self._d_out.cpu().numpy().view(TRANSCRIPT_HITS_DTYPE).reshape(-1)
        return self._rows

    def column(self):
        """The reference's `hits` column for the rows of the step."""
        return format_hits(self.rows)
