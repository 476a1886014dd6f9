"""RNAfold's exchange on the device (issl_folds_* of include/issl_hip.h): Crackling.py:406-497 around the RNAfold program.

`Consensus.folds()` gives a `Folds`: `input()` / `write_input()` are RNAfold's input for a run of the fold list, written on
the GPU from the resident guides; `read()` / `read_file()` take what RNAfold printed for that run -- one page -- and leave
one fold and the three texts ssL1, ssStructure, ssEnergy per row in device memory, where `Consensus.finish(folds)` and
`ResultTable(folds_text=folds)` read them.  RNAfold itself is not part of the package.
"""
import ctypes as C
import os

import numpy as np

from ._lib import lib, check
from .consensus import FOLD_DTYPE
from .results import NO_TEXT, TEXT_SPAN_DTYPE

LINE_BYTES = 101  # 'G' + guide[1:20] + the scaffold + LF


class Folds:
    """RNAfold's answers for the fold list of one Consensus, which must stay open while this object is.
      input(first, n) -> bytes      the lines for rows [first, first + n) of the fold list (n None: to its end)
      read(text, first, n)          one page: RNAfold's output (str or bytes) for these rows, read with a dictionary of its
                                    own as the reference reads a page; a row is read once
      folds, spans, texts()         the result on the host, for tests; the pipeline leaves it on the device"""

    def __init__(self, consensus):
        self._h = None
        self.consensus = consensus
        self.device = consensus.device
        h = C.c_void_p()
        check(lib.issl_folds_open(consensus._h, C.byref(h)))
        self._h = h
        self.n_fold = consensus.n_fold
        self.bytes_per_group = self._info()[3]

    def __len__(self):
        return self.n_fold

    def _info(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(lib.issl_folds_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    @property
    def n_read(self):
        return self._info()[1]

    @property
    def text_bytes(self):
        return self._info()[2]

    def _range(self, first, n):
        first = int(first)
        return first, (self.n_fold - first if n is None else int(n))

    def input(self, first=0, n=None):
        first, n = self._range(first, n)
        if first < 0 or n < 0:
            raise ValueError("first and n: neither below 0")
        if first > self.n_fold or n > self.n_fold - first:
            check(lib.issl_folds_input_copy(self._h, first, n, None, 0))  # (the library's words for a range outside the list)
        out = C.create_string_buffer(max(n * LINE_BYTES, 1))
        check(lib.issl_folds_input_copy(self._h, first, n, out, n * LINE_BYTES))
        return out.raw[:n * LINE_BYTES]

    def write_input(self, path, first=0, n=None):
        first, n = self._range(first, n)
        check(lib.issl_folds_input_write(self._h, first, n, os.fsencode(path)))

    def read(self, text, first=0, n=None):
        first, n = self._range(first, n)
        data = text.encode() if isinstance(text, str) else bytes(text)
        check(lib.issl_folds_read(self._h, first, n, data, len(data)))
        return self

    def read_file(self, path, first=0, n=None):
        first, n = self._range(first, n)
        check(lib.issl_folds_read_file(self._h, first, n, os.fsencode(path)))
        return self

    def times(self):
        """Device time of the last input and the last read in ms (HIP events): {"input", "read"}."""
        a, b = C.c_double(), C.c_double()
        check(lib.issl_folds_times(self._h, C.byref(a), C.byref(b)))
        return {"input": a.value, "read": b.value}

    @property
    def folds(self):
        """FOLD_DTYPE array, one entry per row of the fold list (copied from the device)."""
        out = np.zeros(self.n_fold, dtype=FOLD_DTYPE)
        check(lib.issl_folds_copy(self._h, out.ctypes.data if self.n_fold else None, None, self.n_fold))
        return out

    @property
    def spans(self):
        """TEXT_SPAN_DTYPE array, three per row of the fold list, offsets into the pages' text on the device."""
        out = np.zeros(3 * self.n_fold, dtype=TEXT_SPAN_DTYPE)
        check(lib.issl_folds_copy(self._h, None, out.ctypes.data if self.n_fold else None, self.n_fold))
        return out

    def text(self):
        """The pages' text as it lies on the device (every page at a multiple of 16, padded) -> bytes."""
        import torch
        from .scorer import _DeviceArray
        d_text, n = C.c_void_p(), C.c_uint64()
        check(lib.issl_folds_text_device(self._h, C.byref(d_text), C.byref(n)))
        if not n.value:
            return b""
        t = torch.as_tensor(_DeviceArray(self, d_text.value, (n.value,), "|u1"), device=f"cuda:{self.device}")
        return t.cpu().numpy().tobytes()

    def texts(self):
        """One entry per row of the fold list: None, or (ssL1, ssStructure, ssEnergy) as str, byte for byte (latin-1)."""
        spans, blob = self.spans, self.text()
        at, n = spans["offset"].tolist(), spans["length"].tolist()
        cut = [None if k == NO_TEXT else blob[a:a + k].decode("latin-1") for a, k in zip(at, n)]
        rows = zip(cut[0::3], cut[1::3], cut[2::3])
        return [None if r == (None, None, None) else r for r in rows]

    def text_of(self, row, which):
        """Column `which` (0, 1, 2) of one row through issl_folds_text_copy -> bytes, or None without text."""
        if not 0 <= int(row) < self.n_fold or int(which) not in (0, 1, 2):
            raise ValueError("row: one of the fold list; which: 0, 1 or 2")
        length = int(self.spans[3 * int(row) + int(which)]["length"])
        if length == NO_TEXT:
            return None
        n = C.c_size_t()
        buf = C.create_string_buffer(max(length, 1))  # (as long as the span says, whatever that is)
        check(lib.issl_folds_text_copy(self._h, int(row), int(which), buf, length, C.byref(n)))
        return buf.raw[:n.value]

    def close(self):
        if self._h:
            lib.issl_folds_close(self._h)
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
