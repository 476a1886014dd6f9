"""Efficiency consensus on a resident guide set (issl_consensus_* of include/issl_hip.h): Crackling.py:306-598.

`GuideSet.consensus(config)` runs G20 and the mm10db sequence filters on the device and returns a `Consensus` that names
the guides RNAfold has to fold; `Consensus.finish(folds)` takes RNAfold's answers back, scores the guides with the
sgRNAScorer2 model, counts the consensus and selects the rows for the specificity stage.  RNAfold itself is not part of
the package: `fold_input()` is its input, `read_rnafold_output()` reads what it printed.
"""
import ctypes as C
import re

import numpy as np

from . import _lib
from ._lib import lib, check

OPTIMISATIONS = {"ultralow": 0, "low": 1, "medium": 2, "high": 3}
# issl_consensus_row (32 bytes) and issl_fold (16 bytes)
CONSENSUS_DTYPE = np.dtype([("sgrna_score", "<f8"), ("at", "<f8"), ("ss_energy", "<f8"), ("g20", "u1"), ("lead_t", "u1"),
                            ("at_pct", "u1"), ("tttt", "u1"), ("ss", "u1"), ("mm10db", "u1"), ("sgrna", "u1"), ("count", "u1")])
FOLD_DTYPE = np.dtype([("energy", "<f8"), ("scaffold", "<u4"), ("present", "<u4")])
CODES = "01?!"  # the reference's characters for the codes 0..3 of a row
# The sgRNA scaffold RNAfold folds every guide with (mm10db), and how its fold looks in dot-bracket notation when the guide
# leaves it alone: 28 free characters (the guide and the start of the scaffold), two fixed stretches around 21 free ones.
SCAFFOLD = "GUUUUAGAGCUAGAAAUAGCAAGUUAAAAUAAGGCUAGUCCGUUAUCAACUUGAAAAAGUGGCACCGAGUCGGUGCUUUU"
_SCAFFOLD_FOLD = re.compile(".{28}" + re.escape("((((....))))...))))") + ".{21}" +
                            re.escape("((((....))))(((((((...)))))))...") + r"\s\((.+)\)")
_ENERGY = re.compile(r"\s\((.+)\)")


def load_sgrnascorer2(path):
    """The sgRNAScorer2 model file (a joblib dump of a linear-kernel sklearn SVC) -> (sv uint8 [n_sv, 80], coef float64
    [n_sv], intercept float): support_vectors_, _dual_coef_[0] and _intercept_[0]."""
    import joblib
    clf = joblib.load(path)
    sv = clf.support_vectors_
    sv = np.asarray(sv.toarray() if hasattr(sv, "toarray") else sv, dtype=np.float64)
    if getattr(clf, "kernel", "linear") != "linear" or sv.ndim != 2 or sv.shape[1] != 80:
        raise ValueError("not a linear-kernel model over 80 inputs")
    if not np.all((sv == 0) | (sv == 1)):
        raise ValueError("a support vector has an entry other than 0 or 1")
    dual = np.asarray(clf._dual_coef_.toarray() if hasattr(clf._dual_coef_, "toarray") else clf._dual_coef_, dtype=np.float64)
    return sv.astype(np.uint8), np.ascontiguousarray(dual[0]), float(np.asarray(clf._intercept_, dtype=np.float64)[0])


def read_rnafold_output(text, guides):
    """RNAfold's output as the reference reads it (Crackling.py:439-470, :481-497) -> FOLD_DTYPE array, one entry per guide
    of `guides` (23-mers or their first 20 characters, in the order of the fold list).  The lines come in pairs, the
    sequence and its structure with the energy; a pair is filed under characters [1:20] of its sequence, U read as T, and a
    later pair replaces an earlier one with the same key; a last line without partner is dropped.  A guide looks its pair
    up under guide[1:20]: none -> present = 0.  scaffold = 1 when the structure line matches the fold of the scaffold;
    energy = the number in the parentheses behind the structure, blanks around it allowed."""
    pairs = {}
    first = None
    for i, line in enumerate(text.splitlines()):
        if i % 2 == 0:
            first = line.rstrip()
        else:
            pairs[first[1:20].replace("U", "T")] = line.rstrip()
    out = np.zeros(len(guides), dtype=FOLD_DTYPE)
    for k, g in enumerate(guides):
        second = pairs.get(g[1:20])
        if second is None:
            continue
        m = _SCAFFOLD_FOLD.search(second)
        e = m or _ENERGY.search(second)
        if not e:
            continue  # (the reference leaves such a guide untested)
        out[k] = (float(e.group(1).strip()), 1 if m else 0, 1)
    return out


class Consensus:
    """One run of the efficiency consensus over a GuideSet.  After the constructor: `fold_rows`, `fold_input()`.  After
    `finish(folds)`: `rows`, `selected`, `selected_tensor()`.  The guide set must stay open while this object is."""

    def __init__(self, guide_set, optimisation="high", n=2, mm10db=True, chopchop=True, sgrnascorer2=True, model=None,
                 sgrna_threshold=0.0, low_energy=-30.0, high_energy=-18.0):
        self._h = None
        self.guide_set = guide_set
        cfg = _lib.ConsensusConfig()
        cfg.optimisation = OPTIMISATIONS[optimisation.lower()] if isinstance(optimisation, str) else int(optimisation)
        cfg.n = int(n)
        self.optimisation = cfg.optimisation
        cfg.mm10db, cfg.chopchop, cfg.sgrnascorer2 = int(bool(mm10db)), int(bool(chopchop)), int(bool(sgrnascorer2))
        keep = []
        if model is not None:
            sv, coef, intercept = model
            sv = np.ascontiguousarray(sv, dtype=np.uint8)
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            if sv.ndim != 2 or sv.shape[1] != 80 or coef.shape != (sv.shape[0],):
                raise ValueError("model: (sv [n_sv, 80], coef [n_sv], intercept)")
            cfg.n_sv, cfg.sv, cfg.coef, cfg.intercept = sv.shape[0], sv.ctypes.data, coef.ctypes.data, float(intercept)
            keep = [sv, coef]
        cfg.sgrna_threshold, cfg.low_energy, cfg.high_energy = float(sgrna_threshold), float(low_energy), float(high_energy)
        h = C.c_void_p()
        check(lib.issl_consensus_begin(guide_set._h, C.byref(cfg), C.byref(h)))
        del keep
        self._h = h
        self.n_guides = guide_set.n_guides
        self.device = guide_set.device
        d_rows, n_fold = C.c_void_p(), C.c_uint64()
        check(lib.issl_consensus_fold_list(self._h, C.byref(d_rows), C.byref(n_fold)))
        self.n_fold = n_fold.value
        self.finished = False
        self._fold_rows = self._rows = self._selected = None

    @property
    def fold_rows(self):
        """uint32 array: the rows of the set RNAfold has to fold, ascending (Crackling.py:406-422)."""
        if self._fold_rows is None:
            out = np.empty(self.n_fold, dtype=np.uint32)
            check(lib.issl_consensus_fold_copy(self._h, out.ctypes.data, len(out)))
            self._fold_rows = out
        return self._fold_rows

    def fold_guides(self):
        """The 23-mers of the fold list."""
        from .scorer import decode_guides
        return decode_guides(self.guide_set.guides["guide23"][self.fold_rows], 23)

    def fold_input(self):
        """The lines the reference hands RNAfold (Crackling.py:421), one per row of the fold list."""
        return "".join(f"G{g[1:20]}{SCAFFOLD}\n" for g in self.fold_guides())

    def folds(self):
        """A crackling_amd.Folds for this consensus: RNAfold's input written and its answers read on the device."""
        from .folds import Folds
        return Folds(self)

    def finish(self, folds=None):
        """folds: FOLD_DTYPE array aligned with fold_rows (read_rnafold_output(text, self.fold_guides())), or the Folds of
        this consensus, whose rows are taken where they lie on the device; None when the fold list is empty.  Once."""
        from .folds import Folds
        if isinstance(folds, Folds):
            check(lib.issl_consensus_finish_folds(self._h, folds._h))
        elif folds is None:
            check(lib.issl_consensus_finish(self._h, None, 0))
        else:
            folds = np.ascontiguousarray(folds, dtype=FOLD_DTYPE)
            check(lib.issl_consensus_finish(self._h, folds.ctypes.data if len(folds) else None, len(folds)))
        self.finished = True
        return self

    def _device(self):
        d_rows, d_sel, n_sel = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.issl_consensus_device(self._h, C.byref(d_rows), C.byref(d_sel), C.byref(n_sel)))
        return d_rows.value, d_sel.value, n_sel.value

    @property
    def rows(self):
        """Structured array (CONSENSUS_DTYPE), one row per guide of the set; copied from the device once."""
        if self._rows is None:
            out = np.empty(self.n_guides, dtype=CONSENSUS_DTYPE)
            check(lib.issl_consensus_copy(self._h, out.ctypes.data, len(out)))
            self._rows = out
        return self._rows

    @property
    def n_selected(self):
        return self._device()[2]

    def selected_tensor(self):
        """int32 CUDA tensor over the selection in device memory: the rows the reference's filter yields for the specificity
        stage, ascending (rows are below 2^31: a set holds at most 2^32 - 1 matches of 40 bytes each).  No copy; the tensor
        keeps this object alive, and close() must not be called while it is in use."""
        import torch
        from .scorer import _DeviceArray
        _, d_sel, n_sel = self._device()
        if not n_sel:
            return torch.empty(0, dtype=torch.int32, device=f"cuda:{self.device}")
        return torch.as_tensor(_DeviceArray(self, d_sel, (n_sel,), "<i4"), device=f"cuda:{self.device}")

    @property
    def selected(self):
        """The selection as a uint32 numpy array."""
        if self._selected is None:
            self._selected = self.selected_tensor().cpu().numpy().astype(np.uint32)
        return self._selected

    def selection_pages(self, batch_size, page_length):
        """The reference's pages of the Bowtie step for a run in batches of batch_size rows of the set ([input] batch-size;
        0: one batch) with [bowtie2] page-length page_length (0: one page per batch): int64 CUDA tensor of n_pages + 1
        boundaries in positions of the selection, made on the device.  The tensor is valid until the next call or close()."""
        import torch
        from .scorer import _DeviceArray
        d_starts, n_pages = C.c_void_p(), C.c_uint64()
        check(lib.issl_consensus_selection_pages(self._h, int(batch_size), int(page_length), C.byref(d_starts), C.byref(n_pages)))
        return torch.as_tensor(_DeviceArray(self, d_starts.value, (n_pages.value + 1,), "<i8"), device=f"cuda:{self.device}")

    def bowtie(self, genome, page_length=0, batch_size=0):
        """The Bowtie step (Crackling.py:600-725) over the selection of this finished consensus, on `genome` (a
        crackling_amd.Genome on the same device) -> BowtieStep.  batch_size: [input] batch-size, the pages start again
        with every batch of that many rows of the set (0: one batch)."""
        from .bowtie import BowtieStep
        return BowtieStep(self, genome, page_length, batch_size)

    def close(self):
        if self._h:
            lib.issl_consensus_close(self._h)
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
