"""The run's log: what every batch's stages saw and failed (issl_runlog_* of include/issl_hip.h), and the text the
reference makes of it (Crackling.py:171-261, :276-305 and the printer calls of :305-888).

`BatchCounts` counts on the device, over the rows the stages left there: per batch the figures of every efficiency test,
the batch's share of the fold list, of the selection and of the scored rows, and per page of [offtargetscore] page-length
the rows the method and threshold reject.  Two figures of the log are no counts over finished rows and are not made
here: the Bowtie step's `failed` (Crackling.py:709-717 counts events: a site named reject, accept, reject counts twice)
and the per-file duplicate figures of the extraction (:254-258).  `RunLog` takes them from its caller.

`RunLog` writes the reference's lines: every message as '>>> <timestamp>:\\t<message>\\n' and an empty line
(Helpers.py:31-35), in the reference's order, a stage's block only when its tool is switched on, the page lines by
Paginator.py's rules.  Differences, stated: the '| Calling:' and '| Finished' lines of Helpers.runner and the line
'Batchinator is writing to:' are not written; the stages here run whole-set, so a batch's lines are written when its
counts are known and their timestamps say when the line was written.

Two things the reference does with a page length of 0 are kept, since the log is the reference's: Paginator.py:29-30 hands
out the filter's generator itself, the loop that writes a stage's input consumes it, and the loop that reads the answers
sees nothing.  So with [rnafold] page-length = 0 the block prints the fold list's length as the page's guides and then
'0 of 0 failed here.', and with [offtargetscore] page-length = 0 it prints '0 of <n> failed here.' whatever the scores
are (`BatchCounts.page_failed` still holds the real count of the one page).
"""
import ctypes as C
import datetime
import time

import numpy as np

from ._lib import lib, check

# issl_runlog_batch: 28 words
BATCH_FIELDS = ("loaded", "g20_tested", "g20_failed", "lead_t_tested", "lead_t_failed", "at_tested", "at_failed", "tttt_tested",
                "tttt_failed", "ss_tested", "ss_failed", "ss_erred", "ss_not_found", "mm10db_accepted", "mm10db_failed",
                "sgrna_tested", "sgrna_failed", "consensus_tested", "consensus_failed", "fold_first", "fold_end", "selected_first",
                "selected_end", "scored_first", "scored_end", "page_first", "page_end", "bowtie_rejected")
BATCH_DTYPE = np.dtype([(f, "<u4") for f in BATCH_FIELDS])
assert BATCH_DTYPE.itemsize == 112
DEFAULT_PAGE_LENGTH = 5000000  # the three page lengths of the reference's config.ini


class BatchCounts:
    """issl_runlog_batches over a finished Consensus.  folds: the Folds of the consensus, or None (a row of the fold list
    the consensus left untested then counts as not found); bowtie: its BowtieStep, or None; scores: (rows, mit, cfd) --
    CUDA tensors: the int32 rows of the set that were scored, ascending, and their float64 scores -- or None.  The tensors
    must be complete on their stream's side: the current stream of their device is synchronised here.
    -> `batches` (BATCH_DTYPE, one per batch), `page_failed` (uint32, one per off-target page; a batch's pages are
    [page_first, page_end)), `not_found` (uint32 positions in the fold list, ascending), `ms` (device time of the counting)."""

    def __init__(self, consensus, folds=None, bowtie=None, scores=None, threshold=75.0, method="and", batch_size=0,
                 offtarget_page_length=0):
        import torch
        if not consensus.finished:
            raise ValueError("the consensus is not finished")
        d_bowtie, n_bowtie = None, 0
        if bowtie is not None:
            rows = bowtie.rows_tensor()
            d_bowtie, n_bowtie = rows.data_ptr() if rows.shape[0] else None, rows.shape[0]
        d_scored = d_mit = d_cfd = None
        n_scored = 0
        keep = None
        if scores is not None:
            rows, mit, cfd = scores
            rows, mit, cfd = rows.to(torch.int32).contiguous(), mit.to(torch.float64).contiguous(), cfd.to(torch.float64).contiguous()
            if not (rows.numel() == mit.numel() == cfd.numel()):
                raise ValueError("scores: rows, mit and cfd of one length")
            keep = (rows, mit, cfd)
            n_scored = rows.numel()
            if n_scored:
                d_scored, d_mit, d_cfd = rows.data_ptr(), mit.data_ptr(), cfd.data_ptr()
        torch.cuda.current_stream(consensus.device).synchronize()
        h = C.c_void_p()
        check(lib.issl_runlog_batches(consensus._h, folds._h if folds is not None else None, d_bowtie, n_bowtie, d_scored, d_mit,
                                      d_cfd, n_scored, float(threshold), str(method).encode(), int(batch_size),
                                      int(offtarget_page_length), C.byref(h)))
        del keep
        try:
            n_batches, n_pages, n_not_found, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
            check(lib.issl_runlog_info(h, C.byref(n_batches), C.byref(n_pages), C.byref(n_not_found), C.byref(ms)))
            self.batches = np.zeros(n_batches.value, dtype=BATCH_DTYPE)
            self.page_failed = np.zeros(n_pages.value, dtype=np.uint32)
            self.not_found = np.zeros(n_not_found.value, dtype=np.uint32)
            self.ms = ms.value
            check(lib.issl_runlog_copy(h, self.batches.ctypes.data, len(self.batches), self.page_failed.ctypes.data,
                                       len(self.page_failed), self.not_found.ctypes.data, len(self.not_found)))
        finally:
            lib.issl_runlog_close(h)
        self.batch_size = int(batch_size)
        self.offtarget_page_length = int(offtarget_page_length)


def _pages(first, end, page_length):
    """Paginator.py over positions [first, end): page lengths.  0: exactly one page, also for an empty share."""
    if page_length <= 0:
        return [end - first]
    return [min(page_length, end - a) for a in range(first, end, page_length)]


def _elapsed(seconds):
    return time.strftime("%d %H:%M:%S", time.gmtime(seconds)), seconds


class RunLog:
    """The reference's log as text.  config: the mapping crackling_amd.pipeline.batches takes -- read here: mm10db, chopchop,
    sgrnascorer2 (the tools, default True), offtargetscore (True), page_length ([bowtie2] page-length, 0),
    rnafold_page_length and offtarget_page_length ([rnafold] and [offtargetscore] page-length; absent or None: 5000000, the
    reference's own).  out: a text file to write every line to as it is made, or None; `text()` is everything so far."""

    def __init__(self, config, out=None):
        self.config = dict(config)
        self.out = out
        self.parts = []
        self.started = time.time()

    def _page_length(self, key):
        v = self.config.get(key)
        return DEFAULT_PAGE_LENGTH if v is None else int(v)

    def bare(self, line):
        """A line as print() leaves it."""
        self.parts.append(line + "\n")
        if self.out is not None:
            self.out.write(self.parts[-1])
            self.out.flush()

    def say(self, message):
        """Helpers.printer."""
        self.bare(">>> {}:\t{}\n".format(datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S:%f"), message))

    def text(self):
        return "".join(self.parts)

    def begin(self):
        self.say("Analysing files...")

    def input_file(self, path, identified, repeated, duplicates, distinct, completed_percent):
        """Crackling.py:187, :254-261 for one input.  identified: its matches; duplicates: those of them that met a guide
        seen before; repeated: distinct guides seen twice or more so far; distinct: distinct guides so far."""
        self.say(f"Identifying possible target sites in: {path}")
        percent = round(duplicates / identified * 100.0, 3)
        self.say(f"\tIdentified {identified:,} possible target sites in this file.")
        self.say(f"\tOf these, {repeated:,} are not unique. These sites occur a total of {duplicates} times.")
        self.say(f"\tRemoving {duplicates:,} of {identified:,} ({percent}%) guides.")
        self.say(f"\t{distinct:,} distinct guides have been discovered so far.")
        self.say(f"\tExtracted from {round(completed_percent, 3)}% of input")

    def batch(self, index, n_batches, counts, page_failed=(), not_found=(), bowtie_failed=0, seconds=0.0):
        """The lines of batch `index` (0-based) of n_batches.  counts: its BATCH_DTYPE entry; page_failed: the figures of its
        off-target pages; not_found: (position in the fold list, 20-mer) of its fold-list rows RNAfold did not answer,
        ascending; bowtie_failed: the Bowtie step's events of its pages."""
        c = {f: int(counts[f]) for f in BATCH_FIELDS}
        cfg = self.config
        self.say(f"Processing batch file {index + 1:,} of {n_batches}")
        self.say(f"\tLoaded {c['loaded']:,} guides")
        if cfg.get("chopchop", True):
            self.say("CHOPCHOP - remove those without G in position 20.")
            self.say(f"\t{c['g20_failed']:,} of {c['g20_tested']:,} failed here.")
        if cfg.get("mm10db", True):
            for title, f in (("mm10db - remove all targets with a leading T (+) or trailing A (-).", "lead_t"),
                             ("mm10db - remove based on AT percent.", "at"), ("mm10db - remove all targets that contain TTTT.", "tttt")):
                self.say(title)
                self.say(f"\t{c[f + '_failed']:,} of {c[f + '_tested']:,} failed here.")
            self._secondary_structure(c, list(not_found))
            self.say("Calculating mm10db final result.")
            self.say(f"\t{c['mm10db_accepted']} accepted.")
            self.say(f"\t{c['mm10db_failed']} failed.")
        if cfg.get("sgrnascorer2", True):
            self.say("sgRNAScorer2 - score using model.")
            self.say(f"\t{c['sgrna_failed']:,} of {c['sgrna_tested']:,} failed here.")
        self.say("Evaluating efficiency via consensus approach.")
        self.say(f"\t{c['consensus_failed']:,} of {c['consensus_tested']:,} failed here.")
        if cfg.get("offtargetscore", True):
            self._bowtie(c, int(bowtie_failed))
            self._offtarget(c, [int(x) for x in page_failed])
        self.say("Writing results to file.")
        self.say("Cleaning auxiliary files")
        self.say("Done.")
        self.say(f"{c['loaded']} guides evaluated.")
        self.say("This batch ran in {} (dd hh:mm:ss) or {} seconds".format(*_elapsed(seconds)))

    def _secondary_structure(self, c, not_found):
        self.say("mm10db - check secondary structure.")
        length = self._page_length("rnafold_page_length")
        at = c["fold_first"]
        for k, guides in enumerate(_pages(c["fold_first"], c["fold_end"], length)):
            if length > 0:
                self.say(f"\tProcessing page {k + 1} ({length:,} per page).")
            self.say("\t\tConstructing the RNAfold input file.")
            self.say(f"\t\t{guides:,} guides in this page.")
            self.say("\t\tStarting to process the RNAfold results.")
            if length > 0:
                while not_found and not_found[0][0] < at + guides:
                    self.bare(f"Could not find: {not_found.pop(0)[1]}")
            at += guides
        if length <= 0:  # the page was consumed while it was written: nothing was read
            self.say("\t0 of 0 failed here.")
            return
        self.say(f"\t{c['ss_failed']:,} of {c['ss_tested']:,} failed here.")
        if c["ss_erred"] > 0:
            self.say(f"\t{c['ss_erred']} of {c['ss_tested']} erred here.")
        if c["ss_not_found"] > 0:
            self.say(f"\t{c['ss_not_found']} of {c['ss_tested']} not found in RNAfold output.")

    def _bowtie(self, c, failed):
        self.say("Bowtie analysis.")
        length = int(self.config.get("page_length", 0))
        for k, guides in enumerate(_pages(c["selected_first"], c["selected_end"], length)):
            if length > 0:
                self.say(f"\tProcessing page {k + 1} ({length:,} per page).")
            self.say("\tConstructing the Bowtie input file.")
            self.say(f"\t\t{guides:,} guides in this page.")
            self.say("\tStarting to process the Bowtie results.")
        self.say(f"\t{failed:,} of {c['selected_end'] - c['selected_first']:,} failed here.")

    def _offtarget(self, c, page_failed):
        self.say("Beginning off-target scoring.")
        length = self._page_length("offtarget_page_length")
        pages = _pages(c["scored_first"], c["scored_end"], length)
        if len(page_failed) != len(pages):
            raise ValueError(f"{len(page_failed)} figures for {len(pages)} off-target pages")
        tested = 0
        for k, (guides, failed) in enumerate(zip(pages, page_failed)):
            if length > 0:
                self.say(f"\tProcessing page {k + 1} ({length:,} per page).")
            tested += guides
            if guides != length:
                self.say(f"\t\t{guides:,} guides in this page.")
            self.say(f"\t{failed if length > 0 else 0:,} of {tested:,} failed here.")

    def end(self):
        self.say("Total run time (dd hh:mm:ss) or {} seconds".format(*_elapsed(time.time() - self.started)))
