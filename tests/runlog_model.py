"""Host model of the figures of the reference's log (crackling_amd.runlog, issl_runlog_* of include/issl_hip.h), built on
the host models of the stages: guides_util (extraction), consensus_util (the efficiency tests), batches_util (the pages
of a batched run, RNAfold's answers per page), bowtie_util (the Bowtie step) and the C oracle (the scores).  Nothing of
the library's device code runs here.  tests/test_runlog_model.py pins the model, through crackling_amd.RunLog, to the
reference's own logs (tests/golden/runlog) before tests/test_runlog_gpu.py compares the device's counts with it.

Three kinds of figures:
  batch_counts    per batch, counts over finished rows: what issl_runlog_batches makes on the device
  bowtie_events   the Bowtie step's `failed` (Crackling.py:709-717): the groups of a page are walked in order, and a group
                  that rejects the site it names counts when that site is not rejected at that moment.  A site named
                  reject, accept, reject counts twice; the finished rows only know the last group
  file_counts     per input file (Crackling.py:254-258): its matches, those that met a guide seen before, and the running
                  numbers of distinct guides seen twice or more and of distinct guides"""
import numpy as np

import batches_util as bt
import bowtie_util as bu
import consensus_util as cu
import guides_util as gu
import results_util as ru

FIELDS = ("loaded", "g20_tested", "g20_failed", "lead_t_tested", "lead_t_failed", "at_tested", "at_failed", "tttt_tested",
          "tttt_failed", "ss_tested", "ss_failed", "ss_erred", "ss_not_found", "mm10db_accepted", "mm10db_failed",
          "sgrna_tested", "sgrna_failed", "consensus_tested", "consensus_failed", "fold_first", "fold_end", "selected_first",
          "selected_end", "scored_first", "scored_end", "page_first", "page_end", "bowtie_rejected")
DTYPE = np.dtype([(f, "<u4") for f in FIELDS])
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_RC)


def batch_counts(rows, consensus_n, fold_rows, present, selection, bowtie_codes, scored, mit, cfd, method, threshold, batch_size,
                 offtarget_page_length):
    """rows: consensus rows of all guides (fields g20 .. count); fold_rows, selection, scored: ascending rows of the set;
    present: per row of the fold list, RNAfold answered (None: the rows the consensus left untested did not);
    bowtie_codes: per selected row (None: no Bowtie step); mit, cfd: per scored row.
    -> (DTYPE array per batch, failed per off-target page, positions of the fold list without an answer)."""
    n = len(rows)
    fold_rows, selection, scored = (np.asarray(x, dtype=np.int64) for x in (fold_rows, selection, scored))
    ss = np.asarray(rows["ss"])[fold_rows]
    absent = (ss == 2) if present is None else (np.asarray(present) == 0)
    rejected = np.zeros(len(scored), dtype=bool)
    for k in range(len(scored)):
        a = ru.through_text(float(mit[k])) if method in ru.PRINTS_MIT else -1.0
        c = ru.through_text(float(cfd[k])) if method in ru.PRINTS_CFD else -1.0
        rejected[k] = ru.verdict(a, c, method, float(threshold)) == 0
    out, page_failed = [], []
    for lo, hi in bt.batches(n, batch_size if batch_size < n else 0):
        b = np.zeros((), dtype=DTYPE)
        r = rows[lo:hi]
        b["loaded"] = hi - lo
        for f, name in (("g20", "g20"), ("lead_t", "lead_t"), ("at_pct", "at"), ("tttt", "tttt"), ("sgrna", "sgrna")):
            b[name + "_tested"] = int(np.sum(r[f] <= 1))
            b[name + "_failed"] = int(np.sum(r[f] == 0))
        b["mm10db_accepted"] = int(np.sum(r["mm10db"] == 1))
        b["mm10db_failed"] = int(np.sum(r["mm10db"] != 1))
        b["consensus_tested"] = hi - lo
        b["consensus_failed"] = int(np.sum(r["count"] < consensus_n))
        f0, f1 = (int(np.searchsorted(fold_rows, x)) for x in (lo, hi))
        b["fold_first"], b["fold_end"] = f0, f1
        b["ss_tested"], b["ss_failed"] = int(np.sum(ss[f0:f1] <= 1)), int(np.sum(ss[f0:f1] == 0))
        b["ss_erred"], b["ss_not_found"] = int(np.sum(ss[f0:f1] == 3)), int(np.sum(absent[f0:f1]))
        s0, s1 = (int(np.searchsorted(selection, x)) for x in (lo, hi))
        b["selected_first"], b["selected_end"] = s0, s1
        if bowtie_codes is not None:
            b["bowtie_rejected"] = int(np.sum(np.asarray(bowtie_codes)[s0:s1] == 0))
        k0, k1 = (int(np.searchsorted(scored, x)) for x in (lo, hi))
        b["scored_first"], b["scored_end"] = k0, k1
        b["page_first"] = len(page_failed)
        if offtarget_page_length > 0:
            page_failed += [int(np.sum(rejected[a:min(a + offtarget_page_length, k1)])) for a in range(k0, k1, offtarget_page_length)]
        else:
            page_failed.append(int(np.sum(rejected[k0:k1])))
        b["page_end"] = len(page_failed)
        out.append(b)
    batches = np.array(out, dtype=DTYPE) if out else np.zeros(0, dtype=DTYPE)
    return batches, np.array(page_failed, dtype=np.uint32), np.flatnonzero(absent).astype(np.uint32)


def bowtie_events(model, guides20, starts):
    """model: bowtie_util.Model of the genome; guides20: the 20-mers of the selection; starts: the pages' boundaries.
    -> (events per page, the code every site ends with): the reference's loop, one group per guide in page order."""
    own = model.counts(np.array([bu.sig(g) for g in guides20], dtype=np.uint64))
    events, codes = [], np.full(len(guides20), 2, dtype=np.uint8)
    starts = [int(x) for x in starts]
    for a, b in zip(starts, starts[1:]):
        filed = {}
        for k in range(a, b):
            for pam in bu.PAMS:
                filed[guides20[k] + pam] = k
        count = 0
        for k in range(a, b):
            read = guides20[k] + bu.PAMS[0]
            printed = rc(read) if own["record"][k] != bu.NONE and own["strand"][k] == 1 else read
            t = filed[printed] if printed in filed else filed[rc(printed)]
            if own["nb"][k] > 1:
                count += codes[t] != 0
                codes[t] = 0
            else:
                codes[t] = 1
        events.append(int(count))
    return events, codes


def constructed_page():
    """-> (genome FASTA, three guides in page order, the index of the named one).  The genome holds one window W = CCT N17 NGG
    and, behind it, one more copy of the strand-1 guide's 20-mer in front of CGG.  The guides: the window's strand-1 guide B
    = rc(W), the strand-0 guide A = W, and B's 20-mer with the PAM CGG.  Both B groups print W (their read 0 first occurs on
    strand 1) and so name A, and reject: their reads align twice.  A's own group names A and accepts."""
    w = "CCTGATTGCAGTCAGGTCATCGG"
    b = rc(w)
    assert b.endswith("AGG") and w[20:] != "AGG"
    pad = "ATATATATATAT"
    genome = (">one\n" + pad + w + pad + b[:20] + "CGG" + pad + "\n").encode()
    return genome, [b, w, b[:20] + "CGG"], 1


def file_counts(blobs):
    """-> per input [identified, duplicates, distinct guides seen twice or more so far, distinct guides so far]."""
    seen, out, done = {}, [], 0
    for f in range(len(blobs)):
        records = gu.parse(blobs[:f + 1])  # (what an input's records are depends on the headers of the inputs before it)
        identified = duplicates = 0
        for _, seq in records[done:]:
            for _, _, guide in gu.matches(seq):
                identified += 1
                duplicates += guide in seen
                seen[guide] = seen.get(guide, 0) + 1
        done = len(records)
        out.append([identified, duplicates, sum(v > 1 for v in seen.values()), len(seen)])
    return out


class Run:
    """Every figure of a golden run's log from the host models of the stages.  run: an entry of tests/golden/runlog/runs.json;
    fold_text: what RNAfold's stand-in printed for (a superset of) its guides."""

    def __init__(self, run, fold_text):
        import oracle_util as ou
        import runlog_util as rl
        self.run = run
        self.inputs = rl.golden_inputs(run)
        blobs = [blob for _, blob in self.inputs]
        self.files = file_counts(blobs)
        guides = gu.brute_force(gu.parse(blobs))
        self.seqs = seqs = ru.guide_strings(guides)
        self.n = n = len(seqs)
        kw = ru.golden_keywords(run)
        m = cu.Model(seqs, guides["seen"], **{k: kw[k] for k in ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model",
                                                                 "sgrna_threshold", "low_energy", "high_energy")})
        self.batch_size = run["batch_size"]
        self.fold_rows = m.fold_rows
        fold_guides = [seqs[j] for j in m.fold_rows]
        self.folds, _, _ = bt.fold_answers(fold_text, m.fold_rows, fold_guides, n, self.batch_size, run["rnafold_page_length"])
        m.finish(self.folds)
        self.rows, self.consensus_n, self.selection = m.rows, run["n"], m.selected
        self.bowtie_codes, self.events = None, []
        self.scored, self.mit, self.cfd = np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0)
        if run["enabled"]:
            genome = bu.Model([rl.golden_genome(run)]) if run.get("genome") else bu.golden_model()
            sel = m.selected
            guides20 = [seqs[j][:20] for j in sel]
            self.starts = bt.page_starts(sel, n, self.batch_size, run["page_length"])
            sigs = np.array([bu.sig(g) for g in guides20], dtype=np.uint64)
            brows = bt.paged_rows(genome, sigs, self.starts)
            self.events, codes = bowtie_events(genome, guides20, self.starts)
            assert np.array_equal(codes, brows["code"]), "the loop and the vectorised model end with other verdicts"
            self.bowtie_codes = brows["code"]
            self.scored = sel if m.level < 2 else sel[brows["code"] != 0]
            oracle = ou.OracleIndex(bu.GOLDEN / "index.issl")
            self.mit, self.cfd = oracle.score(np.array([bu.sig(seqs[j][:20]) for j in self.scored], dtype=np.uint64),
                                              run["max_distance"], float(run["score_threshold"]), run["method"])
            oracle.close()

    def counts(self, batch_size=None, offtarget_page_length=None):
        page = self.run["offtarget_page_length"] if offtarget_page_length is None else offtarget_page_length
        return batch_counts(self.rows, self.consensus_n, self.fold_rows, None if self.folds is None else self.folds["present"],
                            self.selection, self.bowtie_codes, self.scored, self.mit, self.cfd, self.run["method"],
                            float(self.run["score_threshold"]), self.batch_size if batch_size is None else batch_size,
                            5000000 if page is None else page)

    def batch_events(self, batches):
        """The Bowtie step's `failed` per batch: the events of the batch's pages."""
        starts = [int(x) for x in self.starts] if self.run["enabled"] else [0]
        return [sum(e for a, e in zip(starts, self.events) if b["selected_first"] <= a < b["selected_end"]) for b in batches]

    def feed(self, log):
        """The whole log into a crackling_amd.RunLog."""
        batches, page_failed, not_found = self.counts()
        events = self.batch_events(batches)
        log.begin()
        total, done = sum(len(blob) for _, blob in self.inputs), 0
        for (identified, duplicates, repeated, distinct), (name, blob) in zip(self.files, self.inputs):
            done += len(blob)
            log.input_file(name, identified, repeated, duplicates, distinct, done / total * 100.0)
        missing = [(int(p), self.seqs[int(self.fold_rows[p])][:20]) for p in not_found]
        for k, b in enumerate(batches):
            log.batch(k, len(batches), b, page_failed[b["page_first"]:b["page_end"]],
                      [x for x in missing if b["fold_first"] <= x[0] < b["fold_end"]], events[k])
        log.end()
        return log
