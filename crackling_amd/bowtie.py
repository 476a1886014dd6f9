"""The Bowtie step on a resident genome (issl_genome_occurrences* of include/issl_hip.h): Crackling.py:600-725.

For every guide that reaches the specificity stage the reference writes eight reads -- the guide's 20-mer followed by the
PAMs of BOWTIE_PAMS -- aligns them with Bowtie2 and rejects the guide when more than one perfect alignment is counted.
`Consensus.bowtie(genome)` answers the same question with exact counts over the genome (`BowtieStep`); Bowtie2 itself is
not part of the package: `bowtie_input()` is its input, `read_bowtie_output()` reads what it printed.

What a real Bowtie2 run can answer differently from the exact counts: it may miss a second perfect alignment within its
effort limits; for a read 0 without a perfect occurrence it reports its best inexact alignment where the step reports
`*`; among equal alignments it picks at random where the step picks the least (record, pos, strand).
"""
import ast

import numpy as np

from .scorer import OCCURRENCE_DTYPE

BOWTIE_PAMS = ("AGG", "CGG", "GGG", "TGG", "AAG", "CAG", "GAG", "TAG")  # the reads of a guide, in the reference's order
NO_RECORD = 0xFFFFFFFF
_CODE_OFFSET = OCCURRENCE_DTYPE.fields["code"][1]
_RC = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s[::-1].translate(_RC)


def _pages(n, page_length):
    if page_length <= 0:
        return [(0, n)] if n else []
    return [(a, min(n, a + page_length)) for a in range(0, n, page_length)]


def bowtie_input(guides23):
    """The lines the reference hands Bowtie2 (Crackling.py:626-640): eight reads per guide, guides in the order given."""
    return "".join(g[:20] + pam + "\n" for g in guides23 for pam in BOWTIE_PAMS)


def read_bowtie_output(sam_text, guides23, record_names=(), page_length=0, page_starts=None):
    """Bowtie2's SAM output (--reorder --no-hd) as the reference reads it (Crackling.py:659-720) -> OCCURRENCE_DTYPE array,
    one row per guide of `guides23` (distinct 23-mers in the order their reads were written).  sam_text: the output of all
    pages, one behind the other; page_length: the [bowtie2] page-length of the run (0: one page); page_starts: in its
    place, the boundaries of pages of any length -- n_pages + 1 positions from 0 to len(guides23), never decreasing --
    for a run in batches, whose pages start again with every batch (BowtieStep.page_starts).

    Per page the reads are filed under their text, a later guide replacing an earlier one with the same 20-mer.  The lines
    come in groups of eight.  A group's guide is looked up under the SEQ of its first line, then under its reverse
    complement; chromosome (column 3) and position (column 4) of that line are the guide's.  A line counts once when it
    contains "XM:i:0" and once more when it also contains "XS:i:0"; more than one rejects the guide.  `aligned`, `repeated`
    and `nb` of a row are those of the guide's own group; code, record, pos and strand come from the last group that names
    the guide (`source`: its index), and a guide that no group names stays untested (code 2, owner 0, source 0xFFFFFFFF)
    with the place its own group prints.

    record_names: the names of the genome's records as Bowtie2 prints them; a name that is not among them, such as `*`,
    gives record 0xFFFFFFFF and pos 0.  pos is column 4 less one; strand is bit 16 of the flag; `aligned` and `repeated`
    come from the tags; n_perfect is nb, SAM says no more."""
    guides23 = list(guides23)
    names = {n: k for k, n in enumerate(record_names)}
    lines = sam_text.splitlines()
    if len(lines) != 8 * len(guides23):
        raise ValueError(f"{len(lines)} SAM lines for {len(guides23)} guides: eight per guide expected")
    rows = np.zeros(len(guides23), dtype=OCCURRENCE_DTYPE)
    rows["record"] = NO_RECORD
    rows["code"] = 2

    def group(i):
        first = lines[i].rstrip().split("\t")
        row = np.zeros((), dtype=OCCURRENCE_DTYPE)
        record = names.get(first[2], NO_RECORD)
        row["record"] = record
        row["pos"] = ast.literal_eval(first[3]) - 1 if record != NO_RECORD else 0
        row["strand"] = (int(first[1]) >> 4) & 1 if record != NO_RECORD else 0
        nb = 0
        for v in range(8):
            if "XM:i:0" in lines[i + v]:
                nb += 1
                row["aligned"] |= 1 << v
                if "XS:i:0" in lines[i + v]:
                    nb += 1
                    row["repeated"] |= 1 << v
        row["nb"] = row["n_perfect"] = nb
        row["code"] = 2
        row["source"] = NO_RECORD
        return first[9], row

    if page_starts is None:
        pages = _pages(len(guides23), page_length)
    else:
        starts = [int(x) for x in page_starts]
        if not starts or starts[0] != 0 or starts[-1] != len(guides23) or any(a > b for a, b in zip(starts, starts[1:])):
            raise ValueError(f"page_starts: boundaries from 0 to {len(guides23)} that never decrease")
        pages = list(zip(starts, starts[1:]))
    for a, b in pages:
        filed = {}
        for k in range(a, b):
            for pam in BOWTIE_PAMS:
                filed[guides23[k][:20] + pam] = k
        groups = [group(8 * k) for k in range(a, b)]
        for k, (_, row) in zip(range(a, b), groups):
            rows[k] = row
        for k, (read, row) in zip(range(a, b), groups):
            target = filed.get(read, filed.get(_rc(read)))
            if target is None:
                raise ValueError(f"SAM line {8 * k + 1}: read {read} belongs to no guide of its page")
            for f in ("record", "pos", "strand"):
                rows[f][target] = row[f]
            rows["owner"][target], rows["code"][target], rows["source"][target] = 1, 0 if row["nb"] > 1 else 1, k
    return rows


def format_columns(rows, record_names):
    """OCCURRENCE_DTYPE rows -> {"passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd"}: lists of str, one entry per row,
    as the reference prints them: start = pos + 1 and end = pos + 23 of the first occurrence of read 0, chromosome = its
    record's name up to the first blank, as Bowtie2 names it; `*`, 0, 22 when read 0 does not occur (what the reference
    makes of an unaligned line); `?` four times for a guide the reference leaves untested."""
    names = [(n.split() or [""])[0] for n in record_names]
    out = {c: [] for c in ("passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd")}
    for row in rows:
        if row["code"] == 2:
            vals = ("?", "?", "?", "?")
        elif row["record"] == NO_RECORD:
            vals = (str(row["code"]), "*", "0", "22")
        else:
            vals = (str(row["code"]), names[row["record"]], str(int(row["pos"]) + 1), str(int(row["pos"]) + 23))
        for c, v in zip(out, vals):
            out[c].append(v)
    return out


class BowtieStep:
    """The Bowtie step over the selection of a finished Consensus (Consensus.bowtie).  `rows`: OCCURRENCE_DTYPE array
    aligned with consensus.selected; `columns()`: the reference's four columns; `selected_tensor()`: the rows that go on
    to off-target scoring.  The signatures are gathered and the rows written on the device.  batch_size: [input]
    batch-size; above 0 the pages start again with every batch of that many rows of the guide set, and `page_starts` keeps
    their boundaries in positions of the selection (an int64 CUDA tensor of its own; None for one batch, whose pages are
    page_length each).  events: the pages' boundaries are made in every case and `page_events` (an int32 CUDA tensor, one
    word per page) receives the figure the reference's log prints as the step's `failed` (Crackling.py:709-717): the groups
    of the page that reject the site they name while it is not rejected -- events, not rows (include/issl_hip.h,
    issl_genome_occurrences_paged_events_device).  The rows are the same bytes with and without."""

    def __init__(self, consensus, genome, page_length=0, batch_size=0, events=False):
        import torch
        if not consensus.finished:
            raise ValueError("the consensus is not finished")
        self.consensus = consensus
        self.genome = genome
        self.page_length = int(page_length)
        self.batch_size = int(batch_size)
        paged = self.batch_size > 0 or events
        self.page_starts = consensus.selection_pages(self.batch_size, self.page_length).clone() if paged else None
        self.page_events = torch.zeros(self.page_starts.numel() - 1, dtype=torch.int32, device=self.page_starts.device) if events else None
        sel = consensus.selected_tensor()
        sigs = consensus.guide_set.sigs_tensor()[sel.to(torch.int64)].contiguous()
        self._d_rows = torch.empty((sigs.numel(), OCCURRENCE_DTYPE.itemsize), dtype=torch.uint8, device=sigs.device)
        genome.occurrences_device(sigs, self._d_rows, self.page_length, stream=torch.cuda.current_stream(sigs.device).cuda_stream,
                                  page_starts=self.page_starts, page_events=self.page_events)
        self._rows = None

    def batch_events(self, batches):
        """The step's `failed` figure of every batch: the events of the pages that start in the batch's share of the
        selection.  batches: runlog.BATCH_DTYPE entries (selected_first, selected_end).  Two small copies from the device,
        one word per page each."""
        if self.page_events is None:
            raise ValueError("the step was made without events")
        starts, events = self.page_starts.cpu().numpy()[:-1], self.page_events.cpu().numpy()
        return [int(events[(starts >= int(b["selected_first"])) & (starts < int(b["selected_end"]))].sum()) for b in batches]

    def rows_tensor(self):
        """uint8 CUDA tensor [n_selected, 32]: the rows in device memory."""
        return self._d_rows

    @property
    def rows(self):
        if self._rows is None:
            self._rows = self._d_rows.cpu().numpy().view(OCCURRENCE_DTYPE).reshape(-1)
        return self._rows

    def columns(self):
        """format_columns() of the rows, with the names of the genome's records."""
        return format_columns(self.rows, [name.decode(errors="replace") for name, _ in self.genome.records])

    def transcripts(self, annotation):
        """The `hits` column of countHitTranscripts.py for the rows of this step (transcripts.TranscriptHits): answered
        from the rows where they lie, the result stays on the device."""
        from .transcripts import TranscriptHits
        return TranscriptHits(self, annotation)

    def selected_tensor(self):
        """int32 CUDA tensor: the rows of the guide set the reference's filter passes on to off-target scoring
        (Crackling.py:85-87, :144-146).  At medium and high these are the consensus selection without the rows Bowtie
        rejected (code 0); at ultralow and low the selection itself.  Built on the device; the host waits once, for the
        number of rows."""
        sel = self.consensus.selected_tensor()
        if self.consensus.optimisation < 2:
            return sel
        return sel[self._d_rows[:, _CODE_OFFSET] != 0]
