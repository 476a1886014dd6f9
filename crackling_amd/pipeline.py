"""Crackling.py from FASTA to its output file over the resident stages: extract -> consensus -> RNAfold -> Bowtie step ->
off-target scores -> result table.  Glue over the package's classes; no configuration file is read and nothing is written
to disk.  One batch is the whole guide set.
"""
from .consensus import Consensus, read_rnafold_output
from .results import ResultTable, read_rnafold_text
from .scorer import GuideSet

CONSENSUS_KEYS = ("optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", "model", "sgrna_threshold", "low_energy", "high_energy")
SCORE_CHUNK = 1 << 22  # guides per scoring call


def run(inputs, genome, index, config, rnafold):
    """inputs: the FASTA inputs of GuideSet.extract (bytes blobs or paths); genome: a Genome (the Bowtie step's text) and
    index: an uploaded IsslIndex, both on the device the guides go to, or None when config["offtargetscore"] is false;
    rnafold: a callable that takes RNAfold's input (Consensus.fold_input()) and returns what RNAfold printed.
    config: a mapping with the keywords of Consensus (CONSENSUS_KEYS) and, all optional,
      offtargetscore  run the Bowtie step and the scoring ([offtargetscore] enabled; default True)
      page_length     [bowtie2] page-length (0: one page)
      max_distance, score_threshold, method   [offtargetscore] max-distance (4), score-threshold (75), method ("and")
      delimiter       [output] delimiter (",")
      device          the GPU (0)
    -> the bytes of the reference's output file for these inputs."""
    import torch
    device = int(config.get("device", 0))
    method = str(config.get("method", "and"))
    threshold = float(config.get("score_threshold", 75.0))
    with GuideSet.extract(inputs, device) as gs, Consensus(gs, **{k: config[k] for k in CONSENSUS_KEYS if k in config}) as c:
        folds_text = None
        if c.n_fold:
            guides = c.fold_guides()
            text = rnafold(c.fold_input())
            folds_text = read_rnafold_text(text, guides)
            c.finish(read_rnafold_output(text, guides))
        else:
            c.finish()
        bowtie = scores = None
        if config.get("offtargetscore", True):
            bowtie = c.bowtie(genome, int(config.get("page_length", 0)))
            rows = bowtie.selected_tensor()
            sigs = gs.sigs_tensor()[rows.to(torch.int64)].contiguous()
            mit = torch.empty(sigs.numel(), dtype=torch.float64, device=sigs.device)
            cfd = torch.empty_like(mit)
            stream = torch.cuda.current_stream(sigs.device).cuda_stream
            for a in range(0, sigs.numel(), SCORE_CHUNK):
                b = min(a + SCORE_CHUNK, sigs.numel())
                index.score_device(sigs[a:b], mit[a:b], cfd[a:b], int(config.get("max_distance", 4)), threshold, method, stream=stream)
            scores = (rows, mit, cfd)
        with ResultTable(c, folds_text, bowtie, scores, config.get("delimiter", ","), method, threshold) as table:
            return table.to_bytes()
