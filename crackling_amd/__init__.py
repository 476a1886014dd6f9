"""crackling_amd -- MI355X-native drop-in for Crackling's ISSL off-target scoring step.

Only the hot path of bmds-lab/Crackling is here: `isslScoreOfftargets`
(reference: src/ISSL/isslScoreOfftargets.cpp, called from src/crackling/Crackling.py:727-837) and the
producer of its input format, `isslCreateIndex` (src/ISSL/isslCreateIndex.cpp).  The compute lives in
libissl_hip.so (hand-written HIP for gfx950 behind the C ABI of include/issl_hip.h); this package is
the thin host-side mirror used by tests, bench.py and Python callers.  Importing it without the built
library raises immediately -- there is no CPU fallback.
"""
from ._lib import lib, IsslError, LIB_PATH  # noqa: F401
from .scorer import (  # noqa: F401
    BULGE_HIT_DTYPE,
    BULGE_VARIANT_HIT_DTYPE,
    GUIDE_DTYPE,
    HAPLOTYPE_HIT_DTYPE,
    Haplotypes,
    INDEL_DTYPE,
    Genome,
    GuideSet,
    IsslIndex,
    IsslNode,
    LANDING_DTYPE,
    LANDING_PROFILE_DTYPE,
    LOCATION_DTYPE,
    METHODS,
    OCCURRENCE_DTYPE,
    OFFTARGET_DTYPE,
    PROFILE_DTYPE,
    SEARCH_HIT_DTYPE,
    SEARCH_QUERY_DTYPE,
    SNP_DTYPE,
    VARIANT_HIT_DTYPE,
    encode_guides,
    extract_offtargets,
    decode_guides,
    format_scores,
    format_scores_native,
    run_scorer_binary,
    parse_scorer_output,
    search_prepare,
    vcf_indels,
    vcf_snps,
    verdicts,
)

from .consensus import (  # noqa: F401
    CONSENSUS_DTYPE,
    Consensus,
    FOLD_DTYPE,
    SCAFFOLD,
    load_sgrnascorer2,
    read_rnafold_output,
)

from .bowtie import (  # noqa: F401
    BOWTIE_PAMS,
    BowtieStep,
    bowtie_input,
    format_columns,
    read_bowtie_output,
)

from .transcripts import (  # noqa: F401
    TRANSCRIPT_HITS_DTYPE,
    Annotation,
    TranscriptHits,
    format_hits,
)

from .results import (  # noqa: F401
    PackedFolds,
    ResultTable,
    read_rnafold_text,
    repr_f64,
)
from .folds import Folds  # noqa: F401
from .runlog import BATCH_DTYPE, BatchCounts, RunLog  # noqa: F401
from . import pipeline  # noqa: F401

__all__ = [
    "BATCH_DTYPE", "BatchCounts", "RunLog", "Folds", "PackedFolds", "ResultTable", "read_rnafold_text", "repr_f64", "pipeline",
    "TRANSCRIPT_HITS_DTYPE", "Annotation", "TranscriptHits", "format_hits",
    "BOWTIE_PAMS", "BowtieStep", "OCCURRENCE_DTYPE", "bowtie_input", "format_columns", "read_bowtie_output",
    "CONSENSUS_DTYPE", "Consensus", "FOLD_DTYPE", "SCAFFOLD", "load_sgrnascorer2", "read_rnafold_output",
    "GUIDE_DTYPE", "Genome", "GuideSet", "IsslIndex", "IsslNode", "IsslError", "LANDING_DTYPE", "LANDING_PROFILE_DTYPE", "LOCATION_DTYPE", "METHODS", "OFFTARGET_DTYPE", "PROFILE_DTYPE", "encode_guides", "extract_offtargets", "decode_guides", "format_scores", "format_scores_native",
    "run_scorer_binary", "parse_scorer_output", "verdicts", "lib", "LIB_PATH", "SEARCH_HIT_DTYPE", "SEARCH_QUERY_DTYPE", "search_prepare",
    "BULGE_HIT_DTYPE", "VARIANT_HIT_DTYPE", "BULGE_VARIANT_HIT_DTYPE", "SNP_DTYPE", "vcf_snps",
    "INDEL_DTYPE", "HAPLOTYPE_HIT_DTYPE", "Haplotypes", "vcf_indels",
]
