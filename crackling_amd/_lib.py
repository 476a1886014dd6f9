"""ctypes binding of libissl_hip.so (C ABI declared in include/issl_hip.h)."""
import ctypes as C
import os

# ISSL_HIP_LIBRARY: another build of the same library (A/B of kernel variants, tools/ablate.py); default: the in-tree one
LIB_PATH = os.environ.get("ISSL_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libissl_hip.so")


class IsslError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()). "
        "crackling_amd has no CPU fallback for the ISSL scorer."
    )



def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64 (same
    SONAME as /opt/rocm's).  If libissl_hip.so pulled in /opt/rocm's copy first, a later `import torch` would bring
    a second runtime into the process and that one finds no GPU.  So when torch is installed, its libamdhip64 is
    loaded first (without importing torch); libissl_hip.so's DT_NEEDED libamdhip64.so.7 then binds to it by SONAME.
    The standalone executables in bin/ do not go through here and use /opt/rocm's runtime."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return cand
    return None


HIP_RUNTIME = _preload_hip_runtime()
lib = C.CDLL(LIB_PATH)


class Header(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_sites", "seq_len", "n_lines", "slice_width", "n_slices", "n_scores")]


class Hit(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("guide", "slice", "pos", "id", "dist", "occ")]


PROFILE_BINS = 7


class Offtarget(C.Structure):
    """issl_offtarget: 40 bytes, no padding."""
    _fields_ = [("site", C.c_uint64), ("mit", C.c_double), ("cfd", C.c_double), ("guide", C.c_uint32), ("id", C.c_uint32),
                ("occ", C.c_uint32), ("dist", C.c_uint16), ("slice", C.c_uint16)]


class Profile(C.Structure):
    """issl_profile: 88 bytes."""
    _fields_ = [("sites", C.c_uint32 * PROFILE_BINS), ("pad", C.c_uint32), ("occurrences", C.c_uint64 * PROFILE_BINS)]


class Location(C.Structure):
    """issl_location: 16 bytes, no padding."""
    _fields_ = [("pos", C.c_uint64), ("record", C.c_uint32), ("strand", C.c_uint32)]


class SearchPattern(C.Structure):
    """issl_search_pattern: 32 bytes."""
    _fields_ = [("allow", C.c_uint32 * 4), ("length", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SearchQuery(C.Structure):
    """issl_search_query: 16 bytes."""
    _fields_ = [("sig", C.c_uint64), ("care", C.c_uint64)]


class SearchHit(C.Structure):
    """issl_search_hit: 32 bytes, no padding."""
    _fields_ = [("site", C.c_uint64), ("pos", C.c_uint64), ("record", C.c_uint32), ("query", C.c_uint32), ("mism", C.c_uint32),
                ("strand", C.c_uint8), ("dist", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class SearchBulges(C.Structure):
    """issl_search_bulges: 16 bytes."""
    _fields_ = [("guide_start", C.c_uint32), ("guide_length", C.c_uint32), ("max_dna", C.c_uint32), ("max_rna", C.c_uint32)]


class BulgeHit(C.Structure):
    """issl_bulge_hit: 32 bytes, no padding."""
    _fields_ = [("site", C.c_uint64), ("pos", C.c_uint64), ("record", C.c_uint32), ("query", C.c_uint32), ("mism", C.c_uint32),
                ("strand", C.c_uint8), ("dist", C.c_uint8), ("bulge", C.c_int8), ("at", C.c_uint8)]


class VariantHit(C.Structure):
    """issl_variant_hit: 40 bytes, no padding."""
    _fields_ = [("pos", C.c_uint64), ("site", C.c_uint32 * 4), ("record", C.c_uint32), ("query", C.c_uint32), ("mism", C.c_uint32),
                ("strand", C.c_uint8), ("dist", C.c_uint8), ("n_var", C.c_uint8), ("reserved", C.c_uint8)]


class BulgeVariantHit(C.Structure):
    """issl_bulge_variant_hit: 48 bytes, no padding."""
    _fields_ = [("pos", C.c_uint64), ("site", C.c_uint32 * 4), ("record", C.c_uint32), ("query", C.c_uint32), ("mism", C.c_uint32),
                ("strand", C.c_uint8), ("dist", C.c_uint8), ("n_var", C.c_uint8), ("bulge", C.c_int8), ("at", C.c_uint8),
                ("reserved", C.c_uint8 * 7)]


class Snp(C.Structure):
    """issl_snp: 16 bytes."""
    _fields_ = [("pos", C.c_uint64), ("record", C.c_uint32), ("ref", C.c_uint8), ("alt", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class VcfCounts(C.Structure):
    """issl_vcf_counts: 48 bytes."""
    _fields_ = [(n, C.c_uint64) for n in ("lines", "snps", "alleles_skipped", "no_allele", "unknown_chrom", "beyond_record")]


class Indel(C.Structure):
    """issl_indel: 32 bytes."""
    _fields_ = [("pos", C.c_uint64), ("record", C.c_uint32), ("ref_len", C.c_uint32), ("alt_len", C.c_uint32), ("ref_at", C.c_uint32),
                ("alt_at", C.c_uint32), ("reserved", C.c_uint32)]


class VcfIndelCounts(C.Structure):
    """issl_vcf_indel_counts: 56 bytes."""
    _fields_ = [(n, C.c_uint64) for n in ("lines", "indels", "alleles_skipped", "no_allele", "unknown_chrom", "beyond_record", "too_long")]


class HaplotypeHit(C.Structure):
    """issl_haplotype_hit: 48 bytes, no padding."""
    _fields_ = [("pos", C.c_uint64), ("site", C.c_uint32 * 4), ("record", C.c_uint32), ("query", C.c_uint32), ("mism", C.c_uint32),
                ("strand", C.c_uint8), ("dist", C.c_uint8), ("n_var", C.c_uint8), ("reserved", C.c_uint8), ("indel", C.c_uint32),
                ("edit_at", C.c_int32)]


class TranscriptHitsRow(C.Structure):
    """issl_transcript_hits: 16 bytes."""
    _fields_ = [("hit", C.c_uint32), ("total", C.c_uint32), ("status", C.c_uint32), ("first", C.c_uint32)]


class Landing(C.Structure):
    """issl_landing: 64 bytes, no padding."""
    _fields_ = [("site", C.c_uint64), ("pos", C.c_uint64), ("record", C.c_uint32), ("strand", C.c_uint32), ("guide", C.c_uint32),
                ("rank", C.c_uint32), ("id", C.c_uint32), ("occ", C.c_uint32), ("dist", C.c_uint16), ("slice", C.c_uint16),
                ("pad", C.c_uint32), ("hits", TranscriptHitsRow)]


class LandingProfile(C.Structure):
    """issl_landing_profile: 144 bytes."""
    _fields_ = [("located", C.c_uint64 * PROFILE_BINS), ("in_exon", C.c_uint64 * PROFILE_BINS), ("absent", C.c_uint32 * PROFILE_BINS),
                ("pad", C.c_uint32)]


class Guide(C.Structure):
    """issl_guide: 32 bytes, no padding."""
    _fields_ = [("guide23", C.c_uint64), ("start", C.c_uint64), ("record", C.c_uint32), ("strand", C.c_uint32),
                ("seen", C.c_uint32), ("reserved", C.c_uint32)]


class ConsensusConfig(C.Structure):
    """issl_consensus_config."""
    _fields_ = [("optimisation", C.c_uint32), ("n", C.c_uint32), ("mm10db", C.c_uint32), ("chopchop", C.c_uint32),
                ("sgrnascorer2", C.c_uint32), ("n_sv", C.c_uint32), ("sv", C.c_void_p), ("coef", C.c_void_p),
                ("intercept", C.c_double), ("sgrna_threshold", C.c_double), ("low_energy", C.c_double), ("high_energy", C.c_double)]


class ResultsConfig(C.Structure):
    """issl_results_config."""
    _fields_ = [("delimiter", C.c_char), ("flags", C.c_uint32), ("method", C.c_char_p), ("threshold", C.c_double)]


class TextSpan(C.Structure):
    """issl_text_span: 16 bytes."""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [
        ("n_guides", C.c_uint64), ("candidates", C.c_uint64), ("hits", C.c_uint64), ("scan_tiles", C.c_uint64),
        ("ms_bin", C.c_double), ("ms_scan", C.c_double), ("ms_verify", C.c_double), ("ms_group", C.c_double),
        ("ms_replay", C.c_double), ("ms_total", C.c_double), ("scan_launches", C.c_uint64), ("raw_records", C.c_uint64), ("n_batches", C.c_uint64),
        ("planned_comparisons", C.c_uint64), ("reference_comparisons", C.c_uint64), ("pruned", C.c_uint64),
        ("ms_scan_events", C.c_double),
    ]


class Span(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_char)), ("len", C.c_size_t)]


class NodeInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int), ("used_rccl", C.c_int), ("ms_upload", C.c_double),
                ("ms_broadcast", C.c_double), ("ms_last_score", C.c_double)]


_P = C.c_void_p
_u64p = C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)

_protos = {
    "issl_last_error": (C.c_char_p, []),
    "issl_abi_version": (C.c_int, []),
    "issl_index_open": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "issl_index_from_memory": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "issl_index_build_from_text": (C.c_int, [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "issl_index_build_from_sites": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "issl_index_build_on_device": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "issl_index_build_on_device_opt": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_char_p, C.POINTER(_P)]),
    "issl_index_build_from_device_sites": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_char_p, C.POINTER(_P)]),
    "issl_index_build_from_fasta": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_size_t, C.c_int,
                                              C.c_char_p, C.POINTER(_P)]),
    "issl_index_build_from_fasta_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_size_t, C.c_int, C.c_char_p,
                                                    C.POINTER(_P)]),
    "issl_index_write": (C.c_int, [_P, C.c_char_p]),
    "issl_index_header": (C.c_int, [_P, C.POINTER(Header)]),
    "issl_index_bucket_sizes": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_index_close": (C.c_int, [_P]),
    "issl_index_device_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "issl_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "issl_index_upload": (C.c_int, [_P, C.c_int]),
    "issl_index_upload_into": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "issl_index_attach_image": (C.c_int, [C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "issl_index_image": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "issl_index_copy_image_to": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_index_cold": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "issl_index_attach_image_cold": (C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(_P)]),
    "issl_index_set_option": (C.c_int, [_P, C.c_char_p, C.c_char_p]),
    "issl_index_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_longlong)]),
    "issl_encode_guides": (C.c_int, [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, _P]),
    "issl_decode_guide": (C.c_int, [C.c_uint64, C.c_size_t, C.c_char_p]),
    "issl_read_query_file": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "issl_free": (None, [_P]),
    "issl_format_scores": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.POINTER(Span)), C.POINTER(C.c_size_t)]),
    "issl_free_spans": (None, [C.POINTER(Span), C.c_size_t]),
    "issl_method_from_string": (C.c_int, [C.c_char_p]),
    "issl_score": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P]),
    "issl_score_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "issl_score_device_async": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "issl_score_wait": (C.c_int, [_P, _P]),
    "issl_score_finish": (C.c_int, [_P, _P]),
    "issl_dump_hits": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_offtarget_profile": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "issl_offtarget_profile_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "issl_offtargets": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_offtargets_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_last_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "issl_count_candidates": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "issl_verdicts": (C.c_int, [_P, _P, C.c_size_t, C.c_double, C.c_char_p, _P]),
    "issl_extract_from_memory": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int,
                                           C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "issl_extract_offtargets": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]),
    "issl_genome_open": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(_P)]),
    "issl_genome_open_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_P)]),
    "issl_genome_info": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "issl_genome_record": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "issl_genome_locate": (C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_genome_locate_device": (C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_search_prepare": (C.c_int, [C.c_char_p, _P, C.c_size_t, C.c_size_t, _P, _P]),
    "issl_genome_search": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_genome_search_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_genome_search_profile": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P]),
    "issl_genome_search_profile_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P, _P]),
    "issl_genome_search_bulges": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_genome_search_bulges_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_genome_search_bulges_profile": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P]),
    "issl_genome_search_bulges_profile_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P]),
    "issl_genome_search_bulges_variants": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_genome_search_bulges_variants_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_genome_search_bulges_variants_profile": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "issl_genome_search_bulges_variants_profile_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P]),
    "issl_genome_search_variants": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_genome_search_variants_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_genome_search_variants_profile": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "issl_genome_search_variants_profile_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P]),
    "issl_vcf_snps": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), _u64p, C.c_size_t, _P, C.c_size_t,
                                C.POINTER(C.c_size_t), C.POINTER(VcfCounts)]),
    "issl_vcf_indels": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), _u64p, C.c_size_t, _P, C.c_size_t,
                                  C.POINTER(C.c_size_t), _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(VcfIndelCounts)]),
    "issl_haplotypes_open": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "issl_haplotypes_open_vcf": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(VcfIndelCounts), C.POINTER(_P)]),
    "issl_haplotypes_info": (C.c_int, [_P, _u64p, _u64p, C.POINTER(C.c_uint32)]),
    "issl_haplotypes_close": (C.c_int, [_P]),
    "issl_haplotypes_search": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_haplotypes_search_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_haplotypes_search_profile": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "issl_haplotypes_search_profile_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P]),
    "issl_genome_apply_snps": (C.c_int, [_P, _P, C.c_size_t, _u64p]),
    "issl_genome_apply_vcf": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(VcfCounts), _u64p]),
    "issl_genome_occurrences": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P]),
    "issl_genome_occurrences_device": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P]),
    "issl_genome_occurrences_paged": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "issl_genome_occurrences_paged_device": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P, _P]),
    "issl_genome_occurrences_paged_events_device": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P]),
    "issl_genome_close": (C.c_int, [_P]),
    "issl_guides_extract": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(_P)]),
    "issl_guides_extract_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_P)]),
    "issl_guides_info": (C.c_int, [_P, _u64p, _u64p, _u64p, _u64p]),
    "issl_guides_record": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "issl_guides_file_counts": (C.c_int, [_P, C.c_uint64, _P]),
    "issl_guides_files": (C.c_int, [_P, _u64p]),
    "issl_guides_copy": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_guides_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "issl_guides_close": (C.c_int, [_P]),
    "issl_consensus_begin": (C.c_int, [_P, C.POINTER(ConsensusConfig), C.POINTER(_P)]),
    "issl_consensus_fold_list": (C.c_int, [_P, C.POINTER(_P), _u64p]),
    "issl_consensus_fold_copy": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_consensus_finish": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_consensus_copy": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_consensus_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), _u64p]),
    "issl_consensus_selection_pages": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(_P), _u64p]),
    "issl_consensus_close": (C.c_int, [_P]),
    "issl_annotation_open": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "issl_annotation_open_file": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "issl_annotation_info": (C.c_int, [_P, _u64p, _u64p, _u64p, _u64p, _u64p]),
    "issl_annotation_seq": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "issl_annotation_lookup": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "issl_annotation_hits": (C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    "issl_annotation_hits_device": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P]),
    "issl_annotation_hits_occurrences_device": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P]),
    "issl_annotation_close": (C.c_int, [_P]),
    "issl_offtarget_landings": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_offtarget_landings_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "issl_offtarget_landing_profile": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P]),
    "issl_offtarget_landing_profile_device": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, _P, _P]),
    "issl_results_build": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t,
                                     C.POINTER(ResultsConfig), C.POINTER(_P)]),
    "issl_results_build_rows": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t,
                                          C.c_uint64, C.c_uint64, C.POINTER(ResultsConfig), C.POINTER(_P)]),
    "issl_results_info": (C.c_int, [_P, _u64p, _u64p, C.POINTER(C.c_uint32)]),
    "issl_results_times": (C.c_int, [_P, _f64p, _f64p, _f64p]),
    "issl_results_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "issl_results_copy": (C.c_int, [_P, _P, C.c_size_t]),
    "issl_results_write": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "issl_results_close": (C.c_int, [_P]),
    "issl_repr_f64_device": (C.c_int, [_P, C.c_size_t, _P, _P, _P]),
    "issl_folds_open": (C.c_int, [_P, C.POINTER(_P)]),
    "issl_folds_info": (C.c_int, [_P, _u64p, _u64p, _u64p, C.POINTER(C.c_uint32)]),
    "issl_folds_times": (C.c_int, [_P, _f64p, _f64p]),
    "issl_folds_input": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(_P), _u64p]),
    "issl_folds_input_copy": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_size_t]),
    "issl_folds_input_write": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_char_p]),
    "issl_folds_read": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t]),
    "issl_folds_read_file": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_char_p]),
    "issl_folds_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "issl_folds_text_device": (C.c_int, [_P, C.POINTER(_P), _u64p]),
    "issl_folds_copy": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "issl_folds_text_copy": (C.c_int, [_P, C.c_uint64, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "issl_folds_close": (C.c_int, [_P]),
    "issl_consensus_finish_folds": (C.c_int, [_P, _P]),
    "issl_results_build_rows_folds": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t, C.c_uint64, C.c_uint64,
                                                C.POINTER(ResultsConfig), C.POINTER(_P)]),
    "issl_runlog_batches": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, C.c_double, C.c_char_p, C.c_uint64, C.c_uint64,
                                      C.POINTER(_P)]),
    "issl_runlog_info": (C.c_int, [_P, _u64p, _u64p, _u64p, _f64p]),
    "issl_runlog_copy": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t]),
    "issl_runlog_close": (C.c_int, [_P]),
    "issl_node_create": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    "issl_node_score": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_double, C.c_int, _P, _P]),
    "issl_node_get_info": (C.c_int, [_P, C.POINTER(NodeInfo)]),
    "issl_node_shard_times": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]),
    "issl_node_close": (C.c_int, [_P]),
}
for _name, (_res, _args) in _protos.items():
    _fn = getattr(lib, _name)  # AttributeError here = library/header mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTS = tuple(_protos)


def check(rc):
    if rc != 0:
        raise IsslError(rc, lib.issl_last_error().decode(errors="replace"))
