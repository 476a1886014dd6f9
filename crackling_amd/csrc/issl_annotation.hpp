// GFF3 annotation -> the flat tables behind issl_annotation (include/issl_hip.h, "transcript hit counts"): the host half
// of the counterpart of src/crackling/utils/countHitTranscripts.py, loadAnnotation (:45-146).  Plain C++, no device call:
// a malformed file is ISSL_E_FORMAT whether or not a GPU is present.  issl_transcripts.hip builds the device form.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace issl {

constexpr uint32_t kNoGene = 0xFFFFFFFFu;
constexpr uint32_t kCoordBits = 40;                           // a breakpoint key is seq << 40 | coordinate
constexpr int64_t kMaxCoord = (int64_t(1) << kCoordBits) - 2; // end + 1 still fits
constexpr uint64_t kMaxSeqs = uint64_t(1) << 24;

struct AnnotationExon {
    uint32_t seq, transcript; // transcript: ordinal among all transcripts of the annotation
    int64_t start, end;       // as the file gives them: start > end is kept and contains nothing
};

// Sequences in order of first appearance on a counted line (names with '.' -> '_').  Transcripts in order of first
// appearance of (sequence, ID) -- an mRNA line's ID or an exon line's Parent -- so the transcripts of one sequence stand
// in the reference's order for that sequence; the same ID on two sequences is two transcripts.  Genes: the distinct
// Parents of mRNA lines, each with the number of mRNA lines that name it (duplicates included).  tr_gene: the Parent of the
// FIRST mRNA line anywhere in the file with the transcript's ID, kNoGene when there is none.
struct AnnotationTables {
    std::vector<std::string> seqs;
    std::vector<uint32_t> tr_seq, tr_gene;
    std::vector<uint32_t> gene_count;
    std::vector<AnnotationExon> exons;
};

// ISSL_OK, or ISSL_E_FORMAT with the line in the message where the reference would stop with a traceback.
int parse_annotation(const char *text, size_t len, AnnotationTables &out);

// The exons as the device wants them: per transcript a set of DISJOINT closed intervals with the same union as its exons
// (start > end dropped, an end below 0 dropped, a start below 0 raised to 0; overlapping and duplicate exons of one
// transcript merged), as keys lo[i] = seq << 40 | start, hi[i] = seq << 40 | (end + 1), with the transcript in tr[i].
// ISSL_E_UNSUPPORTED for a coordinate above 2^40 - 2, for 2^24 sequences or more and for 2^31 intervals or more.
struct AnnotationIntervals {
    std::vector<uint64_t> lo, hi;
    std::vector<uint32_t> tr;
};
int annotation_intervals(const AnnotationTables &t, AnnotationIntervals &out);

// Optional sign and ASCII digits within int64 (Python's int() takes more: blanks, underscores, other digits, any size).
bool parse_int64(const char *s, size_t n, int64_t &v);

} // namespace issl
