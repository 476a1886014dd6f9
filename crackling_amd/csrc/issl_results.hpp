// The result table (issl_results_*, include/issl_hip.h) as its two units see each other: issl_results.cpp prepares the
// tables a row is written from, issl_results.hip measures and writes the rows.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/issl_hip.h"

namespace issl {

constexpr uint32_t kResultRows = 256;         // rows per workgroup, one thread each
constexpr uint32_t kResultStage = 48u * 1024; // bytes of a workgroup's staging buffer in LDS (+ 16 for the span's alignment):
                                              // three workgroups, twelve waves, on a CU's 160 KiB
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
enum ResultRule : uint32_t { kRuleNone, kRuleMit, kRuleCfd, kRuleAnd, kRuleOr, kRuleAvg };

// Everything a row is made of, device pointers.  Text fields are spans of `pool`, already quoted where CSV asks for it.
struct ResultArgs {
    const issl_guide *guides;
    const issl_consensus_row *rows;
    uint32_t first, n;              // the rows of the set the text holds: [first, first + n)
    const issl_text_span *headers;  // per record of the guide set
    const uint32_t *fold_of;        // per guide of the whole set: its place in the fold list / the selection / the scored rows, or kNoRow;
    const uint32_t *sel_of;         // null: no such stage
    const uint32_t *score_of;
    const issl_text_span *ss;       // three per fold
    const issl_occurrence *occ;     // per selected row
    const issl_text_span *chr;      // per record of the genome
    const double *mit, *cfd;        // per scored row
    const char *pool;
    const char *fold_text;          // null: the spans of `ss` lie in pool.  Otherwise they lie here, in the text of an issl_folds
                                    // as RNAfold printed it, and a row quotes what it copies (issl_results_build_rows_folds)
    double threshold;
    uint32_t n_headers, n_fold, n_sel, n_chr, n_scored; // the tables' lengths: an index beyond its table reads as '?'
    uint32_t rule, print_mit, print_cfd, no_sgrna;
    uint32_t fold_quote;            // with fold_text: the bits of a span's `reserved` (issl_folds_text.hpp) that ask for quotes under `delimiter`
    char delimiter;
};

// rule, print_mit and print_cfd of `a` from [offtargetscore] method as configured (issl_results.cpp; issl_runlog.hip counts by it).
void method_rules(const char *method, ResultArgs &a);

inline uint32_t result_groups(uint32_t n) { return (n + kResultRows - 1) / kResultRows; }

// inverse[list[i]] = i for i < n_list (inverse is n words of kNoRow before).
void launch_results_invert(const uint32_t *list, uint32_t n_list, uint32_t *inverse, uint32_t n, void *stream);
// offsets[j] = bytes of the group's rows ahead of row j; sums[g] = bytes of group g.
void launch_results_measure(const ResultArgs &a, uint64_t *offsets, uint64_t *sums, void *stream);
// sums[0 .. groups] -> where every group starts in the text, `first` for group 0; sums[groups] and offsets[n] = the text's length.
void launch_results_scan(uint64_t *sums, uint32_t groups, uint64_t first, uint64_t *offsets, uint32_t n, void *stream);
// The rows into text; offsets become offsets into the text.
void launch_results_emit(const ResultArgs &a, uint64_t *offsets, const uint64_t *sums, char *text, bool direct, void *stream);
void launch_repr(const double *values, size_t n, char *text, uint32_t *len, void *stream);

} // namespace issl
