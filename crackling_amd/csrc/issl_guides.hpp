// The guide set behind issl_guides_* (issl_guides.hip makes it) as the stages that work on its rows in place see it
// (issl_consensus.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "issl_hiputil.hpp"

struct issl_guide_set {
    int device = -1;
    uint64_t n_guides = 0, n_unique = 0, n_matches = 0;
    issl::DevBuf guides, sigs; // issl_guide[n_guides], uint64_t[n_guides]; null when there is no guide
    std::vector<issl::FastaRecord> records;
    std::vector<uint64_t> file_starts;  // where every input's records start in the text, and the text's length
    std::vector<uint32_t> file_counts;  // per input: matches, those that met a guide seen before, guides met here for the
                                        // second time, guides met here first (issl_guides_file_counts)
};
