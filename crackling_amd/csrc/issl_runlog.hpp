// The counts of the run's log (issl_runlog_*, include/issl_hip.h) as its units see each other: issl_runlog.hip counts over
// the rows the stages left on the device; issl_consensus.hip lends the consensus' arrays.
#pragma once
#include <cstdint>

#include "../../include/issl_hip.h"

namespace issl {

// What a finished consensus lends: its rows, its two lists and [consensus] n.
struct RunlogSource {
    int device;
    bool finished;
    uint32_t n;                    // guides of the set
    uint32_t consensus_n;          // [consensus] n
    const issl_consensus_row *rows;
    const uint32_t *fold_list;
    uint64_t n_fold;
    const uint32_t *selection;
    uint64_t n_selected;
};
RunlogSource consensus_runlog_source(const issl_consensus *c);

} // namespace issl
