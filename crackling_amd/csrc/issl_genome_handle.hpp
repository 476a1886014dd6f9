// The handle of a genome resident on the GPU (issl_locate.hip makes it; issl_occur.hip and issl_transcripts.hip read it),
// apart from the query preparation of issl_genome.hpp, which only the units that scan the text need.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_hiputil.hpp"

struct issl_genome {
    int device = -1;
    uint64_t len = 0;     // bytes of text, separators included
    uint64_t n_bases = 0; // sum of the records' lengths
    uint32_t pos_bits = 1; // bits of a text position
    bool timing = false;  // ISSL_LOCATE_TIMING=1, read when the handle is made: one stderr line per stage of a call
    issl::DevBuf seq, starts;
    std::vector<issl::FastaRecord> records;
};

