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

namespace issl {

// A handle's records as the arrays the readers of VCF, SNPs and indels take (issl_variants_text.hpp,
// issl_haplotypes_text.hpp).  The names point into the handle.
struct RecordTable {
    std::vector<const char *> names;
    std::vector<size_t> name_lens;
    std::vector<uint64_t> starts, lengths;
    explicit RecordTable(const issl_genome *g)
    {
        for (const FastaRecord &r : g->records) {
            names.push_back(r.name.data());
            name_lens.push_back(r.name.size());
            starts.push_back(r.start);
            lengths.push_back(r.length);
        }
    }
    size_t size() const { return starts.size(); }
};

} // namespace issl

