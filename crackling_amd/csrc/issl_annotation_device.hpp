// The resident annotation as its device code sees it (issl_transcripts.hip builds and queries it; issl_landing.hip asks
// it once per landing): the handle, the view of its breakpoints and answers, the query, and the table that names the
// annotation's sequence of every record of a genome.  Device functions live in an anonymous namespace, one copy per
// translation unit, like issl_match.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <unordered_map>

#include "../../include/issl_hip.h"
#include "issl_annotation.hpp"
#include "issl_genome_handle.hpp"

struct issl_annotation {
    int device = -1;
    issl::AnnotationTables t; // exons released after the build
    std::unordered_map<std::string, uint32_t> seq_index;
    uint64_t n_exons = 0, n_bp = 0, n_segments = 0;
    issl::DevBuf bp, seq_first, answers; // n_bp keys, n_seqs + 1 indices, n_bp rows
};

namespace issl {

// The sequence of every record of the genome under the name Bowtie2 gives it -- the header from its first non-blank
// character up to the next blank, not '.'->'_' translated -- and, in entry n_records, of '*'; 0xFFFFFFFF where the
// annotation lacks the name.  n_records + 1 words in the memory of the current device, there when the call returns.
int record_sequences(const issl_annotation *a, const issl_genome *g, DevBuf &d_rec_seq);

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// First index in a[lo, hi) with a[i] >= x (hi when there is none).
__device__ __forceinline__ uint32_t first_not_below(const uint64_t *__restrict__ a, uint32_t lo, uint32_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct View {
    const uint64_t *bp;
    const uint32_t *seq_first;
    const uint4 *answers;
    uint32_t n_seqs;
};

inline View view_of(const issl_annotation *a)
{
    return View{static_cast<const uint64_t *>(a->bp.p), static_cast<const uint32_t *>(a->seq_first.p),
                static_cast<const uint4 *>(a->answers.p), static_cast<uint32_t>(a->t.seqs.size())};
}

// The answer row {hit, total, status, first} of (sequence, start): issl_annotation_hits' rule for one query.
__device__ __forceinline__ uint4 answer_at(const View &v, uint32_t seq, long long start)
{
    const uint4 none = make_uint4(0u, 0u, 0u, kNone);
    if (seq >= v.n_seqs || start < 0) return none;
    const uint64_t top = (uint64_t(1) << kCoordBits) - 1; // beyond every breakpoint
    const uint64_t coord = static_cast<uint64_t>(start) < top ? static_cast<uint64_t>(start) : top;
    const uint64_t key = (static_cast<uint64_t>(seq) << kCoordBits) | coord;
    const uint32_t b = v.seq_first[seq], e = v.seq_first[seq + 1];
    const uint32_t ub = first_not_below(v.bp, b, e, key + 1); // first breakpoint above the position
    return ub == b ? none : v.answers[ub - 1];
}

} // namespace
} // namespace issl
