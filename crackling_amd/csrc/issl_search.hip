// Genome search: where a query binds with at most max_dist mismatches, for any PAM pattern and any length up to 32
// (issl_genome_search*, include/issl_hip.h).  No index: the resident text of a genome handle (issl_genome_handle.hpp) is
// compared with every query.  The first unit of SearchDriver (issl_search_device.hpp: the host side, once for all units)
// with the protocol of issl_search_core.hpp -- count, emit, sort, offsets, finish, and the profile -- and that header's
// device pieces: the split of the queries over the waves, the sinks, the hit word, the kCount reduction.  This unit's
// own: k_search with the two-bit front (issl_bulge.hip has the same text; the core header says why it is no function),
// the walk over the queries and the comparison, one distance per survivor and query; a hit word with nothing below the
// strand; k_search_finish, which writes site, mism, dist and the record of a row.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_search_core.hpp"
#include "issl_search_text.hpp"

namespace issl {
namespace {

using search_text::kEven;
using search_text::admits;
using search_text::gather_even_bits;
using search_text::mismatches;
using search_text::reverse_complement;
using search_text::window_word;

// ctr[0]: hits; ctr[1]: the cursor of k_search<kEmit>; ctr[2]: window-strands the pattern admits; ctr[3]: windows of L
// bases A C G T (the figures of the timing line, kCount only).
template <int kMode>
__global__ __launch_bounds__(256) void k_search(const uint8_t *__restrict__ s, uint64_t len, SearchArgs a,
                                                const issl_search_query *__restrict__ q, uint32_t n, uint32_t pos_bits,
                                                unsigned long long *__restrict__ ctr, uint64_t *__restrict__ words, uint64_t cap,
                                                unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t codes[kTileWords], bads[kTileWords];
    __shared__ uint16_t queue[2 * kPosPerBlock]; // tag = position in the tile << 1 | strand
    __shared__ uint32_t q_count;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) q_count = 0;
    pack16(s, base + 16ull * threadIdx.x, len, codes[threadIdx.x], bads[threadIdx.x]);
    if (threadIdx.x < 2) pack16(s, base + kPosPerBlock + 16ull * threadIdx.x, len, codes[256 + threadIdx.x], bads[256 + threadIdx.x]);
    __syncthreads();
    const uint64_t in_mask = a.full | (a.full << 1);

    // -- the pattern on the thread's 16 windows, both strands: two bits per window
    uint32_t pass = 0, windows = 0;
    {
        const uint32_t w0 = codes[threadIdx.x], w1 = codes[threadIdx.x + 1], w2 = codes[threadIdx.x + 2];
        const uint64_t bad48 = bads[threadIdx.x] | (static_cast<uint64_t>(bads[threadIdx.x + 1]) << 16) |
                               (static_cast<uint64_t>(bads[threadIdx.x + 2]) << 32);
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            if (static_cast<uint32_t>(bad48 >> k) & a.win_mask) continue;
            ++windows;
            const uint64_t f = window_word(w0, w1, w2, k, in_mask);
            if (admits(a, f)) pass |= 1u << (2 * k);
            if (admits(a, reverse_complement(f, a.rev_shift))) pass |= 2u << (2 * k);
        }
    }
    // -- the survivors into the queue: a scan inside the wave, one LDS atomic per wave
    {
        const uint32_t cnt = static_cast<uint32_t>(__builtin_popcount(pass));
        uint32_t incl = cnt;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        uint32_t wave_base = 0;
        if (lane == 63 && incl) wave_base = atomicAdd(&q_count, incl);
        wave_base = __shfl(wave_base, 63, 64);
        uint32_t at = wave_base + incl - cnt;
        for (uint32_t m = pass; m; m &= m - 1) {
            const uint32_t bit = static_cast<uint32_t>(__builtin_ctz(m));
            queue[at++] = static_cast<uint16_t>(((threadIdx.x * 16 + (bit >> 1)) << 1) | (bit & 1u));
        }
    }
    __syncthreads();
    const uint32_t n_q = q_count;

    // -- every survivor against every query: a lane holds one survivor, a wave its quarter of the queries
    const QueryRange mine_q = wave_queries(n);
    unsigned long long found = 0; // kCount: the hits of this lane's survivors
    for (uint32_t j0 = 0; j0 < n_q && mine_q.lo < mine_q.hi; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool valid = j < n_q;
        uint32_t tag = 0;
        uint64_t t = 0;
        if (valid) {
            tag = queue[j];
            const uint32_t p = tag >> 1, wi = p >> 4;
            const uint64_t f = window_word(codes[wi], codes[wi + 1], codes[wi + 2], p & 15u, in_mask);
            t = (tag & 1u) ? reverse_complement(f, a.rev_shift) : f;
        }
        const uint64_t live = __ballot(valid);
        uint32_t mine = 0; // kCount: at most 2^22 hits of this lane's survivor
        // one query against the wave's survivors; everything about the query is wave-uniform
        auto compare = [&](const issl_search_query &one, uint32_t qi) {
            const uint32_t dist = search_text::distance(t, one.sig, one.care & ~kEven);
            if (kMode == kCount) { // a lane counts its own hits: no scalar instruction per comparison but the care mask
                mine += dist <= a.max_dist ? 1u : 0u;
                return;
            }
            const uint64_t who = __ballot(dist <= a.max_dist) & live; // (no branch around the lanes without a survivor)
            if (!who) return;
            const bool hit = (who >> lane) & 1u;
            if (kMode == kEmit) emit_hits<0>(who, hit, lane, ctr, words, cap, qi, pos_bits, base, tag, 0);
            else profile_hits(who, hit, dist, lane, counts, qi, a.max_dist + 1);
        };
        // kQueryGroup queries come in with one wait: a scalar load per query and a wait behind each left a wave idle for
        // the scalar cache's latency once per 11 vector instructions
        // the group behind the one being compared is on its way.  (Two groups ping-ponging in registers of their own
        // would save the scalar copies, but scalar loads return out of order: the wait for one group is a wait for
        // both, and the compiler put it right behind the younger load.)
        uint32_t qi = mine_q.lo;
        if (mine_q.hi - mine_q.lo >= kQueryGroup) {
            QueryGroup next = *reinterpret_cast<const QueryGroup *>(q + qi);
            for (; qi + kQueryGroup <= mine_q.hi; qi += kQueryGroup) {
                const QueryGroup group = next;
                if (qi + 2 * kQueryGroup <= mine_q.hi) next = *reinterpret_cast<const QueryGroup *>(q + qi + kQueryGroup);
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) compare(group.q[u], qi + u);
            }
        }
        for (; qi < mine_q.hi; ++qi) compare(q[qi], qi);
        if (kMode == kCount && valid) found += mine;
    }
    if (kMode == kCount) count_totals(windows, found, n_q, lane, ctr);
}

// Row j is sorted word j: the window is read again, as text.
__global__ __launch_bounds__(256) void k_search_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                       SearchArgs a, const issl_search_query *__restrict__ q, uint32_t q_base,
                                                       const uint64_t *__restrict__ starts, uint32_t n_records, uint32_t pos_bits,
                                                       uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    uint32_t qi, strand, low;
    uint64_t pos;
    decode_hit<0>(words[j], pos_bits, qi, pos, strand, low);
    uint64_t f = 0;
    for (uint32_t i = 0; i < a.length; ++i) f |= static_cast<uint64_t>(base_code(s[pos + i]) & 3u) << (2 * i);
    const uint64_t t = strand ? reverse_complement(f, a.rev_shift) : f;
    const uint64_t m = mismatches(t, q[qi].sig, q[qi].care & kEven);
    const uint32_t rec = last_not_above(starts, n_records, pos);
    uint64_t *row = rows + 4ull * j; // issl_search_hit: site, pos, record | query, mism | strand | dist | reserved
    row[0] = t;
    row[1] = pos - starts[rec];
    row[2] = rec | (static_cast<uint64_t>(q_base + qi) << 32);
    row[3] = gather_even_bits(m) | (static_cast<uint64_t>(strand) << 32) | (static_cast<uint64_t>(__popcll(m)) << 40);
}

// ---- host: the unit as SearchDriver takes it (issl_search_device.hpp) ----------------------------------------------------

struct PlainSearch {
    using Row = issl_search_hit;
    using Call = SearchArgs;
    static constexpr size_t kPieceQueries = size_t(1) << 22; // 22 bits of query + 41 of position + 1 of strand = one word
    static constexpr uint32_t kLowBits = 0;
    static constexpr const char *kTag = "[issl search]", *kRows = "hits";
    static std::string counted(const Call &) { return ""; }
    static bool nothing(const issl_genome *g, const Call &a, size_t n) { return n == 0 || g->len < a.length; }
    static size_t bins(const Call &a) { return a.max_dist + 1; }
    static size_t scratch_bytes(const Call &, size_t) { return 0; }

    template <int kMode>
    static void launch(const issl_genome *g, const Call &a, const issl_search_query *d_q, uint32_t n, void *, unsigned long long *ctr,
                       uint64_t *words, uint64_t cap, unsigned long long *counts, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_search<kMode>, dim3(text_blocks(g)), dim3(256), 0, stream, static_cast<const uint8_t *>(g->seq.p), g->len, a, d_q,
                           n, g->pos_bits, ctr, words, cap, counts);
    }

    static void finish(const issl_genome *g, const Call &a, const uint64_t *words, uint32_t total, const issl_search_query *d_q,
                       uint32_t q_base, uint64_t *rows, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_search_finish, dim3((total + 255) / 256), dim3(256), 0, stream, words, total,
                           static_cast<const uint8_t *>(g->seq.p), a, d_q, q_base, static_cast<const uint64_t *>(g->starts.p),
                           static_cast<uint32_t>(g->records.size()), g->pos_bits, rows);
    }
};
using Plain = SearchDriver<PlainSearch>;

} // namespace
} // namespace issl

extern "C" {

int issl_search_prepare(const char *pattern, const char *queries, size_t n, size_t stride, issl_search_pattern *pat,
                        issl_search_query *out)
{
    return issl::abi_call([&]() -> int {
        std::string err;
        if (issl::search_text::prepare(pattern, queries, n, stride, pat, out, err)) return ISSL_OK;
        issl::set_error(err);
        return ISSL_E_ARG;
    });
}

int issl_genome_search(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                       uint64_t *offsets, issl_search_hit *hits, size_t cap, size_t *n_total)
{
    if (!g || !pat || (!queries && n) || !offsets || !n_total || (!hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        return issl::Plain::host_rows(g, a, pat->length, queries, n, offsets, hits, cap, n_total);
    });
}

int issl_genome_search_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n, int max_dist,
                              uint64_t *d_offsets, issl_search_hit *d_hits, size_t cap, size_t *n_total, void *stream)
{
    if (!g || !pat || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        return issl::Plain::device_rows(g, a, d_queries, n, d_offsets, d_hits, cap, n_total, stream);
    });
}

int issl_genome_search_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                               uint64_t *counts)
{
    if (!g || !pat || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        return issl::Plain::host_profile(g, a, pat->length, queries, n, counts);
    });
}

int issl_genome_search_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                      int max_dist, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        return issl::Plain::device_profile(g, a, d_queries, n, d_counts, stream);
    });
}

} // extern "C"
