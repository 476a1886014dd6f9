// Genome search with DNA and RNA bulges beside the mismatches (issl_genome_search_bulges*, include/issl_hip.h): where a
// query binds when up to D bases of the site, or up to R bases of the query, pair with nothing.  The second unit of
// SearchDriver (issl_search_device.hpp) with the protocol and the device pieces of issl_search_core.hpp.  Tile, pattern
// test and survivor queue are k_search's text for windows of L + b bases (the core header says why they are no
// function).  A piece has up to 2^19 queries.  This unit's own:
//   count    k_bulge<kCount>, one launch per bulge b = -R..D (at most seven) with the SearchArgs of that b's pattern P'.
//            A lane holds one survivor's packed word t and the same word shifted by b
//            (a DNA bulge; for an RNA bulge the wave-uniform query is shifted instead: k_bulge<, kRna>); against the query
//            it forms A & B, the positions that differ at both shifts, whose count is a lower bound of the distance at
//            every break point (bulge_both, issl_search_text.hpp).  On random text the bound of a 20-mer lies near 11,
//            so the break points are walked for almost no comparison: a wave takes
//            kQueryGroup bounds, keeps their minimum and asks once per group whether any lane is within max_dist; only
//            then the group's queries are taken one by one, and only a query whose own ballot is non-zero walks the break
//            points -- incrementally, one bit of A in and one bit of B out per step (bulge_min)
//   emit     a row is one word query | text position | strand | b + R; all b of a piece share one buffer and one cursor,
//            so one sort orders a query's rows by position, strand and bulge as a signed number -- b + R ascends with b
//   finish   k_bulge_finish: one thread per row reads the window as text again and recomputes the minimum, its break
//            point, mism and site with the functions the hot loop's decision came from (bulge_row)
//   profile  counts[query][b + R][min dist]
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

using search_text::BulgeArgs;
using search_text::kEven;
using search_text::admits;
using search_text::mismatches;
using search_text::reverse_complement;
using search_text::window_word;
constexpr uint32_t kSlotBits = 3;                  // b + R: 0..6

static_assert(sizeof(issl_search_bulges) == 16 && sizeof(issl_bulge_hit) == 32, "the layouts of include/issl_hip.h");

// ctr[0]: rows; ctr[1]: the cursor of k_bulge<kEmit>; ctr[2]: window-strands the patterns admit; ctr[3]: windows of
// A C G T, summed over the launches of a piece (the figures of the timing line, kCount only).
template <int kMode, bool kRna>
__global__ __launch_bounds__(256) void k_bulge(const uint8_t *__restrict__ s, uint64_t len, SearchArgs a, BulgeArgs ba,
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

    // -- the pattern P' on the thread's 16 windows of L + b bases, both strands: two bits per window
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
    const QueryRange mine_q = wave_queries(n);
    const uint32_t limit = a.max_dist;
    unsigned long long found = 0; // kCount: the rows of this lane's survivors
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
        const uint64_t tq = search_text::bulge_shift(t, ba.b);      // what query position j meets right of the break point
        const uint64_t tb = search_text::bulge_bound_text(t, ba.b); // the bound's second word: site coordinates for an RNA bulge
        // the bound of one query; for an RNA bulge two scalar shifts and one scalar AND more per query
        auto bound = [&](const issl_search_query &one) {
            if (!kRna) return search_text::bulge_both(t, tb, one.sig, one.sig, one.care & ~kEven);
            return search_text::bulge_both(t, tb, one.sig, search_text::bulge_bound_query(one.sig, ba.r),
                                           one.care & search_text::bulge_bound_query(one.care, ba.r) & ~kEven);
        };
        const uint64_t live = __ballot(valid);
        uint32_t mine = 0; // kCount
        // one query whose bound some lane meets: the break points, for the whole wave (the masks are wave-uniform)
        auto walk = [&](const issl_search_query &one, uint32_t qi) {
            if (!(__ballot(bound(one) <= limit) & live)) return;
            uint32_t brk;
            const uint32_t dist = search_text::bulge_min(mismatches(t, one.sig, one.care & kEven), mismatches(tq, one.sig, one.care & kEven), ba, brk);
            const bool hit = valid && dist <= a.max_dist;
            if (kMode == kCount) {
                mine += hit ? 1u : 0u;
                return;
            }
            const uint64_t who = __ballot(hit);
            if (!who) return;
            if (kMode == kEmit) emit_hits<kSlotBits>(who, hit, lane, ctr, words, cap, qi, pos_bits, base, tag, ba.slot);
            else profile_hits(who, hit, dist, lane, counts, static_cast<uint64_t>(qi) * ba.slots + ba.slot, a.max_dist + 1);
        };
        // the group's bounds share one comparison and one branch
        uint32_t qi = mine_q.lo;
        if (mine_q.hi - mine_q.lo >= kQueryGroup) {
            QueryGroup next = *reinterpret_cast<const QueryGroup *>(q + qi);
            for (; qi + kQueryGroup <= mine_q.hi; qi += kQueryGroup) {
                const QueryGroup group = next;
                if (qi + 2 * kQueryGroup <= mine_q.hi) next = *reinterpret_cast<const QueryGroup *>(q + qi + kQueryGroup);
                uint32_t least = ~0u;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) least = min(least, bound(group.q[u]));
                if (!(__ballot(least <= limit) & live)) continue;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) walk(group.q[u], qi + u);
            }
        }
        for (; qi < mine_q.hi; ++qi) walk(q[qi], qi);
        if (kMode == kCount && valid) found += mine;
    }
    if (kMode == kCount) count_totals(windows, found, n_q, lane, ctr);
}

// Row j is sorted word j: the window of L + b bases is read again, as text.
__global__ __launch_bounds__(256) void k_bulge_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                      uint32_t length, issl_search_bulges bg, uint32_t max_dist,
                                                      const issl_search_query *__restrict__ q, uint32_t q_base,
                                                      const uint64_t *__restrict__ starts, uint32_t n_records, uint32_t pos_bits,
                                                      uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    uint32_t qi, strand, slot;
    uint64_t pos;
    decode_hit<kSlotBits>(words[j], pos_bits, qi, pos, strand, slot);
    const int32_t b = static_cast<int32_t>(slot) - static_cast<int32_t>(bg.max_rna);
    const uint32_t window = static_cast<uint32_t>(static_cast<int32_t>(length) + b);
    uint64_t f = 0;
    for (uint32_t i = 0; i < window; ++i) f |= static_cast<uint64_t>(base_code(s[pos + i]) & 3u) << (2 * i);
    const uint64_t t = strand ? reverse_complement(f, 64 - 2 * window) : f;
    uint32_t dist, at, mism;
    (void)search_text::bulge_row(t, q[qi], search_text::make_bulge_args(bg, b), max_dist, dist, at, mism);
    const uint32_t rec = last_not_above(starts, n_records, pos);
    uint64_t *row = rows + 4ull * j; // issl_bulge_hit: site, pos, record | query, mism | strand | dist | bulge | at
    row[0] = t;
    row[1] = pos - starts[rec];
    row[2] = rec | (static_cast<uint64_t>(q_base + qi) << 32);
    row[3] = mism | (static_cast<uint64_t>(strand) << 32) | (static_cast<uint64_t>(dist) << 40) |
             (static_cast<uint64_t>(static_cast<uint8_t>(b)) << 48) | (static_cast<uint64_t>(at) << 56);
}

// ---- host --------------------------------------------------------------------------------------------------------

// k_bulge<kMode, kRna> on the text grid.
template <int kMode, class... Args> void launch_bulge(bool rna, uint32_t blocks, hipStream_t stream, Args... args)
{
    if (rna) hipLaunchKernelGGL((k_bulge<kMode, true>), dim3(blocks), dim3(256), 0, stream, args...);
    else hipLaunchKernelGGL((k_bulge<kMode, false>), dim3(blocks), dim3(256), 0, stream, args...);
}

// One call: the launches of its b, in ascending order.
struct BulgeCall {
    issl_search_bulges bg{};
    uint32_t length = 0, max_dist = 0, n_launches = 0;
    SearchArgs a[7];
    BulgeArgs b[7];
};

// The launches whose window fits the text.
template <class F> void for_each_launch(const issl_genome *g, const BulgeCall &c, F &&f)
{
    for (uint32_t k = 0; k < c.n_launches; ++k)
        if (g->len >= c.a[k].length) f(c.a[k], c.b[k]);
}

// The unit as SearchDriver takes it (issl_search_device.hpp): the launches of b where the plain search has one, three bits
// of b + R below the strand.
struct BulgeSearch {
    using Row = issl_bulge_hit;
    using Call = BulgeCall;
    static constexpr size_t kPieceQueries = size_t(1) << 19; // 19 bits of query + 41 of position + 1 of strand + 3 of bulge = one word
    static constexpr uint32_t kLowBits = kSlotBits;
    static constexpr const char *kTag = "[issl bulges]", *kRows = "rows";
    static std::string counted(const Call &c) { return ", " + std::to_string(c.n_launches) + " bulges"; }
    static bool nothing(const issl_genome *g, const Call &c, size_t n)
    {
        bool any = false;
        for_each_launch(g, c, [&](const SearchArgs &, const BulgeArgs &) { any = true; });
        return n == 0 || !any;
    }
    static size_t bins(const Call &c) { return static_cast<size_t>(c.bg.max_rna + c.bg.max_dna + 1) * (c.max_dist + 1); }
    static size_t scratch_bytes(const Call &, size_t) { return 0; }

    template <int kMode>
    static void launch(const issl_genome *g, const Call &c, const issl_search_query *d_q, uint32_t n, void *, unsigned long long *ctr,
                       uint64_t *words, uint64_t cap, unsigned long long *counts, hipStream_t stream)
    {
        for_each_launch(g, c, [&](const SearchArgs &a, const BulgeArgs &b) {
            launch_bulge<kMode>(b.r != 0, text_blocks(g), stream, static_cast<const uint8_t *>(g->seq.p), g->len, a, b, d_q, n, g->pos_bits, ctr,
                                words, cap, counts);
        });
    }

    static void finish(const issl_genome *g, const Call &c, const uint64_t *words, uint32_t total, const issl_search_query *d_q,
                       uint32_t q_base, uint64_t *rows, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_bulge_finish, dim3((total + 255) / 256), dim3(256), 0, stream, words, total,
                           static_cast<const uint8_t *>(g->seq.p), c.length, c.bg, c.max_dist, d_q, q_base,
                           static_cast<const uint64_t *>(g->starts.p), static_cast<uint32_t>(g->records.size()), g->pos_bits, rows);
    }
};
using Bulged = SearchDriver<BulgeSearch>;

// The checks every entry point makes before any device work.  ISSL_OK: *c holds the launches.
int check_bulge_call(const issl_search_pattern *pat, const issl_search_bulges *bg, int max_dist, size_t n, BulgeCall *c)
{
    SearchArgs plain;
    if (int rc = check_call(pat, max_dist, n, &plain)) return rc;
    std::string err;
    if (!search_text::check_bulges(pat, bg, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    c->bg = *bg;
    c->length = pat->length;
    c->max_dist = static_cast<uint32_t>(max_dist);
    c->n_launches = 0;
    for (int32_t b = -static_cast<int32_t>(bg->max_rna); b <= static_cast<int32_t>(bg->max_dna); ++b) {
        c->a[c->n_launches] = search_text::make_args(search_text::bulge_pattern(*pat, *bg, b), max_dist);
        c->b[c->n_launches++] = search_text::make_bulge_args(*bg, b);
    }
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_genome_search_bulges(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                              const issl_search_query *queries, size_t n, int max_dist, uint64_t *offsets, issl_bulge_hit *hits, size_t cap,
                              size_t *n_total)
{
    if (!g || !pat || !bulges || (!queries && n) || !offsets || !n_total || (!hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        return issl::Bulged::host_rows(g, c, pat->length, queries, n, offsets, hits, cap, n_total);
    });
}

int issl_genome_search_bulges_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                     const issl_search_query *d_queries, size_t n, int max_dist, uint64_t *d_offsets,
                                     issl_bulge_hit *d_hits, size_t cap, size_t *n_total, void *stream)
{
    if (!g || !pat || !bulges || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap))
        return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        return issl::Bulged::device_rows(g, c, d_queries, n, d_offsets, d_hits, cap, n_total, stream);
    });
}

int issl_genome_search_bulges_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                      const issl_search_query *queries, size_t n, int max_dist, uint64_t *counts)
{
    if (!g || !pat || !bulges || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        return issl::Bulged::host_profile(g, c, pat->length, queries, n, counts);
    });
}

int issl_genome_search_bulges_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                             const issl_search_query *d_queries, size_t n, int max_dist, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || !bulges || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        return issl::Bulged::device_profile(g, c, d_queries, n, d_counts, stream);
    });
}

} // extern "C"
