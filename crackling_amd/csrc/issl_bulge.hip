// Genome search with DNA and RNA bulges beside the mismatches (issl_genome_search_bulges*, include/issl_hip.h): where a
// query binds when up to D bases of the site, or up to R bases of the query, pair with nothing.  The protocol, the text
// grid, the tile, the pattern test and the survivor queue are those of issl_search.hip; a piece has up to 2^19 queries.
//
//   count    k_bulge<kCount>, one launch per bulge b = -R..D (at most seven) with the SearchArgs of that b's pattern P':
//            the windows have L + b bases.  A lane holds one survivor's packed word t and the same word shifted by b
//            (a DNA bulge; for an RNA bulge the wave-uniform query is shifted instead: k_bulge<, kRna>); against the query
//            it forms A & B, the positions that differ at both shifts, whose count is a lower bound of the distance at
//            every break point (bulge_both, issl_search_text.hpp).  On random text the bound of a 20-mer lies near 11,
//            so the break points are walked for almost no comparison: a wave takes
//            kQueryGroup bounds, keeps their minimum and asks once per group whether any lane is within max_dist; only
//            then the group's queries are taken one by one, and only a query whose own ballot is non-zero walks the break
//            points -- incrementally, one bit of A in and one bit of B out per step (bulge_min)
//   emit     the same kernel, k_bulge<kEmit>: a row is one word query | text position | strand | b + R; all b of a piece
//            share one buffer and one cursor
//   sort     one radix sort over all b's words of the piece: query-major, then position, strand and bulge as a signed
//            number -- b + R ascends with b
//   offsets  k_search_offsets on the query field
//   finish   k_bulge_finish: one thread per row reads the window as text again and recomputes the minimum, its break
//            point, mism and site with the functions the hot loop's decision came from (bulge_row)
// The profile is k_bulge<kProfile>: counts[query][b + R][min dist], one atomic per wave, query and distance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"
#include "issl_search_device.hpp"
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
constexpr size_t kBulgePieceQueries = size_t(1) << 19; // 19 bits of query + 41 of position + 1 of strand + 3 of bulge = one word

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

    // -- every survivor against every query, as k_search walks them: a lane holds one survivor, a wave a quarter of the
    // queries
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q_lo = static_cast<uint32_t>(static_cast<uint64_t>(n) * wave / 4);
    const uint32_t q_hi = static_cast<uint32_t>(static_cast<uint64_t>(n) * (wave + 1) / 4);
    const uint32_t limit = a.max_dist;
    unsigned long long found = 0;             // kCount: the rows of this lane's survivors
    for (uint32_t j0 = 0; j0 < n_q && q_lo < q_hi; j0 += 64) {
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
            if (kMode == kEmit) {
                const uint32_t before = lanes_before(who);
                const int first = __ffsll(static_cast<unsigned long long>(who)) - 1;
                unsigned long long at = 0;
                if (static_cast<int>(lane) == first) at = atomicAdd(ctr + 1, static_cast<unsigned long long>(__popcll(who)));
                at = __shfl(at, first, 64) + before;
                if (hit && at < cap)
                    words[at] = (static_cast<uint64_t>(qi) << (pos_bits + 1 + kSlotBits)) | ((base + (tag >> 1)) << (1 + kSlotBits)) |
                                (static_cast<uint64_t>(tag & 1u) << kSlotBits) | ba.slot;
            } else {
                uint64_t left = who;
                while (left) { // one atomic per distance that occurs among the wave's rows
                    const int first = __ffsll(static_cast<unsigned long long>(left)) - 1;
                    const uint32_t d = __shfl(dist, first, 64);
                    const uint64_t same = __ballot(hit && dist == d);
                    if (static_cast<int>(lane) == first)
                        atomicAdd(&counts[(static_cast<uint64_t>(qi) * ba.slots + ba.slot) * (a.max_dist + 1) + d],
                                  static_cast<unsigned long long>(__popcll(same)));
                    left &= ~same;
                }
            }
        };
        // kQueryGroup queries come in with one wait, the group behind them is on its way (k_search's fetch); the group's
        // bounds share one comparison and one branch
        uint32_t qi = q_lo;
        if (q_hi - q_lo >= kQueryGroup) {
            QueryGroup next = *reinterpret_cast<const QueryGroup *>(q + qi);
            for (; qi + kQueryGroup <= q_hi; qi += kQueryGroup) {
                const QueryGroup group = next;
                if (qi + 2 * kQueryGroup <= q_hi) next = *reinterpret_cast<const QueryGroup *>(q + qi + kQueryGroup);
                uint32_t least = ~0u;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u)
                    least = min(least, bound(group.q[u]));
                if (!(__ballot(least <= limit) & live)) continue;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) walk(group.q[u], qi + u);
            }
        }
        for (; qi < q_hi; ++qi) walk(q[qi], qi);
        if (kMode == kCount && valid) found += mine;
    }
    if (kMode == kCount) {
        for (int d = 32; d > 0; d >>= 1) {
            windows += __shfl_down(windows, d, 64);
            found += __shfl_down(found, d, 64);
        }
        if (lane == 0) {
            if (found) atomicAdd(ctr, found);
            if (windows) atomicAdd(ctr + 3, static_cast<unsigned long long>(windows));
        }
        if (threadIdx.x == 0 && n_q) atomicAdd(ctr + 2, static_cast<unsigned long long>(n_q));
    }
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
    const uint64_t w = words[j];
    const uint32_t slot = static_cast<uint32_t>(w) & ((1u << kSlotBits) - 1);
    const uint32_t strand = static_cast<uint32_t>(w >> kSlotBits) & 1u;
    const uint64_t pos = (w >> (1 + kSlotBits)) & ((1ull << pos_bits) - 1);
    const uint32_t qi = static_cast<uint32_t>(w >> (pos_bits + 1 + kSlotBits));
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

bool nothing_to_search(const issl_genome *g, const BulgeCall &c, size_t n)
{
    bool any = false;
    for_each_launch(g, c, [&](const SearchArgs &, const BulgeArgs &) { any = true; });
    return n == 0 || !any;
}

struct BulgePiece {
    Arena hit;
    uint64_t n_words = 0;
    const uint64_t *words = nullptr; // sorted: query | text position | strand | b + R
};

// Everything of a piece of n <= 2^19 queries but the rows: d_offsets[0..n] = base + the piece's offsets.
int bulge_piece(const issl_genome *g, const BulgeCall &c, const issl_search_query *d_q, uint32_t n, uint64_t base, uint64_t *d_offsets,
                hipStream_t stream, BulgePiece &pc)
{
    StageTimer clock(g->timing, stream);
    DevBuf ctrb;
    HIP_TRY(hipMalloc(&ctrb.p, 64));
    unsigned long long *ctr = static_cast<unsigned long long *>(ctrb.p);
    HIP_TRY(hipMemsetAsync(ctr, 0, 64, stream));
    const uint8_t *d_seq = static_cast<const uint8_t *>(g->seq.p);
    const uint32_t blocks = text_blocks(g);
    for_each_launch(g, c, [&](const SearchArgs &a, const BulgeArgs &b) {
        launch_bulge<kCount>(b.r != 0, blocks, stream, d_seq, g->len, a, b, d_q, n, g->pos_bits, ctr,
                           static_cast<uint64_t *>(nullptr), 0ull, static_cast<unsigned long long *>(nullptr));
    });
    HIP_TRY(hipGetLastError());
    unsigned long long seen[4] = {};
    HIP_TRY(hipMemcpyAsync(seen, ctr, sizeof seen, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("count");
    pc.n_words = seen[0];
    if (pc.n_words > 0xFFFFFFFFull) return too_many(pc.n_words); // the radix passes place with 32-bit offsets
    const uint32_t shift = g->pos_bits + 1 + kSlotBits;
    if (pc.n_words) {
        Arena &ha = pc.hit;
        const size_t o_ha = ha.reserve(8 * pc.n_words), o_hb = ha.reserve(8 * pc.n_words),
                     o_hh = ha.reserve(4 * radix_hist_words(radix_sort_blocks(pc.n_words)));
        HIP_TRY(hipMalloc(&ha.buf.p, ha.size));
        uint64_t *ha_w = ha.at<uint64_t>(o_ha), *hb_w = ha.at<uint64_t>(o_hb);
        for_each_launch(g, c, [&](const SearchArgs &a, const BulgeArgs &b) {
            launch_bulge<kEmit>(b.r != 0, blocks, stream, d_seq, g->len, a, b, d_q, n, g->pos_bits, ctr, ha_w,
                               pc.n_words, static_cast<unsigned long long *>(nullptr));
        });
        clock.note("emit");
        pc.words = radix_sort_async(ha_w, hb_w, pc.n_words, 0, shift + bits_for(n), ha.at<uint32_t>(o_hh), stream);
        clock.note("sort");
    }
    hipLaunchKernelGGL(k_search_offsets, dim3(n / 256 + 1), dim3(256), 0, stream, pc.words, static_cast<uint32_t>(pc.n_words), shift, n,
                       base, d_offsets);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("offsets");
    if (g->timing)
        std::fprintf(stderr, "[issl bulges] %u queries, %u bulges:%s | windows %llu admitted %llu rows %llu\n", n, c.n_launches,
                     clock.line.c_str(), seen[3], seen[2], seen[0]);
    return ISSL_OK;
}

// The piece's rows to d_rows[0 .. pc.n_words).  Returns when they are written.
int bulge_finish(const issl_genome *g, const BulgeCall &c, const BulgePiece &pc, const issl_search_query *d_q, uint32_t q_base,
                 issl_bulge_hit *d_rows, hipStream_t stream)
{
    if (pc.n_words == 0) return ISSL_OK;
    StageTimer clock(g->timing, stream);
    const uint32_t total = static_cast<uint32_t>(pc.n_words);
    hipLaunchKernelGGL(k_bulge_finish, dim3((total + 255) / 256), dim3(256), 0, stream, pc.words, total,
                       static_cast<const uint8_t *>(g->seq.p), c.length, c.bg, c.max_dist, d_q, q_base,
                       static_cast<const uint64_t *>(g->starts.p), static_cast<uint32_t>(g->records.size()), g->pos_bits,
                       reinterpret_cast<uint64_t *>(d_rows));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("finish");
    if (g->timing) std::fprintf(stderr, "[issl bulges]%s\n", clock.line.c_str());
    return ISSL_OK;
}

// search_run of issl_search.hip for the bulged rows: queries and offsets in device memory; the rows go to device memory
// (`hits`) or, rows_to_host, piece by piece through a device buffer of the piece's size into host memory.
int bulge_run(issl_genome *g, const BulgeCall &c, const issl_search_query *d_q, size_t n, uint64_t *d_offsets, issl_bulge_hit *hits,
              bool rows_to_host, size_t cap, size_t *n_total, hipStream_t stream)
{
    *n_total = 0;
    if (nothing_to_search(g, c, n)) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8 * (n + 1), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    auto rows_of = [&](const BulgePiece &pc, size_t at, uint64_t base) -> int {
        if (!rows_to_host) return bulge_finish(g, c, pc, d_q + at, static_cast<uint32_t>(at), hits + base, stream);
        if (pc.n_words == 0) return ISSL_OK;
        DevBuf d_rows;
        HIP_TRY(hipMalloc(&d_rows.p, sizeof(issl_bulge_hit) * pc.n_words));
        if (int rc = bulge_finish(g, c, pc, d_q + at, static_cast<uint32_t>(at), static_cast<issl_bulge_hit *>(d_rows.p), stream)) return rc;
        HIP_TRY(hipMemcpy(hits + base, d_rows.p, sizeof(issl_bulge_hit) * pc.n_words, hipMemcpyDeviceToHost));
        return ISSL_OK;
    };
    // Counting pass over the pieces; a single piece is finished from what that pass left, several are run once more.
    std::vector<uint64_t> bases;
    uint64_t total = 0;
    for (size_t at = 0; at < n; at += kBulgePieceQueries) {
        const uint32_t cnt = static_cast<uint32_t>(std::min(kBulgePieceQueries, n - at));
        BulgePiece pc;
        bases.push_back(total);
        if (int rc = bulge_piece(g, c, d_q + at, cnt, total, d_offsets + at, stream, pc)) return rc;
        total += pc.n_words;
        if (total > 0xFFFFFFFFull) return too_many(total);
        if (n <= kBulgePieceQueries && hits && total <= cap)
            if (int rc = rows_of(pc, at, 0)) return rc;
    }
    *n_total = total;
    if (n <= kBulgePieceQueries || !hits || total > cap) return ISSL_OK;
    for (size_t at = 0, k = 0; at < n; at += kBulgePieceQueries, ++k) {
        const uint32_t cnt = static_cast<uint32_t>(std::min(kBulgePieceQueries, n - at));
        BulgePiece pc;
        if (int rc = bulge_piece(g, c, d_q + at, cnt, bases[k], d_offsets + at, stream, pc)) return rc;
        if (int rc = rows_of(pc, at, bases[k])) return rc;
    }
    return ISSL_OK;
}

size_t profile_bins(const BulgeCall &c) { return static_cast<size_t>(c.bg.max_rna + c.bg.max_dna + 1) * (c.max_dist + 1); }

int bulge_profile_run(issl_genome *g, const BulgeCall &c, const issl_search_query *d_q, size_t n, uint64_t *d_counts, hipStream_t stream)
{
    if (n == 0) return ISSL_OK;
    const size_t bins = profile_bins(c);
    HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * n * bins, stream));
    if (!nothing_to_search(g, c, n)) {
        StageTimer clock(g->timing, stream);
        for (size_t at = 0; at < n; at += kBulgePieceQueries) {
            const uint32_t cnt = static_cast<uint32_t>(std::min(kBulgePieceQueries, n - at));
            for_each_launch(g, c, [&](const SearchArgs &a, const BulgeArgs &b) {
                launch_bulge<kProfile>(b.r != 0, text_blocks(g), stream, static_cast<const uint8_t *>(g->seq.p),
                                   g->len, a, b, d_q + at, cnt, g->pos_bits, static_cast<unsigned long long *>(nullptr),
                                   static_cast<uint64_t *>(nullptr), 0ull, reinterpret_cast<unsigned long long *>(d_counts + at * bins));
            });
            HIP_TRY(hipGetLastError());
            clock.note("profile");
        }
        if (g->timing) std::fprintf(stderr, "[issl bulges] %zu queries:%s\n", n, clock.line.c_str());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return ISSL_OK;
}

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
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        issl::DevBuf d_q, d_offs;
        if (int rc = issl::upload_queries(g, queries, n, d_q)) return rc;
        HIP_TRY(hipMalloc(&d_offs.p, 8 * (n + 1)));
        if (int rc = issl::bulge_run(g, c, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_offs.p), hits, true, cap,
                                     n_total, nullptr))
            return rc;
        HIP_TRY(hipMemcpy(offsets, d_offs.p, 8 * (n + 1), hipMemcpyDeviceToHost));
        return ISSL_OK;
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
        HIP_TRY(hipSetDevice(g->device));
        return issl::bulge_run(g, c, d_queries, n, d_offsets, d_hits, false, cap, n_total, static_cast<hipStream_t>(stream));
    });
}

int issl_genome_search_bulges_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                      const issl_search_query *queries, size_t n, int max_dist, uint64_t *counts)
{
    if (!g || !pat || !bulges || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        if (n == 0) return ISSL_OK;
        issl::DevBuf d_q, d_counts;
        if (int rc = issl::upload_queries(g, queries, n, d_q)) return rc;
        const size_t bytes = 8 * n * issl::profile_bins(c);
        HIP_TRY(hipMalloc(&d_counts.p, bytes));
        if (int rc = issl::bulge_profile_run(g, c, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_counts.p), nullptr))
            return rc;
        HIP_TRY(hipMemcpy(counts, d_counts.p, bytes, hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

int issl_genome_search_bulges_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                             const issl_search_query *d_queries, size_t n, int max_dist, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || !bulges || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeCall c;
        if (int rc = issl::check_bulge_call(pat, bulges, max_dist, n, &c)) return rc;
        HIP_TRY(hipSetDevice(g->device));
        return issl::bulge_profile_run(g, c, d_queries, n, d_counts, static_cast<hipStream_t>(stream));
    });
}

} // extern "C"
