// Genome search: where a query binds with at most max_dist mismatches, for any PAM pattern and any length up to 32
// (issl_genome_search*, include/issl_hip.h).  No index: the resident text of a genome handle (issl_genome_handle.hpp) is
// compared with every query.
//
// One piece of up to 2^22 queries, everything on one stream, the protocol of issl_locate.hip:
//   count    k_search<kCount> on the text grid of k_match_* (4096 positions per 256-thread workgroup).  The tile and its
//            halo go to LDS as 2-bit codes and one validity bit per base, 16 bases per word; a thread cuts its 16 windows
//            out of three words, tests the pattern on both strands and keeps a bit per window-strand that passes.  The
//            survivors of the workgroup are compacted into an LDS queue of 13-bit tags (one wave scan and one LDS atomic
//            per wave), so that the comparison runs on full waves: a lane holds one survivor's packed word and walks
//            the queries, whose sig and care are wave-uniform and come through scalar loads, kQueryGroup of them per
//            load and one group ahead; each of the four waves takes all survivors against a quarter of the queries.
//            Hits are only counted
//   emit     the same kernel, k_search<kEmit>: a hit is one word query | text position | strand, room reserved with one
//            atomic per wave and query that has a hit.  The order in the buffer does not matter
//   sort     radix sort of the words over the bits in use: query-major, then position, then strand -- which is
//            (record, pos, strand), records being laid out in ascending order.  No two words are equal, so the sorted
//            buffer is the same on every run
//   offsets  k_search_offsets: query k's rows start at the first word of a query >= k (a binary search per query; a
//            query named twice is compared twice and owns its own rows, so there are no ranks to resolve)
//   finish   k_search_finish: one thread per row re-reads the window and writes site, mism, dist and the record
// The profile is k_search<kProfile>: one pass, a hit adds to counts[query][dist] with one atomic per wave, query and
// distance; no row exists anywhere.
// The host waits for the number of hit words (sizes the buffers of the sort) and for the end of a piece.
// pack16, the offsets kernel and the argument checks are issl_search_device.hpp's: issl_bulge.hip takes them too.
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

using search_text::kEven;
using search_text::admits;
using search_text::gather_even_bits;
using search_text::mismatches;
using search_text::reverse_complement;
using search_text::window_word;
constexpr size_t kPieceQueries = size_t(1) << 22;       // 22 bits of query + 41 of position + 1 of strand = one word

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

    // -- every survivor against every query: a lane holds one survivor.  Every wave walks all the survivors, 64 at a time,
    // against its quarter of the queries: the four waves end together whatever the number of survivors is (with a
    // quarter of the survivors each, 530 of them cost a workgroup three rounds where the other waves had two)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (uniform: the queries come through scalar loads)
    const uint32_t q_lo = static_cast<uint32_t>(static_cast<uint64_t>(n) * wave / 4);
    const uint32_t q_hi = static_cast<uint32_t>(static_cast<uint64_t>(n) * (wave + 1) / 4);
    unsigned long long found = 0; // kCount: the hits of this lane's survivors
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
            if (kMode == kEmit) {
                const uint32_t before = lanes_before(who);
                const int first = __ffsll(static_cast<unsigned long long>(who)) - 1;
                unsigned long long at = 0;
                if (static_cast<int>(lane) == first) at = atomicAdd(ctr + 1, static_cast<unsigned long long>(__popcll(who)));
                at = __shfl(at, first, 64) + before;
                if (hit && at < cap)
                    words[at] = (static_cast<uint64_t>(qi) << (pos_bits + 1)) | ((base + (tag >> 1)) << 1) | (tag & 1u);
            } else {
                uint64_t left = who;
                while (left) { // one atomic per distance that occurs among the wave's hits
                    const int first = __ffsll(static_cast<unsigned long long>(left)) - 1;
                    const uint32_t d = __shfl(dist, first, 64);
                    const uint64_t same = __ballot(hit && dist == d);
                    if (static_cast<int>(lane) == first)
                        atomicAdd(&counts[static_cast<uint64_t>(qi) * (a.max_dist + 1) + d], static_cast<unsigned long long>(__popcll(same)));
                    left &= ~same;
                }
            }
        };
        // kQueryGroup queries come in with one wait: a scalar load per query and a wait behind each left a wave idle for
        // the scalar cache's latency once per 11 vector instructions
        // the group behind the one being compared is on its way.  (Two groups ping-ponging in registers of their own
        // would save the scalar copies, but scalar loads return out of order: the wait for one group is a wait for
        // both, and the compiler put it right behind the younger load.)
        uint32_t qi = q_lo;
        if (q_hi - q_lo >= kQueryGroup) {
            QueryGroup next = *reinterpret_cast<const QueryGroup *>(q + qi);
            for (; qi + kQueryGroup <= q_hi; qi += kQueryGroup) {
                const QueryGroup group = next;
                if (qi + 2 * kQueryGroup <= q_hi) next = *reinterpret_cast<const QueryGroup *>(q + qi + kQueryGroup);
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) compare(group.q[u], qi + u);
            }
        }
        for (; qi < q_hi; ++qi) compare(q[qi], qi);
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

// Row j is sorted word j: the window is read again, as text.
__global__ __launch_bounds__(256) void k_search_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                       SearchArgs a, const issl_search_query *__restrict__ q, uint32_t q_base,
                                                       const uint64_t *__restrict__ starts, uint32_t n_records, uint32_t pos_bits,
                                                       uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t w = words[j];
    const uint32_t strand = static_cast<uint32_t>(w & 1u);
    const uint64_t pos = (w >> 1) & ((1ull << pos_bits) - 1);
    const uint32_t qi = static_cast<uint32_t>(w >> (pos_bits + 1));
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

// ---- host --------------------------------------------------------------------------------------------------------

bool nothing_to_search(const issl_genome *g, const SearchArgs &a, size_t n) { return n == 0 || g->len < a.length; }

struct SearchPiece {
    Arena hit;
    uint64_t n_words = 0;
    const uint64_t *words = nullptr; // sorted: query << (pos_bits + 1) | text position << 1 | strand
};

// Everything of a piece of n <= 2^22 queries but the rows: d_offsets[0..n] = base + the piece's offsets.
int search_piece(const issl_genome *g, const SearchArgs &a, const issl_search_query *d_q, uint32_t n, uint64_t base,
                 uint64_t *d_offsets, hipStream_t stream, SearchPiece &pc)
{
    StageTimer clock(g->timing, stream);
    DevBuf ctrb;
    HIP_TRY(hipMalloc(&ctrb.p, 64));
    unsigned long long *ctr = static_cast<unsigned long long *>(ctrb.p);
    HIP_TRY(hipMemsetAsync(ctr, 0, 64, stream));
    const uint8_t *d_seq = static_cast<const uint8_t *>(g->seq.p);
    const uint32_t blocks = text_blocks(g);
    hipLaunchKernelGGL(k_search<kCount>, dim3(blocks), dim3(256), 0, stream, d_seq, g->len, a, d_q, n, g->pos_bits, ctr,
                       static_cast<uint64_t *>(nullptr), 0ull, static_cast<unsigned long long *>(nullptr));
    HIP_TRY(hipGetLastError());
    unsigned long long seen[4] = {};
    HIP_TRY(hipMemcpyAsync(seen, ctr, sizeof seen, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("count");
    pc.n_words = seen[0];
    if (pc.n_words > 0xFFFFFFFFull) return too_many(pc.n_words); // the radix passes place with 32-bit offsets
    const uint32_t shift = g->pos_bits + 1;
    if (pc.n_words) {
        Arena &ha = pc.hit;
        const size_t o_ha = ha.reserve(8 * pc.n_words), o_hb = ha.reserve(8 * pc.n_words),
                     o_hh = ha.reserve(4 * radix_hist_words(radix_sort_blocks(pc.n_words)));
        HIP_TRY(hipMalloc(&ha.buf.p, ha.size));
        uint64_t *ha_w = ha.at<uint64_t>(o_ha), *hb_w = ha.at<uint64_t>(o_hb);
        hipLaunchKernelGGL(k_search<kEmit>, dim3(blocks), dim3(256), 0, stream, d_seq, g->len, a, d_q, n, g->pos_bits, ctr, ha_w,
                           pc.n_words, static_cast<unsigned long long *>(nullptr));
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
        std::fprintf(stderr, "[issl search] %u queries:%s | windows %llu admitted %llu hits %llu\n", n, clock.line.c_str(), seen[3],
                     seen[2], seen[0]);
    return ISSL_OK;
}

// The piece's rows to d_rows[0 .. pc.n_words).  Returns when they are written.
int search_finish(const issl_genome *g, const SearchArgs &a, const SearchPiece &pc, const issl_search_query *d_q, uint32_t q_base,
                  issl_search_hit *d_rows, hipStream_t stream)
{
    if (pc.n_words == 0) return ISSL_OK;
    StageTimer clock(g->timing, stream);
    const uint32_t total = static_cast<uint32_t>(pc.n_words);
    hipLaunchKernelGGL(k_search_finish, dim3((total + 255) / 256), dim3(256), 0, stream, pc.words, total,
                       static_cast<const uint8_t *>(g->seq.p), a, d_q, q_base, static_cast<const uint64_t *>(g->starts.p),
                       static_cast<uint32_t>(g->records.size()), g->pos_bits, reinterpret_cast<uint64_t *>(d_rows));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("finish");
    if (g->timing) std::fprintf(stderr, "[issl search]%s\n", clock.line.c_str());
    return ISSL_OK;
}

// Queries and offsets in device memory; the rows go to device memory (`hits`) or, rows_to_host, piece by piece through a
// device buffer of the piece's size into host memory.
int search_run(issl_genome *g, const SearchArgs &a, const issl_search_query *d_q, size_t n, uint64_t *d_offsets, issl_search_hit *hits,
               bool rows_to_host, size_t cap, size_t *n_total, hipStream_t stream)
{
    *n_total = 0;
    if (nothing_to_search(g, a, n)) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8 * (n + 1), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    auto rows_of = [&](const SearchPiece &pc, size_t at, uint64_t base) -> int {
        if (!rows_to_host) return search_finish(g, a, pc, d_q + at, static_cast<uint32_t>(at), hits + base, stream);
        if (pc.n_words == 0) return ISSL_OK;
        DevBuf d_rows;
        HIP_TRY(hipMalloc(&d_rows.p, sizeof(issl_search_hit) * pc.n_words));
        if (int rc = search_finish(g, a, pc, d_q + at, static_cast<uint32_t>(at), static_cast<issl_search_hit *>(d_rows.p), stream)) return rc;
        HIP_TRY(hipMemcpy(hits + base, d_rows.p, sizeof(issl_search_hit) * pc.n_words, hipMemcpyDeviceToHost));
        return ISSL_OK;
    };
    // Counting pass over the pieces; a single piece is finished from what that pass left, several are run once more.
    std::vector<uint64_t> bases;
    uint64_t total = 0;
    for (size_t at = 0; at < n; at += kPieceQueries) {
        const uint32_t cnt = static_cast<uint32_t>(std::min(kPieceQueries, n - at));
        SearchPiece pc;
        bases.push_back(total);
        if (int rc = search_piece(g, a, d_q + at, cnt, total, d_offsets + at, stream, pc)) return rc;
        total += pc.n_words;
        if (total > 0xFFFFFFFFull) return too_many(total);
        if (n <= kPieceQueries && hits && total <= cap)
            if (int rc = rows_of(pc, at, 0)) return rc;
    }
    *n_total = total;
    if (n <= kPieceQueries || !hits || total > cap) return ISSL_OK;
    for (size_t at = 0, k = 0; at < n; at += kPieceQueries, ++k) {
        const uint32_t cnt = static_cast<uint32_t>(std::min(kPieceQueries, n - at));
        SearchPiece pc;
        if (int rc = search_piece(g, a, d_q + at, cnt, bases[k], d_offsets + at, stream, pc)) return rc;
        if (int rc = rows_of(pc, at, bases[k])) return rc;
    }
    return ISSL_OK;
}

int profile_run(issl_genome *g, const SearchArgs &a, const issl_search_query *d_q, size_t n, uint64_t *d_counts, hipStream_t stream)
{
    if (n == 0) return ISSL_OK;
    const size_t bins = a.max_dist + 1;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * n * bins, stream));
    if (!nothing_to_search(g, a, n)) {
        StageTimer clock(g->timing, stream);
        for (size_t at = 0; at < n; at += kPieceQueries) {
            const uint32_t cnt = static_cast<uint32_t>(std::min(kPieceQueries, n - at));
            hipLaunchKernelGGL(k_search<kProfile>, dim3(text_blocks(g)), dim3(256), 0, stream, static_cast<const uint8_t *>(g->seq.p),
                               g->len, a, d_q + at, cnt, g->pos_bits, static_cast<unsigned long long *>(nullptr),
                               static_cast<uint64_t *>(nullptr), 0ull, reinterpret_cast<unsigned long long *>(d_counts + at * bins));
            HIP_TRY(hipGetLastError());
            clock.note("profile");
        }
        if (g->timing) std::fprintf(stderr, "[issl search] %zu queries:%s\n", n, clock.line.c_str());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return ISSL_OK;
}

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
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        issl::DevBuf d_q, d_offs;
        if (int rc = issl::upload_queries(g, queries, n, d_q)) return rc;
        HIP_TRY(hipMalloc(&d_offs.p, 8 * (n + 1)));
        if (int rc = issl::search_run(g, a, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_offs.p), hits, true,
                                      cap, n_total, nullptr))
            return rc;
        HIP_TRY(hipMemcpy(offsets, d_offs.p, 8 * (n + 1), hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

int issl_genome_search_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n, int max_dist,
                              uint64_t *d_offsets, issl_search_hit *d_hits, size_t cap, size_t *n_total, void *stream)
{
    if (!g || !pat || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        HIP_TRY(hipSetDevice(g->device));
        return issl::search_run(g, a, d_queries, n, d_offsets, d_hits, false, cap, n_total, static_cast<hipStream_t>(stream));
    });
}

int issl_genome_search_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                               uint64_t *counts)
{
    if (!g || !pat || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        if (n == 0) return ISSL_OK;
        issl::DevBuf d_q, d_counts;
        if (int rc = issl::upload_queries(g, queries, n, d_q)) return rc;
        const size_t bytes = 8 * n * (static_cast<size_t>(max_dist) + 1);
        HIP_TRY(hipMalloc(&d_counts.p, bytes));
        if (int rc = issl::profile_run(g, a, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_counts.p), nullptr))
            return rc;
        HIP_TRY(hipMemcpy(counts, d_counts.p, bytes, hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

int issl_genome_search_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                      int max_dist, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::SearchArgs a;
        if (int rc = issl::check_call(pat, max_dist, n, &a)) return rc;
        HIP_TRY(hipSetDevice(g->device));
        return issl::profile_run(g, a, d_queries, n, d_counts, static_cast<hipStream_t>(stream));
    });
}

} // extern "C"
