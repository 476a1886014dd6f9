// What the kernel units of the genome search share (issl_search.hip: mismatches only; issl_bulge.hip: DNA and RNA
// bulges beside them; issl_variants.hip: IUPAC codes in the text; issl_bulge_variants.hip: both) beside the device pieces of issl_search_core.hpp: the tile's 16-base words, the query group a wave
// fetches at once, the offsets kernel, the checks every entry point makes before any device work, and the host driver of
// a unit (SearchDriver: pieces, rows, profile, the bodies of the entry points).  Kernels and device functions live in an
// anonymous namespace, one copy per translation unit, like issl_radix.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"
#include "issl_search_text.hpp"

namespace issl {
namespace {

using search_text::SearchArgs;
constexpr uint32_t kTileWords = kPosPerBlock / 16 + 2; // 16 bases per word; the halo of up to 31 bases is two more words
constexpr uint32_t kQueryGroup = 4;                     // queries a wave fetches at once (64 bytes of scalar loads)
struct QueryGroup { issl_search_query q[kQueryGroup]; };
enum Mode { kCount = 0, kEmit = 1, kProfile = 2 };

static_assert(sizeof(issl_search_pattern) == 32 && sizeof(issl_search_query) == 16 && sizeof(issl_search_hit) == 32,
              "the layouts of include/issl_hip.h");
static_assert(kPosPerBlock == 256 * 16, "a thread owns the 16 windows that start in its word");

// 16 bytes of text at `at` (a multiple of 16) -> 2-bit codes and one bit per base that is not A C G T; what lies behind
// the text is such a base.
__device__ __forceinline__ void pack16(const uint8_t *__restrict__ s, uint64_t at, uint64_t len, uint32_t &code, uint32_t &bad)
{
    code = 0;
    bad = 0;
    if (at + 16 <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(s + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t c = base_code(static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3))));
            code |= (c & 3u) << (2 * i);
            bad |= (c >> 2) << i;
        }
    } else {
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t c = at + i < len ? base_code(s[at + i]) : 4u;
            code |= (c & 3u) << (2 * i);
            bad |= (c >> 2) << i;
        }
    }
}

// out[k] = base + the first sorted word of a query >= k, for k = 0..n.
__global__ __launch_bounds__(256) void k_search_offsets(const uint64_t *__restrict__ words, uint32_t n_words, uint32_t shift, uint32_t n,
                                                        uint64_t base, uint64_t *__restrict__ out)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k > n) return;
    uint32_t lo = 0, hi = n_words;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((words[mid] >> shift) < k) lo = mid + 1;
        else hi = mid;
    }
    out[k] = base + lo;
}

// ---- host --------------------------------------------------------------------------------------------------------

inline int too_many(uint64_t hits)
{
    set_error("more than 2^32 - 1 hits in one call (" + std::to_string(hits) + "): split the query or lower max_dist");
    return ISSL_E_UNSUPPORTED;
}

inline uint32_t text_blocks(const issl_genome *g) { return static_cast<uint32_t>((g->len + kPosPerBlock - 1) / kPosPerBlock); }

// The checks every entry point makes before any device work.  ISSL_OK: *a is what the kernels take.
inline int check_call(const issl_search_pattern *pat, int max_dist, size_t n, SearchArgs *a)
{
    std::string err;
    if (!search_text::check_pattern(pat, max_dist, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    if (n > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 queries in one call");
        return ISSL_E_UNSUPPORTED;
    }
    *a = search_text::make_args(*pat, max_dist);
    return ISSL_OK;
}

inline int check_host_queries(const issl_search_query *queries, size_t n, uint32_t length)
{
    std::string err;
    if (search_text::check_queries(queries, n, length, err)) return ISSL_OK;
    set_error(err);
    return ISSL_E_ARG;
}

// Host queries -> device memory of the handle.
inline int upload_queries(issl_genome *g, const issl_search_query *queries, size_t n, DevBuf &d_q)
{
    HIP_TRY(hipSetDevice(g->device));
    if (n == 0) return ISSL_OK;
    HIP_TRY(hipMalloc(&d_q.p, sizeof(issl_search_query) * n));
    HIP_TRY(hipMemcpy(d_q.p, queries, sizeof(issl_search_query) * n, hipMemcpyHostToDevice));
    return ISSL_OK;
}

// ---- the driver of a unit ------------------------------------------------------------------------------------------
// The host side of the protocol (issl_search_core.hpp), once for every unit.  A unit describes itself with a struct U:
//   Row, Call              the row type; what a checked call carries to the launches (SearchArgs, BulgeCall, VariantArgs,
//                          BulgeVariantCall)
//   kPieceQueries          queries per piece;  kLowBits: the bits of the hit word below the strand
//   kTag, kRows            "[issl search]" / "hits" of the timing lines;  counted(c): what follows "N queries" there
//   nothing(g, c, n)       is there nothing to search
//   scratch_bytes(c, n)    device memory a piece of n queries needs beside its queries, 0 for none: the driver allocates
//                          it once per call for the largest piece and hands it to every launch
//   launch<kMode>(g, c, d_q, n, scratch, ctr, words, cap, counts, stream)   enqueue the count / emit / profile launches of a piece
//   finish(g, c, words, total, d_q, q_base, rows, stream)          enqueue the finish kernel
//   bins(c)                counts per query of the profile

struct SearchPiece {
    Arena hit;
    uint64_t n_words = 0;
    const uint64_t *words = nullptr; // sorted: query | text position | strand | the unit's low bits
};

template <class U> struct SearchDriver {
    using Call = typename U::Call;
    using Row = typename U::Row;

    // Everything of a piece of n <= kPieceQueries queries but the rows: d_offsets[0..n] = base + the piece's offsets.
    static int piece(const issl_genome *g, const Call &c, const issl_search_query *d_q, uint32_t n, void *scratch, uint64_t base,
                     uint64_t *d_offsets, hipStream_t stream, SearchPiece &pc)
    {
        StageTimer clock(g->timing, stream);
        DevBuf ctrb;
        HIP_TRY(hipMalloc(&ctrb.p, 64));
        unsigned long long *ctr = static_cast<unsigned long long *>(ctrb.p);
        HIP_TRY(hipMemsetAsync(ctr, 0, 64, stream));
        U::template launch<kCount>(g, c, d_q, n, scratch, ctr, nullptr, 0, nullptr, stream);
        HIP_TRY(hipGetLastError());
        unsigned long long seen[4] = {};
        HIP_TRY(hipMemcpyAsync(seen, ctr, sizeof seen, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        clock.note("count");
        pc.n_words = seen[0];
        if (pc.n_words > 0xFFFFFFFFull) return too_many(pc.n_words); // the radix passes place with 32-bit offsets
        const uint32_t shift = g->pos_bits + 1 + U::kLowBits;
        if (pc.n_words) {
            Arena &ha = pc.hit;
            const size_t o_ha = ha.reserve(8 * pc.n_words), o_hb = ha.reserve(8 * pc.n_words),
                         o_hh = ha.reserve(4 * radix_hist_words(radix_sort_blocks(pc.n_words)));
            HIP_TRY(hipMalloc(&ha.buf.p, ha.size));
            uint64_t *ha_w = ha.at<uint64_t>(o_ha), *hb_w = ha.at<uint64_t>(o_hb);
            U::template launch<kEmit>(g, c, d_q, n, scratch, ctr, ha_w, pc.n_words, nullptr, stream);
            clock.note("emit");
            pc.words = radix_sort_async(ha_w, hb_w, pc.n_words, 0, shift + bits_for(n), ha.at<uint32_t>(o_hh), stream);
            clock.note("sort");
        }
        hipLaunchKernelGGL(k_search_offsets, dim3(n / 256 + 1), dim3(256), 0, stream, pc.words, static_cast<uint32_t>(pc.n_words), shift,
                           n, base, d_offsets);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        clock.note("offsets");
        if (g->timing)
            std::fprintf(stderr, "%s %u queries%s:%s | windows %llu admitted %llu %s %llu\n", U::kTag, n, U::counted(c).c_str(),
                         clock.line.c_str(), seen[3], seen[2], U::kRows, seen[0]);
        return ISSL_OK;
    }

    // The scratch of the call's largest piece, on the handle's device, which the caller has made current.
    static int piece_scratch(const Call &c, size_t n, DevBuf &buf)
    {
        const size_t bytes = U::scratch_bytes(c, std::min(n, U::kPieceQueries));
        if (bytes) HIP_TRY(hipMalloc(&buf.p, bytes));
        return ISSL_OK;
    }

    // The piece's rows to d_rows[0 .. pc.n_words).  Returns when they are written.
    static int finish(const issl_genome *g, const Call &c, const SearchPiece &pc, const issl_search_query *d_q, uint32_t q_base,
                      Row *d_rows, hipStream_t stream)
    {
        if (pc.n_words == 0) return ISSL_OK;
        StageTimer clock(g->timing, stream);
        U::finish(g, c, pc.words, static_cast<uint32_t>(pc.n_words), d_q, q_base, reinterpret_cast<uint64_t *>(d_rows), stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        clock.note("finish");
        if (g->timing) std::fprintf(stderr, "%s%s\n", U::kTag, clock.line.c_str());
        return ISSL_OK;
    }

    // Queries and offsets in device memory; the rows go to device memory (`hits`) or, rows_to_host, piece by piece through
    // a device buffer of the piece's size into host memory.
    static int run(issl_genome *g, const Call &c, const issl_search_query *d_q, size_t n, uint64_t *d_offsets, Row *hits, bool rows_to_host,
                   size_t cap, size_t *n_total, hipStream_t stream)
    {
        constexpr size_t kPiece = U::kPieceQueries;
        *n_total = 0;
        if (U::nothing(g, c, n)) {
            HIP_TRY(hipMemsetAsync(d_offsets, 0, 8 * (n + 1), stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return ISSL_OK;
        }
        DevBuf scratch;
        if (int rc = piece_scratch(c, n, scratch)) return rc;
        auto rows_of = [&](const SearchPiece &pc, size_t at, uint64_t base) -> int {
            if (!rows_to_host) return finish(g, c, pc, d_q + at, static_cast<uint32_t>(at), hits + base, stream);
            if (pc.n_words == 0) return ISSL_OK;
            DevBuf d_rows;
            HIP_TRY(hipMalloc(&d_rows.p, sizeof(Row) * pc.n_words));
            if (int rc = finish(g, c, pc, d_q + at, static_cast<uint32_t>(at), static_cast<Row *>(d_rows.p), stream)) return rc;
            HIP_TRY(hipMemcpy(hits + base, d_rows.p, sizeof(Row) * pc.n_words, hipMemcpyDeviceToHost));
            return ISSL_OK;
        };
        // Counting pass over the pieces; a single piece is finished from what that pass left, several are run once more.
        std::vector<uint64_t> bases;
        uint64_t total = 0;
        for (size_t at = 0; at < n; at += kPiece) {
            const uint32_t cnt = static_cast<uint32_t>(std::min(kPiece, n - at));
            SearchPiece pc;
            bases.push_back(total);
            if (int rc = piece(g, c, d_q + at, cnt, scratch.p, total, d_offsets + at, stream, pc)) return rc;
            total += pc.n_words;
            if (total > 0xFFFFFFFFull) return too_many(total);
            if (n <= kPiece && hits && total <= cap)
                if (int rc = rows_of(pc, at, 0)) return rc;
        }
        *n_total = total;
        if (n <= kPiece || !hits || total > cap) return ISSL_OK;
        for (size_t at = 0, k = 0; at < n; at += kPiece, ++k) {
            const uint32_t cnt = static_cast<uint32_t>(std::min(kPiece, n - at));
            SearchPiece pc;
            if (int rc = piece(g, c, d_q + at, cnt, scratch.p, bases[k], d_offsets + at, stream, pc)) return rc;
            if (int rc = rows_of(pc, at, bases[k])) return rc;
        }
        return ISSL_OK;
    }

    static int profile_run(issl_genome *g, const Call &c, const issl_search_query *d_q, size_t n, uint64_t *d_counts, hipStream_t stream)
    {
        constexpr size_t kPiece = U::kPieceQueries;
        if (n == 0) return ISSL_OK;
        const size_t bins = U::bins(c);
        HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * n * bins, stream));
        DevBuf scratch; // until the launches have run
        if (!U::nothing(g, c, n)) {
            if (int rc = piece_scratch(c, n, scratch)) return rc;
            StageTimer clock(g->timing, stream);
            for (size_t at = 0; at < n; at += kPiece) {
                const uint32_t cnt = static_cast<uint32_t>(std::min(kPiece, n - at));
                U::template launch<kProfile>(g, c, d_q + at, cnt, scratch.p, nullptr, nullptr, 0,
                                             reinterpret_cast<unsigned long long *>(d_counts + at * bins), stream);
                HIP_TRY(hipGetLastError());
                clock.note("profile");
            }
            if (g->timing) std::fprintf(stderr, "%s %zu queries:%s\n", U::kTag, n, clock.line.c_str());
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }

    // The bodies of a unit's four entry points, behind its null-argument check and its check of the call.
    static int host_rows(issl_genome *g, const Call &c, uint32_t length, const issl_search_query *queries, size_t n, uint64_t *offsets,
                         Row *hits, size_t cap, size_t *n_total)
    {
        if (int rc = check_host_queries(queries, n, length)) return rc;
        DevBuf d_q, d_offs;
        if (int rc = upload_queries(g, queries, n, d_q)) return rc;
        HIP_TRY(hipMalloc(&d_offs.p, 8 * (n + 1)));
        if (int rc = run(g, c, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_offs.p), hits, true, cap, n_total,
                         nullptr))
            return rc;
        HIP_TRY(hipMemcpy(offsets, d_offs.p, 8 * (n + 1), hipMemcpyDeviceToHost));
        return ISSL_OK;
    }

    static int device_rows(issl_genome *g, const Call &c, const issl_search_query *d_queries, size_t n, uint64_t *d_offsets, Row *d_hits,
                           size_t cap, size_t *n_total, void *stream)
    {
        HIP_TRY(hipSetDevice(g->device));
        return run(g, c, d_queries, n, d_offsets, d_hits, false, cap, n_total, static_cast<hipStream_t>(stream));
    }

    static int host_profile(issl_genome *g, const Call &c, uint32_t length, const issl_search_query *queries, size_t n, uint64_t *counts)
    {
        if (int rc = check_host_queries(queries, n, length)) return rc;
        if (n == 0) return ISSL_OK;
        DevBuf d_q, d_counts;
        if (int rc = upload_queries(g, queries, n, d_q)) return rc;
        const size_t bytes = 8 * n * U::bins(c);
        HIP_TRY(hipMalloc(&d_counts.p, bytes));
        if (int rc = profile_run(g, c, static_cast<const issl_search_query *>(d_q.p), n, static_cast<uint64_t *>(d_counts.p), nullptr)) return rc;
        HIP_TRY(hipMemcpy(counts, d_counts.p, bytes, hipMemcpyDeviceToHost));
        return ISSL_OK;
    }

    static int device_profile(issl_genome *g, const Call &c, const issl_search_query *d_queries, size_t n, uint64_t *d_counts, void *stream)
    {
        HIP_TRY(hipSetDevice(g->device));
        return profile_run(g, c, d_queries, n, d_counts, static_cast<hipStream_t>(stream));
    }
};

} // namespace
} // namespace issl
