// What the two kernel units of the genome search share (issl_search.hip: mismatches only; issl_bulge.hip: DNA and RNA
// bulges beside them): the tile's 16-base words, the query group a wave fetches at once, the offsets kernel, and the checks
// every entry point makes before any device work.  Kernels and device functions live in an anonymous namespace, one copy
// per translation unit, like issl_radix.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
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

} // namespace
} // namespace issl
