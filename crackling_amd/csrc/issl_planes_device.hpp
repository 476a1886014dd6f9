// The front of the two kernels that read the text as sets of bases (k_variants, issl_variants.hip; k_bulge_variants,
// issl_bulge_variants.hip), beside issl_search_core.hpp and in its idiom: __device__ __forceinline__ in an anonymous
// namespace, the LDS arrays declared in the kernels and taken by reference.  The tile goes to LDS as four planes (A C G T;
// plane b bit i: base b is in the set of text position i) and a validity bit per position, 32 positions per word; a window
// is four words cut out with a funnel shift; the pattern is four plane masks, and strand 1 is tested on the forward window
// with the reversed, complemented pattern, so no window is reversed in the front.  The plane arithmetic is
// issl_variants_text.hpp's, which tools/variants_sanitize.cpp checks on the CPU.
#pragma once
#include "issl_search_core.hpp"
#include "issl_variants_text.hpp"

namespace issl {
namespace {

namespace vt = variants_text;
using vt::Planes;
using vt::VariantArgs;

constexpr uint32_t kPlaneWords = kPosPerBlock / 32 + 1; // 32 positions per word; the halo of up to 31 is one more word
struct PlaneGroup { Planes q[kQueryGroup]; };            // what a wave fetches at once, as QueryGroup
static_assert(sizeof(Planes) == 16, "a query as planes is the 16 bytes of issl_search_query");

// 16 bytes of text at `at` (a multiple of 16) -> 16 bits of every plane and one bit per byte that is none of the 14
// codes; what lies behind the text is such a byte.
__device__ __forceinline__ void planes16(const uint8_t *__restrict__ s, uint64_t at, uint64_t len, uint32_t (&plane)[4], uint32_t &bad)
{
    plane[0] = plane[1] = plane[2] = plane[3] = 0;
    bad = 0;
    uint32_t w[4] = {0, 0, 0, 0}; // (a zero byte is no code)
    if (at + 16 <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(s + at);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        for (uint32_t i = 0; i < 16; ++i)
            if (at + i < len) w[i >> 2] |= static_cast<uint32_t>(s[at + i]) << (8 * (i & 3));
    }
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t set = vt::text_set(static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3))));
        plane[0] |= (set & 1u) << i;
        plane[1] |= (set >> 1 & 1u) << i;
        plane[2] |= (set >> 2 & 1u) << i;
        plane[3] |= (set >> 3) << i;
        bad |= (set ? 0u : 1u) << i;
    }
}

// 16 positions of the tile: tile[b] is plane b, tile[4] the validity bits, as 32-bit words of which this is 16-bit half
// `half`.  A kernel calls it for its thread's 16 positions and, in the first two threads, for the halo's; its
// __syncthreads() follows.  (Both calls inside one function cost k_variants three registers, 63 to 66: the compiler
// finishes that function before it inlines it.)
__device__ __forceinline__ void fill_planes16(const uint8_t *__restrict__ s, uint64_t at, uint64_t len, uint32_t (&tile)[5][kPlaneWords], uint32_t half)
{
    uint32_t plane[4], bad;
    planes16(s, at, len, plane, bad);
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) reinterpret_cast<uint16_t *>(tile[b])[half] = static_cast<uint16_t>(plane[b]);
    reinterpret_cast<uint16_t *>(tile[4])[half] = static_cast<uint16_t>(bad);
}

// The pattern on the thread's 16 windows, both strands: pass holds two bits per window, windows counts those of codes
// alone with at most max_variants ambiguous positions.
__device__ __forceinline__ void test_plane_windows(const VariantArgs &a, const uint32_t (&tile)[5][kPlaneWords], uint32_t &pass, uint32_t &windows)
{
    pass = 0, windows = 0;
    const uint32_t wi = threadIdx.x >> 1, s0 = (threadIdx.x & 1u) << 4;
    uint32_t lo[5], hi[5];
#pragma unroll
    for (uint32_t b = 0; b < 5; ++b) lo[b] = tile[b][wi], hi[b] = tile[b][wi + 1];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (vt::funnel(lo[4], hi[4], s0 + k) & a.win_mask) continue;
        const Planes f{{vt::funnel(lo[0], hi[0], s0 + k) & a.win_mask, vt::funnel(lo[1], hi[1], s0 + k) & a.win_mask,
                        vt::funnel(lo[2], hi[2], s0 + k) & a.win_mask, vt::funnel(lo[3], hi[3], s0 + k) & a.win_mask}};
        if (static_cast<uint32_t>(__builtin_popcount(vt::ambiguous(f))) > a.max_variants) continue;
        ++windows;
        if (vt::admits(f, a.allow, a.win_mask)) pass |= 1u << (2 * k);
        if (vt::admits(f, a.allow_rc, a.win_mask)) pass |= 2u << (2 * k);
    }
}

// What the strand of the survivor `tag` reads, cut by the pattern.
__device__ __forceinline__ Planes survivor_planes(uint32_t tag, const uint32_t (&tile)[5][kPlaneWords], const VariantArgs &a)
{
    const uint32_t p = tag >> 1, wi = p >> 5, sh = p & 31u;
    const Planes f{{vt::funnel(tile[0][wi], tile[0][wi + 1], sh) & a.win_mask, vt::funnel(tile[1][wi], tile[1][wi + 1], sh) & a.win_mask,
                    vt::funnel(tile[2][wi], tile[2][wi + 1], sh) & a.win_mask, vt::funnel(tile[3][wi], tile[3][wi + 1], sh) & a.win_mask}};
    return vt::intersect((tag & 1u) ? vt::strand1(f, a.rev_shift) : f, a.allow);
}

} // namespace
} // namespace issl
