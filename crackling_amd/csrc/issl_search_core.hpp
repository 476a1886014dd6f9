// The text-search core of the index-free genome search: the protocol that k_search (issl_search.hip: mismatches only),
// k_bulge (issl_bulge.hip: DNA and RNA bulges beside them), k_variants (issl_variants.hip: IUPAC codes in the text as
// sets of bases, on bit planes in place of the 2-bit codes below) and k_bulge_variants (issl_bulge_variants.hip: the
// bulges on those bit planes) follow, and the device pieces they share, __device__
// __forceinline__ in an anonymous namespace, one copy per translation unit, like issl_radix.hpp.
//
// One piece of queries (2^22 of them, less the low bits a unit adds to its hit word), everything on one stream, the
// protocol of issl_locate.hip; the host side is SearchDriver (issl_search_device.hpp):
//   count    the unit's kernel, kCount, on the text grid of k_match_* (4096 positions per 256-thread workgroup).  The tile
//            and its halo go to LDS as 2-bit codes and one validity bit per base, 16 bases per word; a thread cuts its 16
//            windows out of three words, tests the pattern on both strands and keeps a bit per window-strand that passes.
//            The survivors of the workgroup are compacted into an LDS queue of 13-bit tags (one wave scan and one LDS
//            atomic per wave), so that the comparison runs on full waves: a lane holds one survivor's packed word and
//            walks the queries, whose sig and care are wave-uniform and come through scalar loads, kQueryGroup of them per
//            load and one group ahead; each of the four waves takes all survivors against a quarter of the queries
//            (wave_queries).  Hits are only counted
//   emit     the same kernel, kEmit: a hit is one word query | text position | strand | the unit's low field, room reserved
//            with one atomic per wave and query that has a hit (emit_hits).  The order in the buffer does not matter
//   sort     radix sort of the words over the bits in use: query-major, then position, strand and the low field -- which
//            is (record, pos, strand, ..), records being laid out in ascending order.  No two words are equal, so the
//            sorted buffer is the same on every run
//   offsets  k_search_offsets: query k's rows start at the first word of a query >= k (a binary search per query; a
//            query named twice is compared twice and owns its own rows, so there are no ranks to resolve)
//   finish   the unit's finish kernel: one thread per row re-reads the window as text and writes the row
// The profile is the same kernel, kProfile: one pass, a hit adds to the counts of its query with one atomic per wave, query
// and distance (profile_hits); no row exists anywhere.
// The host waits for the number of hit words (sizes the buffers of the sort) and for the end of a piece.
//
// What is shared and what is not.  Shared: the split of the queries over the waves (wave_queries), the kCount reduction
// (count_totals) and the hit word both ways (emit_hits, decode_hit) in all four kernels; the compaction
// (queue_survivors) in the two plane kernels, whose whole front is one copy in issl_planes_device.hpp.  The LDS arrays
// stay declared in the kernels and come in by reference: one __shared__ struct around them moved their offsets and cost
// k_variants instructions and a register.  As functions the pieces do not come back instruction for instruction (the
// operands of commutative instructions swap, v_or3 becomes two v_or), so the bar is that of
// profiles/search_core_isa.txt: the loops over the query groups hold the same instructions, registers, scratch and LDS
// are what they were, and so is the time (profiles/search_fold_ab.json).
// Not shared, with the reason:
//   the two-bit front of k_search and k_bulge (pattern test on the 16 windows, compaction, survivor fetch) is written
//   out in both kernels, the same text.  With test_windows(), queue_survivors() and survivor_word() in its place every
//   loop kept its opcodes and every register count, and the count stage got faster, but the emit stage of 10 000 queries
//   on 200 Mbp went from 72.3 to 73.3 ms in k_search and from 936.3 to 938.3 ms in k_bulge (D = R = 2), outside the
//   parent's spread of 0.3 and 0.8 ms.  The compaction alone as a function still changes 119 lines of k_search<kEmit>;
//   written out, k_search<kEmit | kProfile> and k_bulge<kEmit | kProfile, *> are the parent's text
//   the two calls that fill a tile and its halo: wrapped into one function they cost k_variants three registers, 63 to
//   66, beyond the 64 that eight waves per SIMD allow
//   the walk over the query groups and what it calls (the lambdas compare, bound and walk): it is the hot loop; it has two
//   shapes (compare each query: k_search, k_variants; the group's bound first: k_bulge, k_bulge_variants) over two query
//   types, and as a function taking the lambdas it is as much text as the loops of eight lines it would replace
#pragma once
#include "issl_search_device.hpp"

namespace issl {
namespace {

// The queries of this wave: every wave walks all the survivors, 64 at a time, against its quarter of the queries, so the
// four waves end together whatever the number of survivors is (with a quarter of the survivors each, 530 of them cost a
// workgroup three rounds where the other waves had two).  (Uniform: the queries come through scalar loads.)
struct QueryRange { uint32_t lo, hi; };
__device__ __forceinline__ QueryRange wave_queries(uint32_t n)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return {static_cast<uint32_t>(static_cast<uint64_t>(n) * wave / 4), static_cast<uint32_t>(static_cast<uint64_t>(n) * (wave + 1) / 4)};
}

// The survivors of the workgroup into the queue: bit 2k + strand of `pass` is window k of the thread's 16, its tag the
// position in the tile << 1 | strand.  A scan inside the wave and one LDS atomic per wave; q_count is valid behind the
// caller's __syncthreads().
__device__ __forceinline__ void queue_survivors(uint32_t pass, uint32_t lane, uint16_t (&queue)[2 * kPosPerBlock], uint32_t &q_count)
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

// kCount, at the end of the workgroup: ctr[0] += the hits its lanes found, ctr[3] += the windows they tested, ctr[2] +=
// the survivors of the tile; one atomic per wave and figure that is not zero.
__device__ __forceinline__ void count_totals(uint32_t windows, unsigned long long found, uint32_t n_q, uint32_t lane,
                                             unsigned long long *__restrict__ ctr)
{
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

// kEmit: the hits `who` of the wave against query qi, one word each, query | text position | strand | low (kLowBits
// wide; base: the text position of the tile, tag: the survivor's).  Room from the cursor ctr[1] with one atomic per wave; a
// word behind cap is dropped.
template <uint32_t kLowBits>
__device__ __forceinline__ void emit_hits(uint64_t who, bool hit, uint32_t lane, unsigned long long *__restrict__ ctr,
                                          uint64_t *__restrict__ words, uint64_t cap, uint32_t qi, uint32_t pos_bits, uint64_t base,
                                          uint32_t tag, uint32_t low)
{
    const uint32_t before = lanes_before(who);
    const int first = __ffsll(static_cast<unsigned long long>(who)) - 1;
    unsigned long long at = 0;
    if (static_cast<int>(lane) == first) at = atomicAdd(ctr + 1, static_cast<unsigned long long>(__popcll(who)));
    at = __shfl(at, first, 64) + before;
    if (hit && at < cap)
        words[at] = (static_cast<uint64_t>(qi) << (pos_bits + 1 + kLowBits)) | ((base + (tag >> 1)) << (1 + kLowBits)) |
                    (static_cast<uint64_t>(tag & 1u) << kLowBits) | low;
}

// The finish kernels: what emit_hits put into the word w, the position as a text position.
template <uint32_t kLowBits>
__device__ __forceinline__ void decode_hit(uint64_t w, uint32_t pos_bits, uint32_t &qi, uint64_t &pos, uint32_t &strand, uint32_t &low)
{
    low = static_cast<uint32_t>(w) & ((1u << kLowBits) - 1);
    strand = static_cast<uint32_t>(w >> kLowBits) & 1u;
    pos = (w >> (1 + kLowBits)) & ((1ull << pos_bits) - 1);
    qi = static_cast<uint32_t>(w >> (pos_bits + 1 + kLowBits));
}

// kProfile: counts[row * bins + dist] += the wave's hits at that distance, one atomic per distance that occurs among
// them.
__device__ __forceinline__ void profile_hits(uint64_t who, bool hit, uint32_t dist, uint32_t lane, unsigned long long *__restrict__ counts,
                                             uint64_t row, uint32_t bins)
{
    uint64_t left = who;
    while (left) {
        const int first = __ffsll(static_cast<unsigned long long>(left)) - 1;
        const uint32_t d = __shfl(dist, first, 64);
        const uint64_t same = __ballot(hit && dist == d);
        if (static_cast<int>(lane) == first)
            atomicAdd(&counts[row * bins + d], static_cast<unsigned long long>(__popcll(same)));
        left &= ~same;
    }
}

} // namespace
} // namespace issl
