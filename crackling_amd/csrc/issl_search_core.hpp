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
// What is not in here although the kernels have it: the tile front (pack16 loads, pattern test, compaction), the
// survivor's fetch, the walk over the query groups and the kCount reduction.  The compiler finishes a function before it
// inlines it, and each of these came back with operands of commutative instructions swapped or two instructions in the
// other order (profiles/search_core_isa.txt); they stay written out until the kernels may change.
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
