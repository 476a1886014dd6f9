// What the units on a resident genome share (issl_locate.hip: locations of sites; issl_occur.hip: the Bowtie step;
// issl_landing.hip: off-target landings): the handle, a piece of locate's scan as it stands before its finish, and the
// preparation of a piece of query sites -- signatures -> text-order keys, sorted with their query index,
// runs of equal keys collapsed to ranks, one bit per distinct key in a bitmap -- with the probe the scan of the text
// asks.  Kernels and device functions live in an anonymous namespace, one copy per translation unit, like issl_match.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_match.hpp"

namespace issl {

// ---- a piece of issl_locate.hip, for the units that join its hits with something else (issl_landing.hip) -----------
// What locate_prepare leaves behind for the finish of a piece: query i of the piece owns the hit words
// words[rstart[qrank[i]] .. + offs[i + 1] - offs[i]), sorted by (position, strand), and the piece's locations
// offs[i] .. offs[i + 1) of `total`.  The arenas own the memory; it lives as long as the Piece.
struct Piece {
    Arena query, hit;
    uint32_t n = 0;
    uint64_t n_words = 0, total = 0;
    const uint64_t *words = nullptr; // sorted hit words: rank << (pos_bits + 1) | text position << 1 | strand
    uint32_t *offs = nullptr, *qrank = nullptr, *rstart = nullptr;
};
// Everything of a piece of n_sites <= 2^22 query sites but the locations.  Site i is d_sites[i * site_stride] (1: an array
// of signatures; 5: the `site` fields of issl_offtarget records).  d_offsets[0..n] = base + the piece's offsets, or NULL.
// Waits for the number of hit words and for the number of locations.
int locate_prepare(const issl_genome *g, const uint64_t *d_sites, size_t site_stride, size_t n_sites, uint64_t base,
                   uint64_t *d_offsets, hipStream_t stream, Piece &pc);
// A genome without a possible match, or an empty query.
bool nothing_to_find(const issl_genome *g, size_t n);

namespace {

constexpr uint32_t kPieceBits = 22;                 // query index inside a piece: key (41 bits) | index fits a word
constexpr size_t kPieceSites = size_t(1) << kPieceBits;
constexpr uint64_t kNoKey = 1ull << 40;             // key of a signature with bits above the 20 bases: matches nothing
constexpr uint64_t kHashMul = 0x9E3779B97F4A7C15ull;


// ---- query prep ---------------------------------------------------------------------------------------------------

// Site i is sites[i * stride]: the stride is in 8-byte words.
__global__ __launch_bounds__(256) void k_query_words(const uint64_t *__restrict__ sites, uint32_t stride, uint32_t n,
                                                     uint64_t *__restrict__ words)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t sig = sites[static_cast<uint64_t>(i) * stride];
    uint64_t key = 0;
#pragma unroll
    for (int p = 0; p < 20; ++p) key |= ((sig >> (2 * p)) & 3ull) << (2 * (19 - p));
    if (sig >> 40) key = kNoKey;
    words[i] = (key << kPieceBits) | i;
}

__global__ __launch_bounds__(256) void k_query_heads(const uint64_t *__restrict__ words, uint32_t n, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool head = i < n && (i == 0 || (words[i - 1] >> kPieceBits) != (words[i] >> kPieceBits));
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// first[b]: heads ahead of block b.  Every sorted query learns its rank; a head also lists its key and sets its bit.
__global__ __launch_bounds__(256) void k_query_ranks(const uint64_t *__restrict__ words, uint32_t n, const uint32_t *__restrict__ first,
                                                     uint64_t *__restrict__ ukeys, uint32_t *__restrict__ qrank,
                                                     uint32_t *__restrict__ bitmap, uint32_t hash_shift)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, wave = threadIdx.x >> 6;
    const bool valid = i < n;
    const uint64_t w = valid ? words[i] : 0ull;
    const uint64_t key = w >> kPieceBits;
    const bool head = valid && (i == 0 || (words[i - 1] >> kPieceBits) != key);
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    uint32_t before = first[blockIdx.x] + lanes_before(heads); // heads ahead of i
    for (uint32_t v = 0; v < wave; ++v) before += wave_cnt[v];
    if (!valid) return;
    const uint32_t rank = head ? before : before - 1;
    qrank[w & (kPieceSites - 1)] = rank;
    if (head) {
        ukeys[rank] = key;
        const uint32_t h = static_cast<uint32_t>((key * kHashMul) >> hash_shift);
        atomicOr(&bitmap[h >> 5], 1u << (h & 31));
    }
}

// ---- what the scan of the text asks -------------------------------------------------------------------------------

struct Probe {
    const uint64_t *ukeys;   // distinct query keys, ascending
    const uint32_t *n_ranks; // how many (device memory: the host never reads it)
    const uint32_t *bitmap;
    uint32_t hash_shift;
};

// Rank of `key` among the query's distinct keys, or -1.  `passed`: the bitmap let it through.
__device__ __forceinline__ int probe_key(const Probe &q, uint32_t nr, uint64_t key, uint32_t &passed)
{
    const uint32_t h = static_cast<uint32_t>((key * kHashMul) >> q.hash_shift);
    if (!((q.bitmap[h >> 5] >> (h & 31)) & 1u)) return -1;
    ++passed;
    uint32_t lo = 0, hi = nr;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (q.ukeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < nr && q.ukeys[lo] == key ? static_cast<int>(lo) : -1;
}

// ---- host: the preparation of one piece ---------------------------------------------------------------------------

// reserve() takes the sections of n <= kPieceSites queries in the caller's arena, ahead of its one hipMalloc; enqueue()
// puts the memsets and the launches on the caller's stream and waits nowhere.  Afterwards: `sorted` the n query words in
// key order, `probe` what the scan of the text asks, qrank[i] the rank of query i's key, ctr 64 bytes of zeros for the
// caller's counters.
struct QueryPrep {
    uint32_t n = 0, q_blocks = 0, map_bits = 0;
    size_t o_wb = 0, o_hist = 0, o_first = 0, o_ukeys = 0, o_qrank = 0, o_map = 0, o_ctr = 0;
    const uint64_t *sorted = nullptr;
    Probe probe{};
    uint32_t *qrank = nullptr;
    unsigned long long *ctr = nullptr;

    void reserve(Arena &a, uint32_t n_)
    {
        n = n_;
        q_blocks = (n + 255) / 256;
        map_bits = std::max(16u, bits_for(32ull * n)); // 32 .. 64 bits per query site
        o_wb = a.reserve(8ull * n);
        o_hist = a.reserve(4 * radix_hist_words(radix_sort_blocks(n)));
        o_first = a.reserve(4 * scan_words(q_blocks + 1ull));
        o_ukeys = a.reserve(8ull * n);
        o_qrank = a.reserve(4ull * n);
        o_map = a.reserve(size_t(1) << (map_bits - 3));
        o_ctr = a.reserve(64);
    }

    // wa: room for the n words, the caller's; site i is d_sites[i * stride].  The sort ends in wa or in the arena's buffer; with into_wa the words are
    // copied to wa when it ended in the other one.
    int enqueue(const Arena &a, const uint64_t *d_sites, uint64_t *wa, bool into_wa, hipStream_t stream, uint32_t stride = 1)
    {
        uint64_t *wb = a.at<uint64_t>(o_wb), *ukeys = a.at<uint64_t>(o_ukeys);
        uint32_t *first = a.at<uint32_t>(o_first), *bitmap = a.at<uint32_t>(o_map);
        qrank = a.at<uint32_t>(o_qrank);
        ctr = a.at<unsigned long long>(o_ctr);
        HIP_TRY(hipMemsetAsync(bitmap, 0, size_t(1) << (map_bits - 3), stream));
        HIP_TRY(hipMemsetAsync(ctr, 0, 64, stream));
        HIP_TRY(hipMemsetAsync(first + q_blocks, 0, 4, stream));
        hipLaunchKernelGGL(k_query_words, dim3(q_blocks), dim3(256), 0, stream, d_sites, stride, n, wa);
        sorted = radix_sort_async(wa, wb, n, kPieceBits, kPieceBits + 41, a.at<uint32_t>(o_hist), stream);
        if (into_wa && sorted != wa) {
            HIP_TRY(hipMemcpyAsync(wa, sorted, 8ull * n, hipMemcpyDeviceToDevice, stream));
            sorted = wa;
        }
        hipLaunchKernelGGL(k_query_heads, dim3(q_blocks), dim3(256), 0, stream, sorted, n, first);
        launch_scan(first, q_blocks + 1ull, stream);
        probe = Probe{ukeys, first + q_blocks, bitmap, 64 - map_bits};
        hipLaunchKernelGGL(k_query_ranks, dim3(q_blocks), dim3(256), 0, stream, sorted, n, first, ukeys, qrank, bitmap, probe.hash_shift);
        return ISSL_OK;
    }
};

} // namespace
} // namespace issl
