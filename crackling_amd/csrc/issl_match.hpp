// What the units that read genome text share (issl_extract.hip: site extraction and genome -> index; issl_locate.hip:
// resident genome and locate; issl_guides.hip: candidate guides): the pattern test of extractOfftargets.py:23-24 on the
// device, the LSD radix sort of 64-bit words and the FASTA -> record text pass of the host.  Kernels and device functions
// live in an anonymous namespace, one copy per translation unit, like issl_radix.hpp.  The host plumbing around a launch
// (HIP_TRY, DevBuf, Arena, StageTimer, select_device) is issl_hiputil.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "issl_hiputil.hpp"
#include "issl_radix.hpp"

namespace issl {

// FASTA bytes -> upper-cased sequence text appended to seq, '\n' after every record (issl_extract.hip).  per_file: the
// reference's rules for several inputs.  records (optional): the record table of what was appended; seq is the same
// bytes with or without it.
void append_records(const char *fasta, size_t len, bool per_file, std::string &seq, std::vector<FastaRecord> *records = nullptr);
// The FASTA files at paths[0..n) -> seq: the explode rules for one input, the per-file rules for several.
int read_fasta_files(const char *const *paths, int n, std::string &seq, std::vector<FastaRecord> *records = nullptr);

namespace {

constexpr uint32_t kPosPerBlock = 4096; // text positions per 256-thread workgroup

// 0..3 for A C G T, 4 for anything else
__device__ __forceinline__ uint32_t base_code(uint8_t c)
{
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// Matches starting at position i: bit 0 = forward pattern, bit 1 = reverse pattern; keys of the two sites.
__device__ __forceinline__ uint32_t match_at(const uint8_t *__restrict__ s, uint64_t i, uint64_t len, uint64_t &key_fwd,
                                             uint64_t &key_rev)
{
    if (i + 23 > len) return 0;
    uint32_t code[23];
    bool body = true; // characters 1..20 are [ACGT] in both patterns
#pragma unroll
    for (int k = 0; k < 23; ++k) code[k] = base_code(s[i + k]);
#pragma unroll
    for (int k = 1; k <= 20; ++k) body = body && code[k] < 4u;
    if (!body) return 0;
    const bool fwd = code[0] < 3u && (code[21] == 0u || code[21] == 2u) && code[22] == 2u;
    const bool rev = code[0] == 1u && (code[1] == 1u || code[1] == 3u) && code[21] < 4u &&
                     (code[22] == 3u || code[22] == 2u || code[22] == 1u);
    if (!fwd && !rev) return 0;
    uint64_t kf = 0, kr = 0;
#pragma unroll
    for (int p = 0; p < 20; ++p) {
        kf |= static_cast<uint64_t>(code[p]) << (2 * (19 - p));   // text order: base 0 most significant
        kr |= static_cast<uint64_t>(3u - code[p]) << (2 * p);      // reverse complement of the same 20 characters
    }
    key_fwd = kf;
    key_rev = kr;
    return (fwd ? 1u : 0u) | (rev ? 2u : 0u);
}

__device__ __forceinline__ uint32_t lanes_before(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// Last index i of tab[0..n) with tab[i] <= x (0 when there is none).
template <class T> __device__ __forceinline__ uint32_t last_not_above(const T *tab, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n; // first index with tab[i] > x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (static_cast<uint64_t>(tab[mid]) <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

inline uint32_t bits_for(uint64_t values) // bits that hold 0 .. values - 1
{
    uint32_t b = 1;
    while (b < 64 && (1ull << b) < values) ++b;
    return b;
}

// LSD radix sort of d_keys[0..n) on the bits [lo, hi), 8 per pass, all launches on `stream`, no synchronisation.  d_tmp
// has the size of d_keys, d_hist radix_hist_words(radix_sort_blocks(n)) words.  Returns the buffer the result is in.
inline uint32_t radix_sort_blocks(uint64_t n) { return static_cast<uint32_t>((n + 256ull * kSortItems - 1) / (256ull * kSortItems)); }

inline uint64_t *radix_sort_async(uint64_t *d_keys, uint64_t *d_tmp, uint64_t n, uint32_t lo, uint32_t hi, uint32_t *d_hist,
                                  hipStream_t stream)
{
    if (n < 2) return d_keys;
    const uint32_t n_blocks = radix_sort_blocks(n);
    uint64_t *src = d_keys, *dst = d_tmp;
    for (uint32_t shift = lo; shift < hi; shift += 8) {
        hipLaunchKernelGGL(k_radix_hist, dim3(n_blocks), dim3(256), 0, stream, src, n, shift, d_hist, n_blocks, 0xFFu);
        launch_radix_scan(d_hist, n_blocks, stream);
        hipLaunchKernelGGL(k_radix_scatter<KeyItself>, dim3(n_blocks), dim3(256), 0, stream, src, dst, n, shift, d_hist,
                           n_blocks, KeyItself{}, 0xFFu);
        std::swap(src, dst);
    }
    return src;
}

// Sort d_keys[0..n) ascending on the low `bits` bits; d_tmp has the same size.  Result in d_keys.  Blocking.
inline int radix_sort(uint64_t *d_keys, uint64_t *d_tmp, uint64_t n, uint32_t bits)
{
    if (n < 2) return ISSL_OK;
    DevBuf hist;
    HIP_TRY(hipMalloc(&hist.p, 4ull * radix_hist_words(radix_sort_blocks(n))));
    uint64_t *src = radix_sort_async(d_keys, d_tmp, n, 0, bits, static_cast<uint32_t *>(hist.p), nullptr);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error(std::string("HIP error in radix sort: ") + hipGetErrorString(e));
        return ISSL_E_DEVICE;
    }
    if (src != d_keys) HIP_TRY(hipMemcpy(d_keys, src, 8 * n, hipMemcpyDeviceToDevice));
    return ISSL_OK;
}

} // namespace
} // namespace issl
