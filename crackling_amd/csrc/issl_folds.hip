// RNAfold's exchange, the kernels (issl_folds_*, include/issl_hip.h): Crackling.py:406-497 around the RNAfold program.
//   input    k_folds_input: a workgroup takes 256 rows of the fold list, whose 256 * 101 bytes start at a multiple of 16:
//            the guides go to LDS, the lines are assembled there four bytes at a time (the scaffold of :395 is the same 80
//            characters in every line) and leave as 16-byte stores, all lanes on consecutive addresses
//   read     k_folds_mark: one thread per kFoldGroupBytes of the page's text, four 16-byte loads, one bit per byte that
//            ends a line (LF, or CR with no LF behind it: a CR that is a group's last byte looks at the next group's
//            first), the group's count; launch_scan ranks the groups.  Only the parity of a line's number matters -- even
//            lines are the first of a pair -- so the ranks may wrap at 2^32 lines without harm, and a page has no limit of
//            lines.  k_folds_keys + the radix sort (issl_radix.hpp) order the 38-bit keys guide[1:20] of the page's rows.
//            k_folds_pairs: the same thread per group walks its line ends; behind the end of an odd line starts a pair,
//            whose key (issl_folds_text.hpp) is looked up in the sorted keys and, where a row of the page has it, its
//            first line's offset + 1 goes into the run's first slot with atomicMax: the last pair of the text wins, in
//            whatever order the threads run.  The text's last line has no partner and starts no pair.
//            k_folds_rows: one thread per row finds its key's slot, and reads the pair it names by the shared rules into
//            one issl_fold and three spans; a refused pair goes into the error word with atomicMin (row << 8 | kind).
// No kernel indexes an array in registers at run time, none uses scratch memory.  Nothing here waits.
#include <hip/hip_runtime.h>

#include "issl_folds.hpp"
#include "issl_folds_text.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"

namespace issl {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kKeyMask = (1ull << 38) - 1;
constexpr uint32_t kInputBytes = kThreads * kFoldLineBytes; // 25856 = 16 * 1616: every workgroup starts on a multiple of 16
static_assert(kInputBytes % 16 == 0, "a workgroup's lines are whole 16-byte spans");
static_assert(kFoldGroupBytes == 64, "a group is one bit per byte of a 64-bit mask");
static_assert(sizeof(issl_fold) == 16 && sizeof(issl_text_span) == 16, "written as 16-byte rows");

__device__ const char k_scaffold[81] = "GUUUUAGAGCUAGAAAUAGCAAGUUAAAAUAAGGCUAGUCCGUUAUCAACUUGAAAAAGUGGCACCGAGUCGGUGCUUUU";

// ---- RNAfold's input ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_folds_input(const ulonglong2 *__restrict__ guides, uint32_t n_guides,
                                                          const uint32_t *__restrict__ list, uint64_t first, uint64_t n,
                                                          char *__restrict__ text)
{
    __shared__ uint64_t s_guide[kThreads];
    __shared__ __attribute__((aligned(16))) uint32_t stage[kInputBytes / 4];
    const uint32_t t = threadIdx.x;
    const uint64_t row0 = static_cast<uint64_t>(blockIdx.x) * kThreads; // of the run
    const uint32_t rows = n - row0 < kThreads ? static_cast<uint32_t>(n - row0) : kThreads;
    uint64_t g = 0;
    if (t < rows) {
        const uint32_t j = list[first + row0 + t];
        if (j < n_guides) g = guides[2ull * j].x;
    }
    s_guide[t] = g;
    __syncthreads();
    const uint32_t bytes = rows * kFoldLineBytes;
    for (uint32_t w = t; 4u * w < bytes; w += kThreads) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t at = 4u * w + k, row = at / kFoldLineBytes, pos = at - row * kFoldLineBytes;
            uint32_t c = '\n';
            if (at >= bytes) c = 0;
            else if (pos == 0) c = 'G';
            else if (pos < 20) c = (0x54474341u >> (8 * ((s_guide[row] >> (2 * pos)) & 3u))) & 0xFFu; // A C G T
            else if (pos < 100) c = static_cast<uint8_t>(k_scaffold[pos - 20]);
            v |= c << (8 * k);
        }
        stage[w] = v;
    }
    __syncthreads();
    uint4 *out = reinterpret_cast<uint4 *>(text + row0 * kFoldLineBytes); // (the buffer ends on a multiple of 16)
    const uint4 *src = reinterpret_cast<const uint4 *>(stage);
    for (uint32_t v = t; 16u * v < bytes; v += kThreads) {
        uint4 x = src[v];
        if (16u * v + 16u > bytes) { // the words behind the last line were never written: zero, not what LDS held
            const uint32_t keep = (bytes - 16u * v + 3u) / 4u;
            if (keep < 2) x.y = 0;
            if (keep < 3) x.z = 0;
            if (keep < 4) x.w = 0;
        }
        out[v] = x;
    }
}

__global__ __launch_bounds__(kThreads) void k_folds_clear(ulonglong2 *__restrict__ folds, ulonglong2 *__restrict__ spans,
                                                          uint64_t first, uint64_t n)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    folds[first + i] = make_ulonglong2(0, 0);
    for (uint32_t k = 0; k < 3; ++k) spans[3 * (first + i) + k] = make_ulonglong2(0, folds_text::kNoText);
}

// ---- RNAfold's answers -------------------------------------------------------------------------------------------------

// Bit b: byte 64 g + b of the text ends a line (byte_masks, group_line_ends: issl_folds_text.hpp).
__device__ __forceinline__ uint64_t group_ends(const uint8_t *__restrict__ text, uint64_t len, uint64_t g)
{
    const uint4 *p = reinterpret_cast<const uint4 *>(text + g * kFoldGroupBytes); // (inside the buffer's padding at the end)
    uint64_t lf = 0, cr = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint4 x = p[q];
        folds_text::byte_masks(x.x, 16 * q, lf, cr);
        folds_text::byte_masks(x.y, 16 * q + 4, lf, cr);
        folds_text::byte_masks(x.z, 16 * q + 8, lf, cr);
        folds_text::byte_masks(x.w, 16 * q + 12, lf, cr);
    }
    const uint64_t here = len - g * kFoldGroupBytes; // bytes of the text in this group and behind it (> 0)
    const bool next_is_lf = here > kFoldGroupBytes && text[(g + 1) * kFoldGroupBytes] == '\n';
    return folds_text::group_line_ends(lf, cr, here, next_is_lf);
}

__global__ __launch_bounds__(kThreads) void k_folds_mark(const uint8_t *__restrict__ text, uint64_t len, uint64_t n_groups,
                                                         uint32_t *__restrict__ counts)
{
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (g >= n_groups) return;
    counts[g] = static_cast<uint32_t>(__builtin_popcountll(group_ends(text, len, g)));
}

__device__ __forceinline__ uint64_t row_key(const ulonglong2 *__restrict__ guides, uint32_t n_guides, uint32_t j)
{
    return j < n_guides ? (guides[2ull * j].x >> 2) & kKeyMask : 0;
}

__global__ __launch_bounds__(kThreads) void k_folds_keys(const ulonglong2 *__restrict__ guides, uint32_t n_guides,
                                                         const uint32_t *__restrict__ list, uint64_t first, uint64_t n,
                                                         uint64_t *__restrict__ keys)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) keys[i] = row_key(guides, n_guides, list[first + i]);
}

// First index of sorted[0 .. n) whose key is not below `key`.
__device__ __forceinline__ uint64_t first_not_below(const uint64_t *__restrict__ sorted, uint64_t n, uint64_t key)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void offer_pair(const uint8_t *__restrict__ text, uint64_t len, uint64_t s, uint64_t last_line,
                                           const uint64_t *__restrict__ sorted, uint64_t n, unsigned long long *__restrict__ best)
{
    uint64_t key;
    if (s >= last_line || !folds_text::pair_key(text, s, len, key)) return;
    const uint64_t at = first_not_below(sorted, n, key);
    if (at < n && sorted[at] == key) atomicMax(&best[at], static_cast<unsigned long long>(s + 1));
}

// ranks[g] = line ends ahead of group g, modulo 2^32.
__global__ __launch_bounds__(kThreads) void k_folds_pairs(const uint8_t *__restrict__ text, uint64_t len, uint64_t n_groups,
                                                          const uint32_t *__restrict__ ranks, uint64_t last_line,
                                                          const uint64_t *__restrict__ sorted, uint64_t n,
                                                          unsigned long long *__restrict__ best)
{
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (g >= n_groups) return;
    if (g == 0) offer_pair(text, len, 0, last_line, sorted, n, best); // line 0
    uint64_t ends = group_ends(text, len, g);
    uint32_t line = ranks[g]; // the number of the line the next end closes
    while (ends) {
        const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(ends));
        ends &= ends - 1;
        if (line & 1u) offer_pair(text, len, g * kFoldGroupBytes + b + 1, last_line, sorted, n, best);
        ++line;
    }
}

__global__ __launch_bounds__(kThreads) void k_folds_rows(const ulonglong2 *__restrict__ guides, uint32_t n_guides,
                                                         const uint32_t *__restrict__ list, uint64_t first, uint64_t n,
                                                         const uint8_t *__restrict__ text, uint64_t len, uint64_t base,
                                                         const uint64_t *__restrict__ sorted,
                                                         const unsigned long long *__restrict__ best,
                                                         ulonglong2 *__restrict__ folds, ulonglong2 *__restrict__ spans,
                                                         unsigned long long *__restrict__ error)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = first + i;
    const uint64_t key = row_key(guides, n_guides, list[row]);
    const uint64_t at = first_not_below(sorted, n, key);
    const uint64_t found = at < n && sorted[at] == key ? best[at] : 0;
    if (found == 0 || found > len) return; // no pair under this key: the row keeps present = 0 and no text
    folds_text::Pair p;
    const uint32_t kind = folds_text::read_pair(text, len, found - 1, p);
    if (kind != folds_text::kFine) {
        atomicMin(error, static_cast<unsigned long long>(row << 8 | kind));
        return;
    }
    folds[row] = make_ulonglong2(static_cast<uint64_t>(__double_as_longlong(p.energy)),
                                 static_cast<uint64_t>(p.scaffold) | static_cast<uint64_t>(p.present) << 32);
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) // (reserved: the bytes the table would quote the field for)
        spans[3 * row + k] = make_ulonglong2(base + p.offset[k], static_cast<uint64_t>(p.length[k]) |
                                                                     static_cast<uint64_t>(folds_text::quote_bits(text, p.offset[k], p.length[k])) << 32);
}

uint64_t groups_of(uint64_t len) { return (len + kFoldGroupBytes - 1) / kFoldGroupBytes; }
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The sections of a read's work buffer.
struct Work {
    size_t ranks, keys, tmp, best, hist, size;
    Work(uint64_t n, uint64_t len)
    {
        size_t at = 0;
        ranks = at; at += align256(4 * scan_words(groups_of(len) + 1));
        keys = at; at += align256(8 * n);
        tmp = at; at += align256(8 * n);
        best = at; at += align256(8 * n);
        hist = at; at += align256(4 * radix_hist_words(radix_sort_blocks(n)));
        size = at;
    }
};

} // namespace

void launch_folds_input(const FoldSource &src, uint64_t first, uint64_t n, char *text, hipStream_t stream)
{
    if (!n) return;
    hipLaunchKernelGGL(k_folds_input, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, src.guides, src.n_guides, src.fold_list,
                       first, n, text);
}

void launch_folds_clear(issl_fold *folds, issl_text_span *spans, uint64_t first, uint64_t n, hipStream_t stream)
{
    if (!n) return;
    hipLaunchKernelGGL(k_folds_clear, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, reinterpret_cast<ulonglong2 *>(folds),
                       reinterpret_cast<ulonglong2 *>(spans), first, n);
}

size_t folds_read_work(uint64_t n, uint64_t len) { return Work(n, len).size; }

hipError_t launch_folds_read(const FoldSource &src, const FoldRead &r, hipStream_t stream)
{
    if (!r.n || !r.len) return hipSuccess; // no row to fill, or no pair to fill it with
    const Work w(r.n, r.len);
    char *work = static_cast<char *>(r.work);
    uint32_t *ranks = reinterpret_cast<uint32_t *>(work + w.ranks);
    uint64_t *keys = reinterpret_cast<uint64_t *>(work + w.keys), *tmp = reinterpret_cast<uint64_t *>(work + w.tmp);
    unsigned long long *best = reinterpret_cast<unsigned long long *>(work + w.best);
    const uint64_t n_groups = groups_of(r.len);
    hipError_t e = hipMemsetAsync(ranks + n_groups, 0, 4, stream); // (unset, the ranks and the slots would give wrong pairs)
    if (e == hipSuccess) e = hipMemsetAsync(best, 0, 8 * r.n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_folds_mark, dim3(blocks_for(n_groups, kThreads)), dim3(kThreads), 0, stream, r.text, r.len, n_groups, ranks);
    launch_scan(ranks, n_groups + 1, stream);
    hipLaunchKernelGGL(k_folds_keys, dim3(blocks_for(r.n, kThreads)), dim3(kThreads), 0, stream, src.guides, src.n_guides, src.fold_list,
                       r.first, r.n, keys);
    const uint64_t *sorted = radix_sort_async(keys, tmp, r.n, 0, 38, reinterpret_cast<uint32_t *>(work + w.hist), stream);
    hipLaunchKernelGGL(k_folds_pairs, dim3(blocks_for(n_groups, kThreads)), dim3(kThreads), 0, stream, r.text, r.len, n_groups, ranks,
                       r.last_line, sorted, r.n, best);
    hipLaunchKernelGGL(k_folds_rows, dim3(blocks_for(r.n, kThreads)), dim3(kThreads), 0, stream, src.guides, src.n_guides, src.fold_list,
                       r.first, r.n, r.text, r.len, r.base, sorted, best, reinterpret_cast<ulonglong2 *>(r.folds),
                       reinterpret_cast<ulonglong2 *>(r.spans), reinterpret_cast<unsigned long long *>(r.error));
    return hipGetLastError();
}

} // namespace issl
