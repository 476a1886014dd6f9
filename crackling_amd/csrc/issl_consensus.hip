// Efficiency consensus (issl_consensus_*, include/issl_hip.h): Crackling.py:306-598 and the filter that decides which
// guides every step of it looks at (filterCandidateGuides, :36-149), on the rows of a resident guide set.  G20, the
// mm10db filters (leading T, AT percent, TTTT, the decision rule for RNAfold's answers), sgRNAScorer2 and the count.
//
// Every step of the reference reads and writes the properties of one guide only, and the filter asks about that guide
// alone, so a thread walks one guide through the steps in the reference's order with its codes in registers.  The one
// thing that crosses guides is RNAfold's output, keyed by guide[1:20]: that is settled on the host
// (read_rnafold_output of the package) before the folds come back in the order of the fold list.
//   begin    k_consensus_begin: one thread per guide: G20, leading T, AT percent, TTTT, each only where the filter
//            yields the guide at that point; one 32-byte row per guide; the guides the filter yields for the fold are
//            counted per workgroup, launch_scan ranks the workgroups, k_consensus_list writes the rows ascending
//   finish   k_consensus_fold: one thread per fold: the rule of :476-498 into its row; k_consensus_finish: one thread
//            per guide: the mm10db verdict, the sgRNAScorer2 score where the filter yields the guide, the count; the
//            guides the specificity filter yields are counted and listed the same way
// The sgRNAScorer2 model is a linear-kernel SVC over 80 one-hot inputs whose support vectors are 0/1 rows: the kernel
// value of support vector i is popcount(sv_i & onehot(guide)), the decision value libsvm's sum in support-vector order.
// A support vector is 24 bytes here (80 mask bits, the coefficient); every lane of a wave reads the same one, so the
// loads are scalar and a guide costs three popcounts, a conversion, a multiply and an add per support vector.  Products
// and sums are rounded one by one (__dmul_rn, __dadd_rn: no contraction), as libsvm built without FMA rounds them.
//   pages    issl_consensus_selection_pages: the reference's Bowtie pages of a run in batches, as boundaries in the
//            selection (k_pages_edges, k_pages_count, launch_scan, k_pages_fill further down)
// The host waits once per list, for its length, and once per set of pages, for their number.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_folds.hpp"
#include "issl_guides.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"
#include "issl_runlog.hpp"

namespace issl {
namespace {

constexpr uint32_t kThreads = 256;              // guides per workgroup of every kernel here
constexpr uint32_t kNo = 0, kYes = 1, kUntested = 2, kError = 3; // the codes of issl_consensus_row
enum Module : uint32_t { kChopchop, kMm10db, kSgrna, kSpecificity };
enum List : uint32_t { kFoldList, kSelection };

static_assert(sizeof(issl_consensus_row) == 32, "issl_consensus_row is 32 bytes");
static_assert(sizeof(issl_fold) == 16, "issl_fold is 16 bytes");

// What the kernels need of issl_consensus_config, by value.
struct Config {
    uint32_t optimisation, n, mm10db, chopchop, sgrna, n_sv;
    double intercept, sgrna_threshold, low_energy, high_energy;
};

// One support vector: bit 4p + j of the 80 = sv[i][4p + j].
struct SupportVector {
    uint64_t lo;   // inputs 0..63
    uint32_t hi;   // inputs 64..79
    uint32_t pad;
    double coef;
};
static_assert(sizeof(SupportVector) == 24, "three scalar loads of 8 bytes");

// The properties of a guide the filter reads.
struct State {
    uint32_t g20 = kUntested, lead_t = kUntested, at_pct = kUntested, tttt = kUntested, ss = kUntested, mm10db = kUntested,
             sgrna = kUntested, count = 0;
    bool unique = false;
};

__device__ __forceinline__ uint64_t pack_codes(const State &s)
{
    return static_cast<uint64_t>(s.g20) | static_cast<uint64_t>(s.lead_t) << 8 | static_cast<uint64_t>(s.at_pct) << 16 |
           static_cast<uint64_t>(s.tttt) << 24 | static_cast<uint64_t>(s.ss) << 32 | static_cast<uint64_t>(s.mm10db) << 40 |
           static_cast<uint64_t>(s.sgrna) << 48 | static_cast<uint64_t>(s.count) << 56;
}

__device__ __forceinline__ State unpack_codes(uint64_t w, bool unique)
{
    State s;
    s.g20 = w & 0xFFu;
    s.lead_t = (w >> 8) & 0xFFu;
    s.at_pct = (w >> 16) & 0xFFu;
    s.tttt = (w >> 24) & 0xFFu;
    s.ss = (w >> 32) & 0xFFu;
    s.mm10db = (w >> 40) & 0xFFu;
    s.sgrna = (w >> 48) & 0xFFu;
    s.count = static_cast<uint32_t>(w >> 56);
    s.unique = unique;
    return s;
}

// filterCandidateGuides (Crackling.py:36-149) for one guide; passedBowtie is untested here and rejects nothing.
__device__ __forceinline__ bool assess(const Config &c, Module module, const State &s)
{
    if (c.optimisation == 0) return true;  // ultralow
    if (!s.unique) return false;
    if (c.optimisation == 1) return true;  // low
    if (module == kSpecificity) return s.count >= c.n;
    if (c.optimisation == 3) {             // high: is the consensus still open for this guide?
        const int64_t accepted = (s.mm10db == kYes) + (s.g20 == kYes) + (s.sgrna == kYes);
        const int64_t assessed = (s.mm10db <= kYes) + (s.g20 <= kYes) + (s.sgrna <= kYes);
        const int64_t tools = (c.mm10db != 0) + (c.chopchop != 0) + (c.sgrna != 0);
        const int64_t n = c.n;
        if (accepted >= n) return false;
        if (tools - assessed < n - accepted) return false;
    }
    if (module == kMm10db &&
        (s.lead_t == kNo || s.at_pct == kNo || s.tttt == kNo || s.ss == kNo || s.mm10db == kNo))
        return false;
    return true;
}

__device__ __forceinline__ bool listed(const Config &c, List which, const State &s)
{
    return which == kFoldList ? c.mm10db != 0 && assess(c, kMm10db, s) : assess(c, kSpecificity, s);
}

// counts[workgroup] = its lanes with `mine`.
__device__ __forceinline__ void count_block(bool mine, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_cnt[kThreads / 64];
    const uint64_t b = __ballot(mine);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__builtin_popcountll(b));
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// guides: issl_guide as two 16-byte halves, {guide23, start} and {record | strand << 32, seen}.
__device__ __forceinline__ bool seen_once(const ulonglong2 *__restrict__ guides, uint64_t j)
{
    return static_cast<uint32_t>(guides[2 * j + 1].y) == 1u;
}

// Crackling.py:310-384.  rows: issl_consensus_row as two halves, {sgrna_score, at} and {ss_energy, codes}.
__global__ __launch_bounds__(kThreads) void k_consensus_begin(const ulonglong2 *__restrict__ guides, uint32_t n, Config c,
                                                              ulonglong2 *__restrict__ rows, uint32_t *__restrict__ counts)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    bool fold = false;
    if (j < n) {
        const uint64_t guide = guides[2ull * j].x;
        State s;
        s.unique = seen_once(guides, j);
        double at = __builtin_nan("");
        if (c.chopchop && assess(c, kChopchop, s)) s.g20 = ((guide >> 38) & 3u) == 2u ? kYes : kNo;   // guide[19] == 'G'
        if (c.mm10db) {
            if (assess(c, kMm10db, s)) s.lead_t = (guide & 3u) == 3u ? kNo : kYes;                   // guide[0] == 'T'
            if (assess(c, kMm10db, s)) {
                // A = 00 and T = 11: the two bits of the base are equal
                const uint64_t even = 0x5555555555ull; // 20 bases
                const uint32_t cnt = static_cast<uint32_t>(__builtin_popcountll(~(guide ^ (guide >> 1)) & even));
                at = __ddiv_rn(__dmul_rn(100.0, static_cast<double>(cnt)), 20.0);
                s.at_pct = (at < 20.0 || at > 65.0) ? kNo : kYes;
            }
            if (assess(c, kMm10db, s)) {
                const uint64_t t = guide & (guide >> 1) & 0x155555555555ull; // bit 2p: guide[p] == 'T', 23 bases
                s.tttt = (t & (t >> 2) & (t >> 4) & (t >> 6)) ? kNo : kYes;
            }
        }
        fold = listed(c, kFoldList, s);
        const uint64_t nan_bits = static_cast<uint64_t>(__double_as_longlong(__builtin_nan("")));
        rows[2ull * j] = make_ulonglong2(nan_bits, static_cast<uint64_t>(__double_as_longlong(at)));
        rows[2ull * j + 1] = make_ulonglong2(nan_bits, pack_codes(s));
    }
    count_block(fold, counts);
}

// The rows `which` lists, ascending: first[b] = listed rows ahead of workgroup b.  Nothing is written at or above n_list.
__global__ __launch_bounds__(kThreads) void k_consensus_list(const ulonglong2 *__restrict__ guides, uint32_t n, Config c, List which,
                                                             const ulonglong2 *__restrict__ rows, const uint32_t *__restrict__ first,
                                                             uint32_t *__restrict__ list, uint32_t n_list)
{
    __shared__ uint32_t wave_cnt[kThreads / 64];
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x, wave = threadIdx.x >> 6;
    const bool mine = j < n && listed(c, which, unpack_codes(rows[2ull * j + 1].y, seen_once(guides, j)));
    const uint64_t b = __ballot(mine);
    if ((threadIdx.x & 63) == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(b));
    __syncthreads();
    uint32_t at = first[blockIdx.x] + lanes_before(b);
    for (uint32_t v = 0; v < wave; ++v) at += wave_cnt[v];
    if (mine && at < n_list) list[at] = j;
}

// Crackling.py:472-498 for fold i of the list.  energy: the number RNAfold printed; scaffold: its structure matched the
// pattern of :396; present == 0: no line for this guide, the row keeps '?'.
__global__ __launch_bounds__(kThreads) void k_consensus_fold(const ulonglong2 *__restrict__ guides, uint32_t n, Config c,
                                                             const uint32_t *__restrict__ list, const issl_fold *__restrict__ folds,
                                                             uint32_t n_list, issl_consensus_row *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t j = list[i];
    const issl_fold f = folds[i];
    if (j >= n || !f.present) return;
    uint32_t ss;
    if ((guides[2ull * j].x & 3u) == 3u) ss = kError; // RNAfold's line starts with G, C or A for no guide that starts with T (:476)
    else if (f.scaffold) ss = f.energy < c.low_energy ? kNo : kYes;
    else ss = f.energy <= c.high_energy ? kNo : kYes;
    rows[j].ss_energy = f.energy;
    rows[j].ss = static_cast<uint8_t>(ss);
}

// The reference's one-hot input (:545-563) as 80 bits: A 0001, C 0010, T 0100, G 1000 as strings, string index 0 = bit 0.
__device__ __forceinline__ void onehot(uint64_t guide, uint64_t &lo, uint32_t &hi)
{
    lo = 0;
    hi = 0;
#pragma unroll
    for (int p = 0; p < 16; ++p) lo |= static_cast<uint64_t>((0x2148u >> (4 * ((guide >> (2 * p)) & 3u))) & 0xFu) << (4 * p);
#pragma unroll
    for (int p = 16; p < 20; ++p) hi |= ((0x2148u >> (4 * ((guide >> (2 * p)) & 3u))) & 0xFu) << (4 * (p - 16));
}

// Crackling.py:518-530, :556-575, :586-591.
__global__ __launch_bounds__(kThreads) void k_consensus_finish(const ulonglong2 *__restrict__ guides, uint32_t n, Config c,
                                                               const SupportVector *__restrict__ sv, ulonglong2 *__restrict__ rows,
                                                               uint32_t *__restrict__ counts)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    bool selected = false;
    if (j < n) {
        const uint64_t guide = guides[2ull * j].x;
        State s = unpack_codes(rows[2ull * j + 1].y, seen_once(guides, j));
        if (c.mm10db) s.mm10db = (s.at_pct == kYes && s.tttt == kYes && s.ss == kYes && s.lead_t == kYes) ? kYes : kNo;
        if (c.sgrna && assess(c, kSgrna, s)) {
            uint64_t lo;
            uint32_t hi;
            onehot(guide, lo, hi);
            double sum = 0.0;
#pragma unroll 4
            for (uint32_t i = 0; i < c.n_sv; ++i) { // i is the same in every lane: the support vector comes by scalar loads
                const SupportVector v = sv[i];
                const int k = __builtin_popcountll(v.lo & lo) + __builtin_popcount(v.hi & hi);
                sum = __dadd_rn(sum, __dmul_rn(v.coef, static_cast<double>(k)));
            }
            const double score = -__dadd_rn(sum, c.intercept);
            rows[2ull * j].x = static_cast<uint64_t>(__double_as_longlong(score));
            s.sgrna = score < c.sgrna_threshold ? kNo : kYes;
        }
        s.count = (s.mm10db == kYes) + (s.sgrna == kYes) + (s.g20 == kYes);
        rows[2ull * j + 1].y = pack_codes(s);
        selected = listed(c, kSelection, s);
    }
    count_block(selected, counts);
}

// ---- the pages of a batched run (issl_consensus_selection_pages) ---------------------------------------------------
// A batch is rows [b B, min((b + 1) B, n)) of the set, and the reference's pages start again with every batch: its
// boundaries, in positions of the ascending selection.  k_pages_edges: one lower bound per batch edge; k_pages_count:
// the pages of every batch; launch_scan: the pages ahead of every batch; k_pages_fill: one thread per PAGE finds its
// batch in those offsets, so one batch cut into 10^8 pages of one row is no more work per thread than any other.

// edges[e] = selected rows below row min(e * batch, n) of the set, e = 0 .. n_batches.
__global__ __launch_bounds__(kThreads) void k_pages_edges(const uint32_t *__restrict__ selection, uint32_t n_selected, uint64_t n,
                                                          uint64_t batch, uint32_t n_batches, uint32_t *__restrict__ edges)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e > n_batches) return;
    const uint64_t row = e == n_batches || e * batch > n ? n : e * batch; // (e * batch < 2^64: e > 0 only with batch < n < 2^32)
    uint32_t a = 0, b = n_selected; // first position with selection[a] >= row
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (selection[mid] < row) a = mid + 1;
        else b = mid;
    }
    edges[e] = a;
}

// counts[b] = pages of batch b: its selected rows in pages of page_length, or one page when it has any (page_length 0).
__global__ __launch_bounds__(kThreads) void k_pages_count(const uint32_t *__restrict__ edges, uint32_t n_batches, uint64_t page_length,
                                                          uint32_t *__restrict__ counts)
{
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= n_batches) return;
    const uint64_t rows = edges[b + 1] - edges[b];
    counts[b] = static_cast<uint32_t>(page_length ? (rows + page_length - 1) / page_length : (rows ? 1u : 0u));
}

// first[b] = pages ahead of batch b, first[n_batches] = all pages.  starts[p] for p < all pages, starts[all pages] = n_selected;
// the grid covers `cap`, the host's upper bound of the pages, and one more.
__global__ __launch_bounds__(kThreads) void k_pages_fill(const uint32_t *__restrict__ edges, const uint32_t *__restrict__ first,
                                                         uint32_t n_batches, uint64_t page_length, uint32_t n_selected,
                                                         uint64_t cap, uint64_t *__restrict__ starts)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t n_pages = first[n_batches];
    if (p > n_pages || p > cap) return;
    if (p == n_pages) {
        starts[p] = n_selected;
        return;
    }
    const uint32_t b = last_not_above(first, n_batches, p); // behind the batches without a page: first[b] <= p < first[b + 1]
    starts[p] = edges[b] + (p - first[b]) * page_length;
}

} // namespace
} // namespace issl

struct issl_consensus {
    int device = -1;
    uint32_t n = 0;                       // guides of the set
    const ulonglong2 *guides = nullptr;   // the set's rows: it outlives this object
    issl::Config cfg{};
    issl::OwnedStream stream;             // ahead of the buffers: they are released first
    issl::DevBuf rows, counts, sv, fold_list, selection;
    issl::DevBuf pages;                   // the boundaries of the last issl_consensus_selection_pages
    uint64_t n_fold = 0, n_selected = 0;
    bool finished = false;
};

namespace issl {
namespace {

// counts[0 .. blocks) of the kernel before -> the list: its length to the host, its rows ascending into `list`.
int make_list(issl_consensus *c, List which, DevBuf &list, uint64_t &n_list)
{
    hipStream_t stream = c->stream.s;
    const uint32_t blocks = blocks_for(c->n, kThreads);
    uint32_t *counts = static_cast<uint32_t *>(c->counts.p);
    launch_scan(counts, blocks + 1ull, stream);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + blocks, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total > c->n) {
        set_error("consensus list on the device: " + std::to_string(total) + " of " + std::to_string(c->n) + " guides");
        return ISSL_E_DEVICE;
    }
    n_list = total;
    if (total) {
        HIP_TRY(hipMalloc(&list.p, 4ull * total));
        hipLaunchKernelGGL(k_consensus_list, dim3(blocks), dim3(kThreads), 0, stream, c->guides, c->n, c->cfg, which,
                           static_cast<const ulonglong2 *>(c->rows.p), counts, static_cast<uint32_t *>(list.p), total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return ISSL_OK;
}

int consensus_begin(const issl_guide_set *gs, const issl_consensus_config *cfg, issl_consensus **out)
{
    std::vector<SupportVector> table;
    if (cfg->sgrnascorer2) {
        table.resize(cfg->n_sv);
        for (uint32_t i = 0; i < cfg->n_sv; ++i) {
            SupportVector v{0, 0, 0, cfg->coef[i]};
            for (uint32_t b = 0; b < 80; ++b) {
                const uint8_t x = cfg->sv[80ull * i + b];
                if (x > 1) {
                    set_error("support vector " + std::to_string(i) + ", input " + std::to_string(b) + " is " + std::to_string(x) +
                              ": the kernel takes 0 / 1 rows");
                    return ISSL_E_UNSUPPORTED;
                }
                if (x && b < 64) v.lo |= 1ull << b;
                if (x && b >= 64) v.hi |= 1u << (b - 64);
            }
            table[i] = v;
        }
    }
    std::unique_ptr<issl_consensus> c(new issl_consensus());
    c->device = gs->device;
    c->n = static_cast<uint32_t>(gs->n_guides); // (a set has at most 2^32 - 1 matches)
    c->guides = static_cast<const ulonglong2 *>(gs->guides.p);
    c->cfg = Config{cfg->optimisation, cfg->n, cfg->mm10db, cfg->chopchop, cfg->sgrnascorer2, cfg->sgrnascorer2 ? cfg->n_sv : 0u,
                    cfg->intercept, cfg->sgrna_threshold, cfg->low_energy, cfg->high_energy};
    if (c->n) {
        if (int rc = select_device(c->device, "the extraction")) return rc;
        HIP_TRY(hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
        hipStream_t stream = c->stream.s;
        const uint32_t blocks = blocks_for(c->n, kThreads);
        HIP_TRY(hipMalloc(&c->rows.p, 32ull * c->n));
        HIP_TRY(hipMalloc(&c->counts.p, 4 * scan_words(blocks + 1ull)));
        if (!table.empty()) {
            HIP_TRY(hipMalloc(&c->sv.p, sizeof(SupportVector) * table.size()));
            HIP_TRY(hipMemcpyAsync(c->sv.p, table.data(), sizeof(SupportVector) * table.size(), hipMemcpyHostToDevice, stream));
        }
        uint32_t *counts = static_cast<uint32_t *>(c->counts.p);
        HIP_TRY(hipMemsetAsync(counts + blocks, 0, 4, stream));
        hipLaunchKernelGGL(k_consensus_begin, dim3(blocks), dim3(kThreads), 0, stream, c->guides, c->n, c->cfg,
                           static_cast<ulonglong2 *>(c->rows.p), counts);
        HIP_TRY(hipGetLastError());
        if (int rc = make_list(c.get(), kFoldList, c->fold_list, c->n_fold)) return rc; // (waits: the table may go)
    }
    *out = c.release();
    return ISSL_OK;
}

// folds: host memory, or with on_device the rows where issl_folds_read left them.
int consensus_finish(issl_consensus *c, const issl_fold *folds, bool on_device = false)
{
    if (c->n) {
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t stream = c->stream.s;
        const uint32_t blocks = blocks_for(c->n, kThreads);
        DevBuf d_folds;
        if (c->n_fold) {
            const uint32_t n_fold = static_cast<uint32_t>(c->n_fold);
            if (!on_device) {
                HIP_TRY(hipMalloc(&d_folds.p, 16ull * n_fold));
                HIP_TRY(hipMemcpyAsync(d_folds.p, folds, 16ull * n_fold, hipMemcpyHostToDevice, stream));
            }
            hipLaunchKernelGGL(k_consensus_fold, dim3(blocks_for(n_fold, kThreads)), dim3(kThreads), 0, stream, c->guides, c->n, c->cfg,
                               static_cast<const uint32_t *>(c->fold_list.p), on_device ? folds : static_cast<const issl_fold *>(d_folds.p), n_fold,
                               static_cast<issl_consensus_row *>(c->rows.p));
            HIP_TRY(hipGetLastError());
        }
        uint32_t *counts = static_cast<uint32_t *>(c->counts.p);
        HIP_TRY(hipMemsetAsync(counts + blocks, 0, 4, stream));
        hipLaunchKernelGGL(k_consensus_finish, dim3(blocks), dim3(kThreads), 0, stream, c->guides, c->n, c->cfg,
                           static_cast<const SupportVector *>(c->sv.p), static_cast<ulonglong2 *>(c->rows.p), counts);
        HIP_TRY(hipGetLastError());
        if (int rc = make_list(c, kSelection, c->selection, c->n_selected)) return rc; // (waits: the folds may go)
    }
    c->finished = true;
    return ISSL_OK;
}

int consensus_selection_pages(issl_consensus *c, uint64_t batch_size, uint64_t page_length, const uint64_t **d_page_starts,
                              uint64_t *n_pages)
{
    if (int rc = select_device(c->device, "the extraction")) return rc;
    c->pages.release();
    const uint64_t n = c->n;
    const uint32_t n_selected = static_cast<uint32_t>(c->n_selected);
    if (n == 0) { // no batch: no page, and the one boundary that ends them
        HIP_TRY(hipMalloc(&c->pages.p, 8));
        HIP_TRY(hipMemset(c->pages.p, 0, 8));
        *d_page_starts = static_cast<const uint64_t *>(c->pages.p);
        *n_pages = 0;
        return ISSL_OK;
    }
    hipStream_t stream = c->stream.s;
    const uint32_t n_batches = batch_size == 0 || batch_size >= n ? 1u : static_cast<uint32_t>((n + batch_size - 1) / batch_size);
    // a batch with r selected rows has at most r / page_length + 1 pages and none without a row
    const uint64_t by_length = page_length ? n_selected / page_length + n_batches : n_batches;
    const uint64_t cap = by_length < n_selected ? by_length : n_selected;
    Arena work;
    const size_t o_edges = work.reserve(4 * (n_batches + 1ull)), o_counts = work.reserve(4 * scan_words(n_batches + 1ull));
    HIP_TRY(hipMalloc(&work.buf.p, work.size));
    HIP_TRY(hipMalloc(&c->pages.p, 8 * (cap + 1)));
    uint32_t *edges = work.at<uint32_t>(o_edges), *counts = work.at<uint32_t>(o_counts);
    uint64_t *starts = static_cast<uint64_t *>(c->pages.p);
    HIP_TRY(hipMemsetAsync(counts + n_batches, 0, 4, stream));
    hipLaunchKernelGGL(k_pages_edges, dim3(static_cast<uint32_t>((n_batches + 1ull + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       static_cast<const uint32_t *>(c->selection.p), n_selected, n, batch_size, n_batches, edges);
    hipLaunchKernelGGL(k_pages_count, dim3(blocks_for(n_batches, kThreads)), dim3(kThreads), 0, stream, edges, n_batches, page_length, counts);
    launch_scan(counts, n_batches + 1ull, stream);
    hipLaunchKernelGGL(k_pages_fill, dim3(static_cast<uint32_t>((cap + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, edges,
                       counts, n_batches, page_length, n_selected, cap, starts);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + n_batches, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // the one wait: the boundaries are written and the work buffers may go
    if (total > cap) {
        set_error("pages on the device: " + std::to_string(total) + ", at most " + std::to_string(cap) + " expected");
        return ISSL_E_DEVICE;
    }
    *d_page_starts = starts;
    *n_pages = total;
    return ISSL_OK;
}

} // namespace

FoldSource consensus_fold_source(const issl_consensus *c)
{
    return FoldSource{c->device, c->guides, c->n, static_cast<const uint32_t *>(c->fold_list.p), c->n_fold};
}

RunlogSource consensus_runlog_source(const issl_consensus *c)
{
    return RunlogSource{c->device, c->finished, c->n, c->cfg.n, static_cast<const issl_consensus_row *>(c->rows.p),
                        static_cast<const uint32_t *>(c->fold_list.p), c->n_fold, static_cast<const uint32_t *>(c->selection.p),
                        c->n_selected};
}

} // namespace issl

extern "C" {

int issl_consensus_begin(const issl_guide_set *gs, const issl_consensus_config *cfg, issl_consensus **out)
{
    if (out) *out = nullptr;
    if (!gs || !cfg || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (cfg->optimisation > 3) return issl::fail(ISSL_E_ARG, "optimisation: 0 ultralow, 1 low, 2 medium, 3 high");
    if (cfg->sgrnascorer2 && cfg->n_sv == 0) return issl::fail(ISSL_E_ARG, "sgrnascorer2 is in the consensus and the model has no support vector");
    if (cfg->sgrnascorer2 && (!cfg->sv || !cfg->coef)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::consensus_begin(gs, cfg, out); });
}

int issl_consensus_fold_list(const issl_consensus *c, const uint32_t **d_rows, uint64_t *n_fold)
{
    if (!c || !d_rows || !n_fold) return issl::fail(ISSL_E_ARG, "null argument");
    *d_rows = static_cast<const uint32_t *>(c->fold_list.p);
    *n_fold = c->n_fold;
    return ISSL_OK;
}

int issl_consensus_fold_copy(const issl_consensus *c, uint32_t *rows, size_t cap)
{
    if (!c || (!rows && c->n_fold)) return issl::fail(ISSL_E_ARG, "null argument");
    if (cap < c->n_fold) {
        issl::set_error("room for " + std::to_string(cap) + " rows, the fold list has " + std::to_string(c->n_fold));
        return ISSL_E_ARG;
    }
    if (c->n_fold == 0) return ISSL_OK;
    return issl::abi_call([&] { return issl::copy_to_host(c->device, rows, c->fold_list.p, 4 * c->n_fold); });
}

int issl_consensus_finish(issl_consensus *c, const issl_fold *folds, size_t n_folds)
{
    if (!c) return issl::fail(ISSL_E_ARG, "null argument");
    if (c->finished) return issl::fail(ISSL_E_STATE, "the consensus is finished already");
    if (n_folds != c->n_fold) {
        issl::set_error(std::to_string(n_folds) + " folds for a fold list of " + std::to_string(c->n_fold));
        return ISSL_E_ARG;
    }
    if (!folds && n_folds) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::consensus_finish(c, folds); });
}

int issl_consensus_finish_folds(issl_consensus *c, const issl_folds *f)
{
    if (!c || !f) return issl::fail(ISSL_E_ARG, "null argument");
    if (f->consensus != c) return issl::fail(ISSL_E_ARG, "the folds belong to another consensus");
    if (c->finished) return issl::fail(ISSL_E_STATE, "the consensus is finished already");
    return issl::abi_call([&] { return issl::consensus_finish(c, static_cast<const issl_fold *>(f->folds.p), true); });
}

int issl_consensus_copy(const issl_consensus *c, issl_consensus_row *out, size_t cap)
{
    if (!c || (!out && c->n)) return issl::fail(ISSL_E_ARG, "null argument");
    if (!c->finished) return issl::fail(ISSL_E_STATE, "the consensus is not finished");
    if (cap < c->n) {
        issl::set_error("room for " + std::to_string(cap) + " rows, the set has " + std::to_string(c->n));
        return ISSL_E_ARG;
    }
    if (c->n == 0) return ISSL_OK;
    return issl::abi_call([&] { return issl::copy_to_host(c->device, out, c->rows.p, 32ull * c->n); });
}

int issl_consensus_device(const issl_consensus *c, const issl_consensus_row **d_rows, const uint32_t **d_selected, uint64_t *n_selected)
{
    if (!c || !d_rows || !d_selected || !n_selected) return issl::fail(ISSL_E_ARG, "null argument");
    if (!c->finished) return issl::fail(ISSL_E_STATE, "the consensus is not finished");
    *d_rows = static_cast<const issl_consensus_row *>(c->rows.p);
    *d_selected = static_cast<const uint32_t *>(c->selection.p);
    *n_selected = c->n_selected;
    return ISSL_OK;
}

int issl_consensus_selection_pages(issl_consensus *c, uint64_t batch_size, uint64_t page_length, const uint64_t **d_page_starts,
                                   uint64_t *n_pages)
{
    if (!c || !d_page_starts || !n_pages) return issl::fail(ISSL_E_ARG, "null argument");
    *d_page_starts = nullptr;
    *n_pages = 0;
    if (!c->finished) return issl::fail(ISSL_E_STATE, "the consensus is not finished");
    return issl::abi_call([&] { return issl::consensus_selection_pages(c, batch_size, page_length, d_page_starts, n_pages); });
}

int issl_consensus_close(issl_consensus *c)
{
    if (!c) return ISSL_OK;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    delete c;
    return ISSL_OK;
}

} // extern "C"
