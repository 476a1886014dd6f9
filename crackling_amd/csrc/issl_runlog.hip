// The counts of the run's log (issl_runlog_*, include/issl_hip.h): what Crackling.py:305-598 and :727-837 print per batch,
// counted over the rows the stages left on the device.
//   batches    k_runlog_edges: one thread per batch finds its share of the three ascending row lists (fold list, selection,
//              scored rows) by lower bounds and the number of its off-target pages; launch_scan turns those into the pages
//              ahead of every batch (k_runlog_page_spans writes them to the batches)
//   counts     one pass per list, one thread per row and kItems rows per thread: k_runlog_rows over the consensus rows (the
//              eight code bytes of a row are one 8-byte load), k_runlog_folds over the fold list, k_runlog_bowtie over the
//              selection, k_runlog_scored over the scored rows.  A row's batch is row / batch.  A workgroup whose rows all
//              lie in one batch -- every one but the few at a boundary once batches are larger than kChunk rows -- sums
//              in LDS and ends with one global atomic per counter; otherwise a wave whose lanes name one batch adds its
//              ballot's population with one atomic (a batch of exactly a wave), and a wave that straddles batches adds
//              lane by lane.  Integer sums: the same figures on every run
//   not found  the fold-list rows without an answer, ascending: counted per workgroup by k_runlog_folds, ranked by
//              launch_scan, written by k_runlog_not_found only when there is one
// The host waits once, for the two totals (pages, rows not found), and once more when rows are listed.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <string>

#include "../../include/issl_hip.h"
#include "issl_folds.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"
#include "issl_repr.hpp"
#include "issl_results.hpp"
#include "issl_runlog.hpp"

static_assert(sizeof(issl_runlog_batch) == 112, "issl_runlog_batch is 28 words");

namespace issl {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kItems = 8;                   // rows per thread
constexpr uint32_t kChunk = kThreads * kItems;   // rows per workgroup
constexpr uint32_t kWords = sizeof(issl_runlog_batch) / 4;

// The words of issl_runlog_batch the kernels add to.
enum Field : uint32_t {
    kLoaded = offsetof(issl_runlog_batch, loaded) / 4,
    kG20Tested = offsetof(issl_runlog_batch, g20_tested) / 4, kG20Failed = offsetof(issl_runlog_batch, g20_failed) / 4,
    kLeadTested = offsetof(issl_runlog_batch, lead_t_tested) / 4, kLeadFailed = offsetof(issl_runlog_batch, lead_t_failed) / 4,
    kAtTested = offsetof(issl_runlog_batch, at_tested) / 4, kAtFailed = offsetof(issl_runlog_batch, at_failed) / 4,
    kTtttTested = offsetof(issl_runlog_batch, tttt_tested) / 4, kTtttFailed = offsetof(issl_runlog_batch, tttt_failed) / 4,
    kSsTested = offsetof(issl_runlog_batch, ss_tested) / 4, kSsFailed = offsetof(issl_runlog_batch, ss_failed) / 4,
    kSsErred = offsetof(issl_runlog_batch, ss_erred) / 4, kSsNotFound = offsetof(issl_runlog_batch, ss_not_found) / 4,
    kMmAccepted = offsetof(issl_runlog_batch, mm10db_accepted) / 4, kMmFailed = offsetof(issl_runlog_batch, mm10db_failed) / 4,
    kSgTested = offsetof(issl_runlog_batch, sgrna_tested) / 4, kSgFailed = offsetof(issl_runlog_batch, sgrna_failed) / 4,
    kConsTested = offsetof(issl_runlog_batch, consensus_tested) / 4, kConsFailed = offsetof(issl_runlog_batch, consensus_failed) / 4,
    kBowtieRejected = offsetof(issl_runlog_batch, bowtie_rejected) / 4,
};

// First position of list[0..n) with list[p] >= row.
__device__ __forceinline__ uint32_t lower_bound(const uint32_t *__restrict__ list, uint32_t n, uint64_t row)
{
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (list[mid] < row) a = mid + 1;
        else b = mid;
    }
    return a;
}

// Batch b is rows [b * batch, min((b + 1) * batch, n)) of the set: its shares of the lists, its rows, its pages.
__global__ __launch_bounds__(kThreads) void k_runlog_edges(uint32_t n, uint64_t batch, uint32_t n_batches,
                                                           const uint32_t *__restrict__ fold_list, uint32_t n_fold,
                                                           const uint32_t *__restrict__ selection, uint32_t n_selected,
                                                           const uint32_t *__restrict__ scored, uint32_t n_scored, uint64_t page_length,
                                                           issl_runlog_batch *__restrict__ batches, uint32_t *__restrict__ pages)
{
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= n_batches) return;
    const uint64_t lo = b * batch;                                  // (below n < 2^32)
    const uint64_t hi = lo + batch < n ? lo + batch : n;
    issl_runlog_batch &out = batches[b];
    out.loaded = static_cast<uint32_t>(hi - lo);
    out.fold_first = lower_bound(fold_list, n_fold, lo);
    out.fold_end = lower_bound(fold_list, n_fold, hi);
    out.selected_first = lower_bound(selection, n_selected, lo);
    out.selected_end = lower_bound(selection, n_selected, hi);
    const uint32_t first = lower_bound(scored, n_scored, lo), end = lower_bound(scored, n_scored, hi);
    out.scored_first = first;
    out.scored_end = end;
    pages[b] = page_length ? static_cast<uint32_t>((end - first + page_length - 1) / page_length) : 1u;
}

// first[b] = pages ahead of batch b (the scanned counts), first[n_batches] = all pages.
__global__ __launch_bounds__(kThreads) void k_runlog_page_spans(const uint32_t *__restrict__ first, uint32_t n_batches,
                                                                issl_runlog_batch *__restrict__ batches)
{
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= n_batches) return;
    batches[b].page_first = first[b];
    batches[b].page_end = first[b + 1];
}

// Where a workgroup's counts go.  `one`: every row of the workgroup names slot `slot0`; its counts are summed in `lds`
// (`width` counters, cleared here) and flush() adds them to the slot's counters with one atomic each.
struct Tally {
    uint32_t *lds;
    bool one;

    __device__ __forceinline__ void begin(uint32_t width)
    {
        if (threadIdx.x < width) lds[threadIdx.x] = 0;
        __syncthreads();
    }
    // One for every lane whose flag is set, to counter `field` of the lane's slot.  Reached by all lanes of the wave;
    // `slot` is valid in every lane, also where flag is false.
    __device__ __forceinline__ void add(uint32_t *__restrict__ counters, uint32_t width, uint64_t slot, uint32_t field, bool flag) const
    {
        const bool wave_one = one || __all(slot == static_cast<uint64_t>(__shfl(static_cast<unsigned long long>(slot), 0)));
        uint32_t *cell = one ? lds + field : counters + slot * width + field;
        if (wave_one) {
            const uint64_t m = __ballot(flag);
            if (m && (threadIdx.x & 63u) == 0) atomicAdd(cell, static_cast<uint32_t>(__popcll(m)));
        } else if (flag) {
            atomicAdd(cell, 1u);
        }
    }
    __device__ __forceinline__ void flush(uint32_t *__restrict__ counters, uint32_t width, uint64_t slot0) const
    {
        __syncthreads();
        if (one && threadIdx.x < width && lds[threadIdx.x]) atomicAdd(counters + slot0 * width + threadIdx.x, lds[threadIdx.x]);
    }
};

// The consensus rows: everything of the table but the secondary structure.  codes[4 j + 3] holds row j's eight code bytes.
__global__ __launch_bounds__(kThreads) void k_runlog_rows(const uint64_t *__restrict__ codes, uint32_t n, uint64_t batch,
                                                          uint32_t consensus_n, uint32_t *__restrict__ counters)
{
    __shared__ uint32_t lds[kWords];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kChunk;
    const uint64_t last = base + kChunk - 1 < n ? base + kChunk - 1 : n - 1ull;
    const uint64_t slot0 = base / batch;
    Tally t{lds, slot0 == last / batch};
    t.begin(kWords);
    for (uint32_t it = 0; it < kItems; ++it) {
        const uint64_t j = base + it * kThreads + threadIdx.x;
        const bool valid = j < n;
        const uint64_t jj = valid ? j : n - 1ull;
        const uint64_t w = codes[4 * jj + 3];
        const uint32_t g20 = w & 0xFFu, lead = (w >> 8) & 0xFFu, at = (w >> 16) & 0xFFu, tttt = (w >> 24) & 0xFFu,
                       mm = (w >> 40) & 0xFFu, sg = (w >> 48) & 0xFFu, count = static_cast<uint32_t>(w >> 56);
        const uint64_t slot = jj / batch;
        t.add(counters, kWords, slot, kG20Tested, valid && g20 <= 1u);
        t.add(counters, kWords, slot, kG20Failed, valid && g20 == 0u);
        t.add(counters, kWords, slot, kLeadTested, valid && lead <= 1u);
        t.add(counters, kWords, slot, kLeadFailed, valid && lead == 0u);
        t.add(counters, kWords, slot, kAtTested, valid && at <= 1u);
        t.add(counters, kWords, slot, kAtFailed, valid && at == 0u);
        t.add(counters, kWords, slot, kTtttTested, valid && tttt <= 1u);
        t.add(counters, kWords, slot, kTtttFailed, valid && tttt == 0u);
        t.add(counters, kWords, slot, kMmAccepted, valid && mm == 1u);
        t.add(counters, kWords, slot, kMmFailed, valid && mm != 1u);
        t.add(counters, kWords, slot, kSgTested, valid && sg <= 1u);
        t.add(counters, kWords, slot, kSgFailed, valid && sg == 0u);
        t.add(counters, kWords, slot, kConsTested, valid);
        t.add(counters, kWords, slot, kConsFailed, valid && count < consensus_n);
    }
    t.flush(counters, kWords, slot0);
}

// Row i of the fold list has no answer: present == 0 in its fold, or, without folds, the code the consensus leaves then.
__device__ __forceinline__ bool fold_not_found(const issl_fold *__restrict__ folds, uint64_t i, uint32_t ss)
{
    return folds ? folds[i].present == 0u : ss == 2u;
}

// The fold list: the secondary structure's figures, and not_found[workgroup] = its rows without an answer.
__global__ __launch_bounds__(kThreads) void k_runlog_folds(const uint32_t *__restrict__ fold_list, uint32_t n_fold,
                                                           const issl_fold *__restrict__ folds, const uint64_t *__restrict__ codes,
                                                           uint64_t batch, uint32_t *__restrict__ counters,
                                                           uint32_t *__restrict__ not_found)
{
    __shared__ uint32_t lds[kWords];
    __shared__ uint32_t missing;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kChunk;
    const uint64_t last = base + kChunk - 1 < n_fold ? base + kChunk - 1 : n_fold - 1ull;
    const uint64_t slot0 = fold_list[base] / batch;
    Tally t{lds, slot0 == fold_list[last] / batch};
    if (threadIdx.x == 0) missing = 0;
    t.begin(kWords);
    for (uint32_t it = 0; it < kItems; ++it) {
        const uint64_t i = base + it * kThreads + threadIdx.x;
        const bool valid = i < n_fold;
        const uint64_t ii = valid ? i : n_fold - 1ull;
        const uint32_t row = fold_list[ii];
        const uint32_t ss = (codes[4ull * row + 3] >> 32) & 0xFFu;
        const bool absent = valid && fold_not_found(folds, ii, ss);
        const uint64_t slot = row / batch;
        t.add(counters, kWords, slot, kSsTested, valid && ss <= 1u);
        t.add(counters, kWords, slot, kSsFailed, valid && ss == 0u);
        t.add(counters, kWords, slot, kSsErred, valid && ss == 3u);
        t.add(counters, kWords, slot, kSsNotFound, absent);
        const uint64_t m = __ballot(absent);
        if (m && (threadIdx.x & 63u) == 0) atomicAdd(&missing, static_cast<uint32_t>(__popcll(m)));
    }
    t.flush(counters, kWords, slot0);
    if (threadIdx.x == 0) not_found[blockIdx.x] = missing; // (behind flush's barrier)
}

// first[g] = rows without an answer ahead of workgroup g's chunk: their positions in the fold list into list[0..total).
__global__ __launch_bounds__(kThreads) void k_runlog_not_found(const uint32_t *__restrict__ fold_list, uint32_t n_fold,
                                                               const issl_fold *__restrict__ folds, const uint64_t *__restrict__ codes,
                                                               const uint32_t *__restrict__ first, uint32_t total,
                                                               uint32_t *__restrict__ list)
{
    __shared__ uint32_t wave_n[kThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kChunk;
    uint32_t run = first[blockIdx.x];
    for (uint32_t it = 0; it < kItems; ++it) {
        const uint64_t i = base + it * kThreads + threadIdx.x;
        bool absent = false;
        if (i < n_fold) absent = fold_not_found(folds, i, (codes[4ull * fold_list[i] + 3] >> 32) & 0xFFu);
        const uint64_t m = __ballot(absent);
        if (lane == 0) wave_n[wave] = static_cast<uint32_t>(__popcll(m));
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            if (w < wave) before += wave_n[w];
            all += wave_n[w];
        }
        const uint32_t at = run + before + lanes_before(m);
        if (absent && at < total) list[at] = static_cast<uint32_t>(i);
        run += all;
        __syncthreads();
    }
}

// The selection: the rows the Bowtie step ends rejected.  code_of[32 k + 21] is the code of occurrence row k.
__global__ __launch_bounds__(kThreads) void k_runlog_bowtie(const uint32_t *__restrict__ selection, uint32_t n_selected,
                                                            const issl_occurrence *__restrict__ occ, uint64_t batch,
                                                            uint32_t *__restrict__ counters)
{
    __shared__ uint32_t lds[kWords];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kChunk;
    const uint64_t last = base + kChunk - 1 < n_selected ? base + kChunk - 1 : n_selected - 1ull;
    const uint64_t slot0 = selection[base] / batch;
    Tally t{lds, slot0 == selection[last] / batch};
    t.begin(kWords);
    for (uint32_t it = 0; it < kItems; ++it) {
        const uint64_t k = base + it * kThreads + threadIdx.x;
        const bool valid = k < n_selected;
        const uint64_t kk = valid ? k : n_selected - 1ull;
        t.add(counters, kWords, selection[kk] / batch, kBowtieRejected, valid && occ[kk].code == 0u);
    }
    t.flush(counters, kWords, slot0);
}

struct ScoreRule {
    double threshold;
    uint32_t rule, print_mit, print_cfd;
};

// The page of scored row k: those ahead of its batch and the full pages of the batch's share ahead of it.
__device__ __forceinline__ uint64_t page_of(uint64_t k, uint32_t row, uint64_t batch, uint64_t page_length,
                                            const issl_runlog_batch *__restrict__ batches)
{
    const issl_runlog_batch &b = batches[row / batch];
    return b.page_first + (page_length ? (k - b.scored_first) / page_length : 0u);
}

// The scored rows: page_failed[p] = rows of page p the rule rejects (issl_results.hip's verdict).
__global__ __launch_bounds__(kThreads) void k_runlog_scored(const uint32_t *__restrict__ scored, uint32_t n_scored,
                                                            const double *__restrict__ mit, const double *__restrict__ cfd,
                                                            ScoreRule rule, uint64_t batch, uint64_t page_length,
                                                            const issl_runlog_batch *__restrict__ batches, uint32_t n_pages_cap,
                                                            uint32_t *__restrict__ page_failed)
{
    __shared__ uint32_t lds[1];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kChunk;
    const uint64_t last = base + kChunk - 1 < n_scored ? base + kChunk - 1 : n_scored - 1ull;
    const uint64_t slot0 = page_of(base, scored[base], batch, page_length, batches);
    Tally t{lds, slot0 == page_of(last, scored[last], batch, page_length, batches)};
    t.begin(1);
    for (uint32_t it = 0; it < kItems; ++it) {
        const uint64_t k = base + it * kThreads + threadIdx.x;
        const bool valid = k < n_scored;
        const uint64_t kk = valid ? k : n_scored - 1ull;
        const double a = rule.print_mit ? through_text(mit[kk]) : -1.0, c = rule.print_cfd ? through_text(cfd[kk]) : -1.0;
        const double th = rule.threshold;
        bool reject;
        switch (rule.rule) {
        case kRuleNone: reject = false; break;
        case kRuleMit: reject = a < th; break;
        case kRuleCfd: reject = c < th; break;
        case kRuleAnd: reject = a < th && c < th; break;
        case kRuleOr: reject = a < th || c < th; break;
        default: reject = __ddiv_rn(__dadd_rn(a, c), 2.0) < th; break;
        }
        uint64_t slot = page_of(kk, scored[kk], batch, page_length, batches);
        if (slot >= n_pages_cap) { slot = 0; reject = false; } // (never: the host sized the array for every page)
        t.add(page_failed, 1, slot, 0, valid && reject);
    }
    t.flush(page_failed, 1, slot0 < n_pages_cap ? slot0 : 0);
}

uint32_t chunks_of(uint64_t n) { return static_cast<uint32_t>((n + kChunk - 1) / kChunk); }

} // namespace
} // namespace issl

struct issl_runlog {
    int device = -1;
    uint64_t n_batches = 0, n_pages = 0, n_not_found = 0;
    issl::DevBuf batches, page_failed, not_found; // n_batches structures, n_pages and n_not_found words
    float ms = 0;
};

namespace issl {
namespace {

struct Inputs {
    RunlogSource src;
    const issl_fold *folds;
    const issl_occurrence *d_bowtie;
    const uint32_t *d_scored;
    const double *d_mit, *d_cfd;
    uint32_t n_scored;
    ScoreRule rule;
    uint64_t batch_size, page_length;
};

int runlog_batches(const Inputs &in, issl_runlog **out)
{
    std::unique_ptr<issl_runlog> r(new issl_runlog());
    const RunlogSource &src = in.src;
    r->device = src.device;
    const uint32_t n = src.n;
    if (n == 0) { // no row, no batch
        *out = r.release();
        return ISSL_OK;
    }
    if (int rc = select_device(src.device, "the extraction")) return rc;
    const uint64_t batch = in.batch_size == 0 || in.batch_size >= n ? n : in.batch_size;
    const uint32_t n_batches = static_cast<uint32_t>((n + batch - 1) / batch);
    const uint32_t n_fold = static_cast<uint32_t>(src.n_fold), n_selected = static_cast<uint32_t>(src.n_selected), n_scored = in.n_scored;
    // a batch with s scored rows has at most s / page_length + 1 pages
    const uint64_t page_cap = in.page_length ? n_scored / in.page_length + n_batches : n_batches;
    if (page_cap > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 off-target pages");
        return ISSL_E_UNSUPPORTED;
    }
    const uint32_t fold_chunks = chunks_of(n_fold);
    OwnedStream stream;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    Arena work;
    const size_t o_pages = work.reserve(4 * scan_words(n_batches + 1ull)), o_missing = work.reserve(4 * scan_words(fold_chunks + 1ull));
    HIP_TRY(hipMalloc(&work.buf.p, work.size));
    HIP_TRY(hipMalloc(&r->batches.p, sizeof(issl_runlog_batch) * static_cast<size_t>(n_batches)));
    HIP_TRY(hipMalloc(&r->page_failed.p, 4 * page_cap));
    uint32_t *pages = work.at<uint32_t>(o_pages), *missing = work.at<uint32_t>(o_missing);
    issl_runlog_batch *batches = static_cast<issl_runlog_batch *>(r->batches.p);
    uint32_t *counters = static_cast<uint32_t *>(r->batches.p), *page_failed = static_cast<uint32_t *>(r->page_failed.p);
    const uint64_t *codes = reinterpret_cast<const uint64_t *>(src.rows);

    Events<2> ev;
    if (int rc = ev.create()) return rc;
    HIP_TRY(hipEventRecord(ev.e[0], stream.s));
    HIP_TRY(hipMemsetAsync(r->batches.p, 0, sizeof(issl_runlog_batch) * static_cast<size_t>(n_batches), stream.s));
    HIP_TRY(hipMemsetAsync(r->page_failed.p, 0, 4 * page_cap, stream.s));
    HIP_TRY(hipMemsetAsync(pages + n_batches, 0, 4, stream.s));
    HIP_TRY(hipMemsetAsync(missing + fold_chunks, 0, 4, stream.s));
    hipLaunchKernelGGL(k_runlog_edges, dim3(blocks_for(n_batches, kThreads)), dim3(kThreads), 0, stream.s, n, batch, n_batches, src.fold_list, n_fold,
                       src.selection, n_selected, in.d_scored, n_scored, in.page_length, batches, pages);
    launch_scan(pages, n_batches + 1ull, stream.s);
    hipLaunchKernelGGL(k_runlog_page_spans, dim3(blocks_for(n_batches, kThreads)), dim3(kThreads), 0, stream.s, pages, n_batches, batches);
    hipLaunchKernelGGL(k_runlog_rows, dim3(chunks_of(n)), dim3(kThreads), 0, stream.s, codes, n, batch, src.consensus_n, counters);
    if (n_fold) {
        hipLaunchKernelGGL(k_runlog_folds, dim3(fold_chunks), dim3(kThreads), 0, stream.s, src.fold_list, n_fold, in.folds, codes, batch,
                           counters, missing);
        launch_scan(missing, fold_chunks + 1ull, stream.s);
    }
    if (in.d_bowtie && n_selected)
        hipLaunchKernelGGL(k_runlog_bowtie, dim3(chunks_of(n_selected)), dim3(kThreads), 0, stream.s, src.selection, n_selected,
                           in.d_bowtie, batch, counters);
    if (n_scored)
        hipLaunchKernelGGL(k_runlog_scored, dim3(chunks_of(n_scored)), dim3(kThreads), 0, stream.s, in.d_scored, n_scored, in.d_mit,
                           in.d_cfd, in.rule, batch, in.page_length, batches, static_cast<uint32_t>(page_cap), page_failed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], stream.s));
    uint32_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&totals[0], pages + n_batches, 4, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipMemcpyAsync(&totals[1], missing + fold_chunks, 4, hipMemcpyDeviceToHost, stream.s));
    HIP_TRY(hipStreamSynchronize(stream.s)); // the one wait: the counts are there
    HIP_TRY(hipEventElapsedTime(&r->ms, ev.e[0], ev.e[1]));
    if (totals[0] > page_cap || totals[1] > n_fold) {
        set_error("log counts on the device: " + std::to_string(totals[0]) + " pages, at most " + std::to_string(page_cap) +
                  " expected; " + std::to_string(totals[1]) + " rows not found in a fold list of " + std::to_string(n_fold));
        return ISSL_E_DEVICE;
    }
    r->n_batches = n_batches;
    r->n_pages = totals[0];
    r->n_not_found = totals[1];
    if (totals[1]) {
        HIP_TRY(hipMalloc(&r->not_found.p, 4ull * totals[1]));
        hipLaunchKernelGGL(k_runlog_not_found, dim3(fold_chunks), dim3(kThreads), 0, stream.s, src.fold_list, n_fold, in.folds, codes,
                           missing, totals[1], static_cast<uint32_t *>(r->not_found.p));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream.s));
    }
    *out = r.release();
    return ISSL_OK;
}

int runlog_copy(const issl_runlog *r, issl_runlog_batch *batches, uint32_t *page_failed, uint32_t *not_found)
{
    HIP_TRY(hipSetDevice(r->device));
    if (batches && r->n_batches)
        HIP_TRY(hipMemcpy(batches, r->batches.p, sizeof(issl_runlog_batch) * r->n_batches, hipMemcpyDeviceToHost));
    if (page_failed && r->n_pages) HIP_TRY(hipMemcpy(page_failed, r->page_failed.p, 4 * r->n_pages, hipMemcpyDeviceToHost));
    if (not_found && r->n_not_found) HIP_TRY(hipMemcpy(not_found, r->not_found.p, 4 * r->n_not_found, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_runlog_batches(const issl_consensus *c, const issl_folds *f, const issl_occurrence *d_bowtie, size_t n_bowtie,
                        const uint32_t *d_scored, const double *d_mit, const double *d_cfd, size_t n_scored, double threshold,
                        const char *method, uint64_t batch_size, uint64_t offtarget_page_length, issl_runlog **out)
{
    if (out) *out = nullptr;
    if (!c || !method || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (f && f->consensus != c) return issl::fail(ISSL_E_ARG, "the folds belong to another consensus");
    issl::Inputs in{};
    in.src = issl::consensus_runlog_source(c);
    if (!in.src.finished) return issl::fail(ISSL_E_STATE, "the consensus is not finished");
    if ((d_bowtie || n_bowtie) && (!d_bowtie || n_bowtie != in.src.n_selected)) {
        issl::set_error(std::to_string(n_bowtie) + " rows of the Bowtie step for a selection of " + std::to_string(in.src.n_selected));
        return ISSL_E_ARG;
    }
    if (n_scored && (!d_scored || !d_mit || !d_cfd)) return issl::fail(ISSL_E_ARG, "scored rows without their list or one of the scores");
    if (n_scored > in.src.n) {
        issl::set_error(std::to_string(n_scored) + " scored rows, the set has " + std::to_string(in.src.n));
        return ISSL_E_ARG;
    }
    return issl::abi_call([&] {
        issl::ResultArgs a{};
        issl::method_rules(method, a);
        in.folds = f ? static_cast<const issl_fold *>(f->folds.p) : nullptr;
        in.d_bowtie = d_bowtie;
        in.d_scored = d_scored;
        in.d_mit = d_mit;
        in.d_cfd = d_cfd;
        in.n_scored = static_cast<uint32_t>(n_scored);
        in.rule = issl::ScoreRule{threshold, a.rule, a.print_mit, a.print_cfd};
        in.batch_size = batch_size;
        in.page_length = offtarget_page_length;
        return issl::runlog_batches(in, out);
    });
}

int issl_runlog_info(const issl_runlog *r, uint64_t *n_batches, uint64_t *n_pages, uint64_t *n_not_found, double *ms)
{
    if (!r) return issl::fail(ISSL_E_ARG, "null argument");
    if (n_batches) *n_batches = r->n_batches;
    if (n_pages) *n_pages = r->n_pages;
    if (n_not_found) *n_not_found = r->n_not_found;
    if (ms) *ms = r->ms;
    return ISSL_OK;
}

int issl_runlog_copy(const issl_runlog *r, issl_runlog_batch *batches, size_t cap_batches, uint32_t *page_failed,
                     size_t cap_pages, uint32_t *not_found, size_t cap_not_found)
{
    if (!r) return issl::fail(ISSL_E_ARG, "null argument");
    if ((batches && cap_batches < r->n_batches) || (page_failed && cap_pages < r->n_pages) || (not_found && cap_not_found < r->n_not_found)) {
        issl::set_error("room for " + std::to_string(cap_batches) + " batches, " + std::to_string(cap_pages) + " pages and " +
                        std::to_string(cap_not_found) + " rows; there are " + std::to_string(r->n_batches) + ", " +
                        std::to_string(r->n_pages) + " and " + std::to_string(r->n_not_found));
        return ISSL_E_ARG;
    }
    if (r->n_batches == 0) return ISSL_OK;
    return issl::abi_call([&] { return issl::runlog_copy(r, batches, page_failed, not_found); });
}

int issl_runlog_close(issl_runlog *r)
{
    if (!r) return ISSL_OK;
    if (r->device >= 0 && r->n_batches) (void)hipSetDevice(r->device);
    delete r;
    return ISSL_OK;
}

} // extern "C"
