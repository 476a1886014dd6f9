// The result table's kernels (issl_results_*, include/issl_hip.h): Crackling.py:842-852 as a two-pass text writer over the
// rows of a guide set.
//   measure  k_results_measure: one thread per row walks the row's fields into a sink that only counts; a workgroup's 256
//            lengths are summed (block_exclusive_scan, 64-bit) into the rows' places inside the group and the group's bytes
//   scan     k_results_scan: one workgroup turns the groups' bytes into their places in the text, behind the header row
//   emit     k_results_emit: the same walk into a sink that writes.  A workgroup's rows are one contiguous span of the text:
//            as many consecutive rows as fit kResultStage bytes are written into LDS -- at the span's own alignment modulo
//            16 -- and the span leaves with 16-byte stores, all lanes on consecutive addresses; then the next rows.  A row
//            that alone is larger than the buffer (a header name has no bound) is stored by its thread straight to global
//            memory, as every row is with ISSL_RESULTS_DIRECT.  Both ways run the same field code, so what was measured
//            is what is written.
// A table may hold a run of rows of the set (issl_results_build_rows: the text leaves the device a batch at a time): row j of
// the text is row a.first + j of the set in measure and emit; the three inversions stay those of the whole set.
// Numbers are formatted in registers (issl_repr.hpp: digits as four-bit fields of a word, no per-thread array); a row
// costs two shortest-digit conversions per float it prints, one to measure and one to write.
#include <hip/hip_runtime.h>

#include "issl_kernels.hpp"
#include "issl_repr.hpp"
#include "issl_results.hpp"

#define ISSL_REPR_QUAL __device__ const
#include "repr_tables.inc"
static_assert(ISSL_REPR_POW10_MIN == issl::kReprPow10Min && ISSL_REPR_POW10_MAX == issl::kReprPow10Max, "repr_tables.inc");

namespace issl {
namespace {

static_assert(kResultRows == 256, "block_exclusive_scan works on 256 threads");
static_assert(sizeof(issl_text_span) == 16 && sizeof(issl_guide) == 32 && sizeof(issl_consensus_row) == 32 &&
              sizeof(issl_occurrence) == 32, "the rows are read as laid out in issl_hip.h");

__device__ __forceinline__ void put_text(CountSink &s, const char *, uint64_t len) { s.n += len; }
__device__ __forceinline__ void put_text(WriteSink &s, const char *src, uint64_t len)
{
    for (uint64_t i = 0; i < len; ++i) s.p[i] = src[i];
    s.p += len;
}

// A span of the pool, or '?'.
template <class Sink> __device__ __forceinline__ void put_span(Sink &s, const ResultArgs &a, const issl_text_span &t)
{
    if (t.length == 0xFFFFFFFFu) s.put('?');
    else put_text(s, a.pool + t.offset, t.length);
}

// A span of an issl_folds' text, or '?': RNAfold's bytes as they stand, quoted here as csv_append (issl_results_text.hpp)
// quotes on the host -- with the delimiter, '"', LF or CR inside, an embedded '"' doubled.  Whether it has one of them the
// read has noted in the span (issl_folds_text.hpp, quote_bits): a field without -- every one of RNAfold's under ',' -- is
// measured without a look at its text and copied in one pass.
template <class Sink> __device__ __forceinline__ void put_fold_span(Sink &s, const ResultArgs &a, const issl_text_span &t)
{
    if (t.length == 0xFFFFFFFFu) {
        s.put('?');
        return;
    }
    const char *src = a.fold_text + t.offset;
    if (!(t.reserved & a.fold_quote)) {
        put_text(s, src, t.length);
        return;
    }
    s.put('"');
    for (uint32_t i = 0; i < t.length; ++i) {
        if (src[i] == '"') s.put('"');
        s.put(src[i]);
    }
    s.put('"');
}

template <class Sink> __device__ __forceinline__ void put_code(Sink &s, uint32_t code)
{
    s.put(static_cast<char>(0x213F3130u >> (8 * (code & 3u)))); // 0 1 ? !
}

template <class Sink> __device__ __forceinline__ void put_float(Sink &s, double v)
{
    if (v != v) s.put('?'); // NaN: the reference never assigned it
    else put_repr(s, v, issl_repr_pow10);
}

// Row j of the set: the 26 columns of Constants.py:42-70 in their order, and the line end.
template <class Sink> __device__ void put_row(Sink &s, const ResultArgs &a, uint32_t j)
{
    const issl_guide g = a.guides[j];
    const issl_consensus_row r = a.rows[j];
    const char d = a.delimiter;
    for (uint32_t p = 0; p < 23; ++p) s.put(static_cast<char>(0x54474341u >> (8 * ((g.guide23 >> (2 * p)) & 3u)))); // A C G T
    s.put(d);
    if (a.no_sgrna) s.put('?');
    else put_float(s, r.sgrna_score);
    s.put(d);
    if (g.seen == 1u) {
        if (g.record < a.n_headers) put_span(s, a, a.headers[g.record]);
        else s.put('?'); // (no such record: not a row of this set)
        s.put(d);
        put_u64(s, g.start);
        s.put(d);
        put_u64(s, g.start + 23u);
        s.put(d);
        s.put(g.strand ? '-' : '+');
        s.put(d);
        s.put('1');
    } else {
        for (uint32_t k = 0; k < 4; ++k) { s.put('-'); s.put(d); }
        s.put('0');
    }
    s.put(d);
    put_code(s, r.g20);
    s.put(d);
    put_code(s, r.tttt);
    s.put(d);
    put_code(s, r.at_pct);
    s.put(d);
    put_code(s, r.ss);
    s.put(d);
    uint32_t f = a.fold_of ? a.fold_of[j] : kNoRow;
    if (f >= a.n_fold) f = kNoRow;
    for (uint32_t k = 0; k < 3; ++k) {
        if (f == kNoRow) s.put('?');
        else if (a.fold_text) put_fold_span(s, a, a.ss[3ull * f + k]);
        else put_span(s, a, a.ss[3ull * f + k]);
        s.put(d);
    }
    put_code(s, r.mm10db);
    s.put(d);
    put_code(s, r.sgrna);
    s.put(d);
    s.put(static_cast<char>('0' + r.count % 10u));
    s.put(d);
    // the Bowtie step's row and the scores, read once for the columns they fill further on
    const uint32_t b = a.sel_of ? a.sel_of[j] : kNoRow;
    issl_occurrence occ;
    occ.code = 2;
    if (b < a.n_sel) occ = a.occ[b];
    const bool tested = occ.code != 2 && (occ.record == 0xFFFFFFFFu || occ.record < a.n_chr);
    uint32_t k = a.score_of ? a.score_of[j] : kNoRow;
    if (k >= a.n_scored) k = kNoRow;
    double mit = -1.0, cfd = -1.0;
    if (k != kNoRow) {
        if (a.print_mit) mit = through_text(a.mit[k]);
        if (a.print_cfd) cfd = through_text(a.cfd[k]);
    }
    if (tested) put_code(s, occ.code);
    else s.put('?');
    s.put(d);
    if (k == kNoRow || a.rule == kRuleNone) {
        s.put('?');
    } else {
        const double t = a.threshold;
        bool reject;
        switch (a.rule) {
        case kRuleMit: reject = mit < t; break;
        case kRuleCfd: reject = cfd < t; break;
        case kRuleAnd: reject = mit < t && cfd < t; break;
        case kRuleOr: reject = mit < t || cfd < t; break;
        default: reject = __ddiv_rn(__dadd_rn(mit, cfd), 2.0) < t; break;
        }
        s.put(reject ? '0' : '1');
    }
    s.put(d);
    put_float(s, r.at);
    s.put(d);
    if (!tested) {
        s.put('?'); s.put(d); s.put('?'); s.put(d); s.put('?');
    } else if (occ.record == 0xFFFFFFFFu) {
        s.put('*'); s.put(d); s.put('0'); s.put(d); s.put('2'); s.put('2');
    } else {
        put_span(s, a, a.chr[occ.record]);
        s.put(d);
        put_u64(s, occ.pos + 1u);
        s.put(d);
        put_u64(s, occ.pos + 23u);
    }
    s.put(d);
    if (k == kNoRow) {
        s.put('?'); s.put(d); s.put('?');
    } else {
        put_repr(s, mit, issl_repr_pow10); // (a NaN score prints nan, as float("nan") would)
        s.put(d);
        put_repr(s, cfd, issl_repr_pow10);
    }
    s.put(d);
    put_code(s, r.lead_t);
    s.put('\n');
}

__global__ __launch_bounds__(256) void k_results_invert(const uint32_t *__restrict__ list, uint32_t n_list,
                                                        uint32_t *__restrict__ inverse, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t j = list[i];
    if (j < n) inverse[j] = i;
}

__global__ __launch_bounds__(kResultRows) void k_results_measure(ResultArgs a, uint64_t *__restrict__ offsets,
                                                                 uint64_t *__restrict__ sums)
{
    __shared__ uint64_t lds[256];
    const uint32_t j = blockIdx.x * kResultRows + threadIdx.x; // row a.first + j of the set is row j of the text
    CountSink s;
    if (j < a.n) put_row(s, a, a.first + j);
    uint64_t total;
    const uint64_t at = block_exclusive_scan(s.n, lds, &total);
    if (j < a.n) offsets[j] = at;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_results_scan(uint64_t *__restrict__ sums, uint32_t groups, uint64_t first,
                                                      uint64_t *__restrict__ offsets, uint32_t n)
{
    __shared__ uint64_t lds[256];
    uint64_t carry = first;
    for (uint32_t base = 0; base < groups; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t val = i < groups ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(val, lds, &total);
        if (i < groups) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        sums[groups] = carry;
        offsets[n] = carry;
    }
}

__global__ __launch_bounds__(kResultRows) void k_results_emit(ResultArgs a, uint64_t *__restrict__ offsets,
                                                              const uint64_t *__restrict__ sums, char *__restrict__ text,
                                                              uint32_t direct)
{
    __shared__ uint64_t s_off[kResultRows + 1];                // the rows' places inside the group's span
    __shared__ __attribute__((aligned(16))) char stage[kResultStage + 16];
    const uint32_t t = threadIdx.x, j = blockIdx.x * kResultRows + t;
    const uint64_t base = sums[blockIdx.x], bytes_all = sums[blockIdx.x + 1] - base;
    s_off[t] = j < a.n ? offsets[j] : bytes_all; // (rows beyond the set: empty, at the span's end)
    if (t == 0) s_off[kResultRows] = bytes_all;
    __syncthreads();
    const uint64_t my_start = s_off[t];
    if (j < a.n) offsets[j] = base + my_start;
    if (direct) {
        if (j < a.n) {
            WriteSink s{text + base + my_start};
            put_row(s, a, a.first + j);
        }
        return;
    }
    uint32_t first = 0;
    while (first < kResultRows) { // (every value that steers the loop is the same in all threads)
        const uint64_t w0 = s_off[first];
        // rows first .. last - 1 fit the buffer together: the largest `last` with s_off[last] - w0 <= kResultStage
        uint32_t lo = first, hi = kResultRows;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (s_off[mid] - w0 <= kResultStage) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t last = lo;
        if (last == first) { // this row alone is larger than the buffer
            if (t == first && j < a.n) {
                WriteSink s{text + base + my_start};
                put_row(s, a, a.first + j);
            }
            first += 1;
            continue;
        }
        const uint32_t shift = static_cast<uint32_t>(base + w0) & 15u; // the text pointer is 256-byte aligned
        if (t >= first && t < last && j < a.n) {
            WriteSink s{stage + shift + (my_start - w0)};
            put_row(s, a, a.first + j);
        }
        __syncthreads();
        const uint32_t bytes = static_cast<uint32_t>(s_off[last] - w0);
        char *g = text + base + w0;
        const char *src = stage + shift;
        const uint32_t to_align = (16u - shift) & 15u, head = bytes < to_align ? bytes : to_align;
        if (t < head) g[t] = src[t];
        const uint32_t body = (bytes - head) / 16u;
        for (uint32_t v = t; v < body; v += kResultRows)
            *reinterpret_cast<uint4 *>(g + head + 16u * v) = *reinterpret_cast<const uint4 *>(src + head + 16u * v);
        const uint32_t done = head + 16u * body;
        if (t < bytes - done) g[done + t] = src[done + t];
        __syncthreads();
        first = last;
    }
}

__global__ __launch_bounds__(256) void k_repr_f64(const double *__restrict__ values, uint64_t n, char *__restrict__ text,
                                                  uint32_t *__restrict__ len)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    char *out = text + 32u * i;
    WriteSink s{out};
    put_repr(s, values[i], issl_repr_pow10);
    const uint32_t used = static_cast<uint32_t>(s.p - out);
    for (uint32_t k = used; k < 32u; ++k) out[k] = 0;
    len[i] = used;
}

} // namespace

void launch_results_invert(const uint32_t *list, uint32_t n_list, uint32_t *inverse, uint32_t n, void *stream)
{
    if (!n_list) return;
    hipLaunchKernelGGL(k_results_invert, dim3((n_list + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), list,
                       n_list, inverse, n);
}

void launch_results_measure(const ResultArgs &a, uint64_t *offsets, uint64_t *sums, void *stream)
{
    hipLaunchKernelGGL(k_results_measure, dim3(result_groups(a.n)), dim3(kResultRows), 0, static_cast<hipStream_t>(stream), a,
                       offsets, sums);
}

void launch_results_scan(uint64_t *sums, uint32_t groups, uint64_t first, uint64_t *offsets, uint32_t n, void *stream)
{
    hipLaunchKernelGGL(k_results_scan, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sums, groups, first, offsets, n);
}

void launch_results_emit(const ResultArgs &a, uint64_t *offsets, const uint64_t *sums, char *text, bool direct, void *stream)
{
    hipLaunchKernelGGL(k_results_emit, dim3(result_groups(a.n)), dim3(kResultRows), 0, static_cast<hipStream_t>(stream), a,
                       offsets, sums, text, direct ? 1u : 0u);
}

void launch_repr(const double *values, size_t n, char *text, uint32_t *len, void *stream)
{
    if (!n) return;
    hipLaunchKernelGGL(k_repr_f64, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       values, static_cast<uint64_t>(n), text, len);
}

} // namespace issl
