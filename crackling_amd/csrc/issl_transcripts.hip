// Transcript hit counts (include/issl_hip.h, issl_annotation_*): countTranscripts of
// src/crackling/utils/countHitTranscripts.py:148-193 resolved once per position when the annotation is opened.
//
// The exon intervals of all transcripts (issl_annotation.cpp: disjoint per transcript) cut every sequence into elementary
// segments at their starts and their ends + 1.  Inside a segment the set of transcripts that contain a position does not
// change, so the reference's answer -- how many transcripts, which is the first, do they agree on a gene, how many mRNA
// lines does that gene have -- is one 16-byte row per segment.  Opening builds: the sorted distinct breakpoints (keys
// seq << 40 | coordinate), the first breakpoint of every sequence, per segment the list of covering transcripts (count,
// scan, fill) and from the lists the answers; the lists are freed, breakpoints and answers stay resident.  A query is a
// binary search among the breakpoints of its sequence.
//
// Spreading the cover passes: a lane takes one interval and finds its segment range [lo, hi) by two binary searches.
// Ranges below 64 segments are walked by the lane itself; every longer one is then walked by the whole wave, 64
// consecutive segments per step, so one long exon costs the wave (hi - lo) / 64 steps instead of hi - lo and its
// atomics go out as whole rows.  The answers pass treats the lists the same way: below 64 entries per lane, longer
// lists per wave with a shuffle reduction.  Min, max and the length are all an answer needs, so the order in which the
// fill pass's atomics placed the entries does not reach the result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "issl_annotation_device.hpp"
#include "issl_hiputil.hpp"
#include "issl_match.hpp"

namespace issl {
namespace {

constexpr uint32_t kWaveSpan = 64; // ranges and lists of this length or more are walked by the wave

// ---- distinct breakpoints ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_tr_heads(const uint64_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool head = i < n && (i == 0 || keys[i - 1] != keys[i]);
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// first[b]: heads ahead of block b.
__global__ __launch_bounds__(256) void k_tr_unique(const uint64_t *__restrict__ keys, uint32_t n, const uint32_t *__restrict__ first,
                                                   uint64_t *__restrict__ bp)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, wave = threadIdx.x >> 6;
    const bool head = i < n && (i == 0 || keys[i - 1] != keys[i]);
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    uint32_t before = first[blockIdx.x] + lanes_before(heads);
    for (uint32_t v = 0; v < wave; ++v) before += wave_cnt[v];
    if (head) bp[before] = keys[i];
}

__global__ __launch_bounds__(256) void k_tr_seq_first(const uint64_t *__restrict__ bp, uint32_t n_bp, uint32_t n_seqs,
                                                      uint32_t *__restrict__ seq_first)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s > n_seqs) return;
    seq_first[s] = first_not_below(bp, 0, n_bp, static_cast<uint64_t>(s) << kCoordBits);
}

// ---- cover lists ---------------------------------------------------------------------------------------------------

// kFill == false: cnt[j] += 1 for every segment j of every interval, *total += the segments of all intervals.
// kFill == true: cnt is the cursor of every segment (zeroed), off its list's start; the interval's transcript is appended.
template <bool kFill>
__global__ __launch_bounds__(256) void k_tr_cover(const uint64_t *__restrict__ lo_key, const uint64_t *__restrict__ hi_key,
                                                  const uint32_t *__restrict__ tr, uint32_t m, const uint64_t *__restrict__ bp,
                                                  uint32_t n_bp, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                  uint32_t *__restrict__ list, unsigned long long *__restrict__ total)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = 0, t = 0;
    if (i < m) { // both keys are breakpoints: the searches find them
        lo = first_not_below(bp, 0, n_bp, lo_key[i]);
        hi = first_not_below(bp, lo, n_bp, hi_key[i]);
        t = tr[i];
    }
    const uint32_t span = hi - lo;
    auto put = [&](uint32_t j, uint32_t who) {
        if (kFill) list[off[j] + atomicAdd(&cnt[j], 1u)] = who;
        else atomicAdd(&cnt[j], 1u);
    };
    if (!kFill) {
        unsigned long long sum = span;
        for (uint32_t d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0 && sum) atomicAdd(total, sum);
    }
    if (span < kWaveSpan)
        for (uint32_t j = lo; j < hi; ++j) put(j, t);
    for (uint64_t wide = __ballot(span >= kWaveSpan); wide; wide &= wide - 1) {
        const int src = __builtin_ctzll(wide);
        const uint32_t wlo = __shfl(lo, src, 64), whi = __shfl(hi, src, 64), wt = __shfl(t, src, 64);
        for (uint32_t j = wlo + lane; j < whi; j += 64) put(j, wt);
    }
}

// ---- answers -------------------------------------------------------------------------------------------------------

struct Fold {
    uint32_t first = kNone, gmin = kNone, gmax = 0; // least ordinal; least and greatest gene among the mapped ones
    __device__ __forceinline__ void add(uint32_t t, const uint32_t *__restrict__ tr_gene)
    {
        first = min(first, t);
        const uint32_t g = tr_gene[t];
        if (g != kNone) {
            gmin = min(gmin, g);
            gmax = max(gmax, g);
        }
    }
};

// off: n_bp + 1 list starts.  One row per segment; a segment nobody covers answers 0/0.
__global__ __launch_bounds__(256) void k_tr_answers(const uint32_t *__restrict__ off, const uint32_t *__restrict__ list, uint32_t n_bp,
                                                    const uint32_t *__restrict__ tr_gene, const uint32_t *__restrict__ gene_count,
                                                    uint4 *__restrict__ answers)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t a = 0, len = 0;
    if (j < n_bp) {
        a = off[j];
        len = off[j + 1] - a;
    }
    Fold f;
    if (len < kWaveSpan)
        for (uint32_t k = 0; k < len; ++k) f.add(list[a + k], tr_gene);
    for (uint64_t wide = __ballot(len >= kWaveSpan); wide; wide &= wide - 1) {
        const int src = __builtin_ctzll(wide);
        const uint32_t wa = __shfl(a, src, 64), wlen = __shfl(len, src, 64);
        Fold w;
        for (uint32_t k = lane; k < wlen; k += 64) w.add(list[wa + k], tr_gene);
        for (uint32_t d = 32; d; d >>= 1) {
            w.first = min(w.first, static_cast<uint32_t>(__shfl_xor(w.first, d, 64)));
            w.gmin = min(w.gmin, static_cast<uint32_t>(__shfl_xor(w.gmin, d, 64)));
            w.gmax = max(w.gmax, static_cast<uint32_t>(__shfl_xor(w.gmax, d, 64)));
        }
        if (static_cast<int>(lane) == src) f = w;
    }
    if (j >= n_bp) return;
    uint4 row = make_uint4(len, 0u, 0u, f.first); // hit, total, status, first
    if (len) {
        if (f.gmin != kNone && f.gmin != f.gmax) {
            row.z = 2u; // more than one gene
        } else {
            const uint32_t g = tr_gene[f.first];
            if (g == kNone) row.z = 3u; // the first hit transcript has no mRNA line
            else row.y = gene_count[g];
        }
    }
    answers[j] = row;
}

// ---- queries -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_tr_hits(View v, const uint32_t *__restrict__ seq, const long long *__restrict__ start, uint64_t n,
                                                 uint4 *__restrict__ out)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = answer_at(v, seq[i], start[i]);
}

// rows: issl_occurrence, two 16-byte halves each.  rec_seq: n_records + 1 entries, the last one for '*'.
__global__ __launch_bounds__(256) void k_tr_hits_rows(View v, const ulonglong2 *__restrict__ rows, uint64_t n,
                                                      const uint32_t *__restrict__ rec_seq, uint32_t n_records, uint4 *__restrict__ out)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 head = rows[2 * i]; // {pos; record, n_perfect}
    const uint32_t code = static_cast<uint32_t>(rows[2 * i + 1].x >> 40) & 0xFFu;
    if (code == 2u) {
        out[i] = make_uint4(0u, 0u, 1u, kNone);
        return;
    }
    const uint32_t record = static_cast<uint32_t>(head.y);
    const uint32_t seq = record == kNone ? rec_seq[n_records] : record < n_records ? rec_seq[record] : kNone;
    const uint64_t start = record == kNone ? 0 : head.x + 1; // bowtieStart: the reference prints '*', 0, 22 for a guide that does not occur
    out[i] = answer_at(v, seq, static_cast<long long>(start >> kCoordBits ? uint64_t(1) << kCoordBits : start));
}

// ---- host ----------------------------------------------------------------------------------------------------------

int build_device(issl_annotation *a, const AnnotationIntervals &iv)
{
    const uint32_t m = static_cast<uint32_t>(iv.tr.size()), n_keys = 2 * m, n_seqs = static_cast<uint32_t>(a->t.seqs.size());
    hipStream_t stream = nullptr;
    HIP_TRY(hipMalloc(&a->seq_first.p, 4ull * (n_seqs + 1)));
    HIP_TRY(hipMemset(a->seq_first.p, 0, 4ull * (n_seqs + 1)));
    if (m == 0) return ISSL_OK;
    // -- the distinct breakpoints
    const uint32_t blocks = (n_keys + 255) / 256, sort_blocks = radix_sort_blocks(n_keys);
    Arena ar;
    const size_t o_keys = ar.reserve(8ull * n_keys), o_tmp = ar.reserve(8ull * n_keys), o_hist = ar.reserve(4 * radix_hist_words(sort_blocks)),
                 o_first = ar.reserve(4 * scan_words(blocks + 1ull)), o_lo = ar.reserve(8ull * m), o_hi = ar.reserve(8ull * m),
                 o_tr = ar.reserve(4ull * m), o_total = ar.reserve(8);
    HIP_TRY(hipMalloc(&ar.buf.p, ar.size));
    uint64_t *keys = ar.at<uint64_t>(o_keys), *tmp = ar.at<uint64_t>(o_tmp), *d_lo = ar.at<uint64_t>(o_lo), *d_hi = ar.at<uint64_t>(o_hi);
    uint32_t *hist = ar.at<uint32_t>(o_hist), *first = ar.at<uint32_t>(o_first), *d_tr = ar.at<uint32_t>(o_tr);
    unsigned long long *d_total = ar.at<unsigned long long>(o_total);
    HIP_TRY(hipMemcpy(d_lo, iv.lo.data(), 8ull * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_hi, iv.hi.data(), 8ull * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_tr, iv.tr.data(), 4ull * m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(keys, d_lo, 8ull * m, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(keys + m, d_hi, 8ull * m, hipMemcpyDeviceToDevice));
    const uint64_t *sorted = radix_sort_async(keys, tmp, n_keys, 0, kCoordBits + bits_for(std::max<uint64_t>(2, n_seqs)), hist, stream);
    HIP_TRY(hipMemsetAsync(first + blocks, 0, 4, stream));
    hipLaunchKernelGGL(k_tr_heads, dim3(blocks), dim3(256), 0, stream, sorted, n_keys, first);
    launch_scan(first, blocks + 1ull, stream);
    HIP_TRY(hipGetLastError());
    uint32_t n_bp = 0;
    HIP_TRY(hipMemcpy(&n_bp, first + blocks, 4, hipMemcpyDeviceToHost));
    a->n_bp = n_bp;
    HIP_TRY(hipMalloc(&a->bp.p, 8ull * n_bp));
    uint64_t *bp = static_cast<uint64_t *>(a->bp.p);
    hipLaunchKernelGGL(k_tr_unique, dim3(blocks), dim3(256), 0, stream, sorted, n_keys, first, bp);
    hipLaunchKernelGGL(k_tr_seq_first, dim3((n_seqs + 256) / 256), dim3(256), 0, stream, bp, n_bp, n_seqs,
                       static_cast<uint32_t *>(a->seq_first.p));
    HIP_TRY(hipGetLastError());
    // -- cover lists: count, scan, fill
    const uint32_t iv_blocks = (m + 255) / 256, bp_blocks = (n_bp + 255) / 256;
    DevBuf cnt, cursor, list, genes;
    HIP_TRY(hipMalloc(&cnt.p, 4 * scan_words(n_bp + 1ull)));
    HIP_TRY(hipMalloc(&cursor.p, 4ull * n_bp));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, 4ull * (n_bp + 1ull), stream));
    HIP_TRY(hipMemsetAsync(cursor.p, 0, 4ull * n_bp, stream));
    HIP_TRY(hipMemsetAsync(d_total, 0, 8, stream));
    uint32_t *d_cnt = static_cast<uint32_t *>(cnt.p);
    hipLaunchKernelGGL(k_tr_cover<false>, dim3(iv_blocks), dim3(256), 0, stream, d_lo, d_hi, d_tr, m, bp, n_bp, d_cnt, nullptr, nullptr,
                       d_total);
    HIP_TRY(hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(hipMemcpy(&total, d_total, 8, hipMemcpyDeviceToHost));
    if (total > 0xFFFFFFFFull) {
        set_error("cover lists of " + std::to_string(total) + " entries: more than 2^32 - 1");
        return ISSL_E_UNSUPPORTED;
    }
    launch_scan(d_cnt, n_bp + 1ull, stream);
    HIP_TRY(hipMalloc(&list.p, 4ull * std::max<unsigned long long>(total, 1)));
    hipLaunchKernelGGL(k_tr_cover<true>, dim3(iv_blocks), dim3(256), 0, stream, d_lo, d_hi, d_tr, m, bp, n_bp,
                       static_cast<uint32_t *>(cursor.p), d_cnt, static_cast<uint32_t *>(list.p), nullptr);
    HIP_TRY(hipGetLastError());
    // -- answers
    const size_t n_tr = a->t.tr_gene.size(), n_genes = a->t.gene_count.size();
    HIP_TRY(hipMalloc(&genes.p, 4ull * (n_tr + n_genes + 1)));
    uint32_t *d_tr_gene = static_cast<uint32_t *>(genes.p), *d_gene_count = d_tr_gene + n_tr;
    HIP_TRY(hipMemcpy(d_tr_gene, a->t.tr_gene.data(), 4ull * n_tr, hipMemcpyHostToDevice));
    if (n_genes) HIP_TRY(hipMemcpy(d_gene_count, a->t.gene_count.data(), 4ull * n_genes, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&a->answers.p, 16ull * n_bp));
    hipLaunchKernelGGL(k_tr_answers, dim3(bp_blocks), dim3(256), 0, stream, d_cnt, static_cast<const uint32_t *>(list.p), n_bp, d_tr_gene,
                       d_gene_count, static_cast<uint4 *>(a->answers.p));
    HIP_TRY(hipGetLastError());
    // the segments between neighbouring breakpoints of a sequence
    std::vector<uint32_t> sf(n_seqs + 1);
    HIP_TRY(hipMemcpy(sf.data(), a->seq_first.p, 4ull * (n_seqs + 1), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < n_seqs; ++s)
        if (sf[s + 1] > sf[s]) a->n_segments += sf[s + 1] - sf[s] - 1;
    HIP_TRY(hipDeviceSynchronize()); // the lists are released on return
    return ISSL_OK;
}

int open_annotation(const char *gff, size_t len, int device, issl_annotation **out)
{
    std::unique_ptr<issl_annotation> a(new issl_annotation());
    const char *timing = std::getenv("ISSL_ANNOTATION_TIMING");
    const bool timed = timing && timing[0] == '1';
    const double t0 = now_ms();
    if (int rc = parse_annotation(gff, len, a->t)) return rc;
    const double t1 = now_ms();
    AnnotationIntervals iv;
    if (int rc = annotation_intervals(a->t, iv)) return rc;
    const double t2 = now_ms();
    if (int rc = select_device(device, "the extraction")) return rc;
    a->device = device;
    a->n_exons = a->t.exons.size();
    std::vector<AnnotationExon>().swap(a->t.exons);
    for (size_t s = 0; s < a->t.seqs.size(); ++s) a->seq_index.emplace(a->t.seqs[s], static_cast<uint32_t>(s));
    const double t3 = now_ms();
    if (int rc = build_device(a.get(), iv)) return rc; // ends in a synchronise
    if (timed)
        std::fprintf(stderr, "[issl annotation] parse %.3f ms intervals %.3f ms device build %.3f ms | %zu intervals %llu breakpoints\n", t1 - t0,
                     t2 - t1, now_ms() - t3, iv.tr.size(), static_cast<unsigned long long>(a->n_bp));
    *out = a.release();
    return ISSL_OK;
}

int hits_device(issl_annotation *a, const uint32_t *d_seq, const int64_t *d_start, size_t n, issl_transcript_hits *d_out, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(a->device));
    if (n == 0) return ISSL_OK;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) {
        set_error("more than 2^39 rows in one call");
        return ISSL_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_tr_hits, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, stream, view_of(a), d_seq,
                       reinterpret_cast<const long long *>(d_start), static_cast<uint64_t>(n), reinterpret_cast<uint4 *>(d_out));
    HIP_TRY(hipGetLastError());
    return ISSL_OK;
}

int hits_host(issl_annotation *a, const uint32_t *seq, const int64_t *start, size_t n, issl_transcript_hits *out)
{
    HIP_TRY(hipSetDevice(a->device));
    if (n == 0) return ISSL_OK;
    DevBuf d_seq, d_start, d_out;
    HIP_TRY(hipMalloc(&d_seq.p, 4 * n));
    HIP_TRY(hipMalloc(&d_start.p, 8 * n));
    HIP_TRY(hipMalloc(&d_out.p, 16 * n));
    HIP_TRY(hipMemcpy(d_seq.p, seq, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_start.p, start, 8 * n, hipMemcpyHostToDevice));
    if (int rc = hits_device(a, static_cast<const uint32_t *>(d_seq.p), static_cast<const int64_t *>(d_start.p), n,
                             static_cast<issl_transcript_hits *>(d_out.p), nullptr))
        return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, 16 * n, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

int hits_occurrences_device(issl_annotation *a, const issl_genome *g, const issl_occurrence *d_rows, size_t n, issl_transcript_hits *d_out,
                            hipStream_t stream)
{
    HIP_TRY(hipSetDevice(a->device));
    if (n == 0) return ISSL_OK;
    if (g->device != a->device) {
        set_error("the genome and the annotation live on different devices");
        return ISSL_E_ARG;
    }
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) {
        set_error("more than 2^39 rows in one call");
        return ISSL_E_UNSUPPORTED;
    }
    DevBuf d_rec_seq;
    if (int rc = record_sequences(a, g, d_rec_seq)) return rc;
    const size_t n_records = g->records.size();
    hipLaunchKernelGGL(k_tr_hits_rows, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, stream, view_of(a),
                       reinterpret_cast<const ulonglong2 *>(d_rows), static_cast<uint64_t>(n), static_cast<const uint32_t *>(d_rec_seq.p),
                       static_cast<uint32_t>(n_records), reinterpret_cast<uint4 *>(d_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream)); // the table is released on return
    return ISSL_OK;
}

} // namespace

int record_sequences(const issl_annotation *a, const issl_genome *g, DevBuf &d_rec_seq)
{
    const size_t n_records = g->records.size();
    std::vector<uint32_t> rec_seq(n_records + 1, kNone);
    auto lookup = [&](const std::string &name) {
        const auto it = a->seq_index.find(name);
        return it == a->seq_index.end() ? kNone : it->second;
    };
    static const char blanks[] = " \t\n\v\f\r";
    for (size_t r = 0; r < n_records; ++r) {
        const std::string &name = g->records[r].name;
        const size_t b = name.find_first_not_of(blanks);
        if (b == std::string::npos) rec_seq[r] = lookup(std::string());
        else rec_seq[r] = lookup(name.substr(b, name.find_first_of(blanks, b) - b));
    }
    rec_seq[n_records] = lookup("*");
    HIP_TRY(hipMalloc(&d_rec_seq.p, 4 * rec_seq.size()));
    HIP_TRY(hipMemcpy(d_rec_seq.p, rec_seq.data(), 4 * rec_seq.size(), hipMemcpyHostToDevice)); // rec_seq ends with the call
    return ISSL_OK;
}

} // namespace issl

extern "C" {

int issl_annotation_open(const char *gff, size_t len, int device, issl_annotation **out)
{
    if (out) *out = nullptr;
    if (!out || (!gff && len)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::open_annotation(gff ? gff : "", len, device, out); });
}

int issl_annotation_open_file(const char *path, int device, issl_annotation **out)
{
    if (out) *out = nullptr;
    if (!out || !path) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        std::vector<char> text;
        if (int rc = issl::read_whole_file(path, text, "annotation ")) return rc;
        return issl::open_annotation(text.empty() ? "" : text.data(), text.size(), device, out);
    });
}

int issl_annotation_info(const issl_annotation *a, uint64_t *n_seqs, uint64_t *n_transcripts, uint64_t *n_genes, uint64_t *n_exons,
                         uint64_t *n_segments)
{
    if (!a || !n_seqs || !n_transcripts || !n_genes || !n_exons || !n_segments) return issl::fail(ISSL_E_ARG, "null argument");
    *n_seqs = a->t.seqs.size();
    *n_transcripts = a->t.tr_seq.size();
    *n_genes = a->t.gene_count.size();
    *n_exons = a->n_exons;
    *n_segments = a->n_segments;
    return ISSL_OK;
}

int issl_annotation_seq(const issl_annotation *a, uint64_t k, const char **name, size_t *name_len)
{
    if (!a || !name || !name_len) return issl::fail(ISSL_E_ARG, "null argument");
    if (k >= a->t.seqs.size()) {
        issl::set_error("sequence out of range");
        return ISSL_E_ARG;
    }
    *name = a->t.seqs[k].data();
    *name_len = a->t.seqs[k].size();
    return ISSL_OK;
}

int issl_annotation_lookup(const issl_annotation *a, const char *name, size_t name_len, uint32_t *seq)
{
    if (!a || !seq || (!name && name_len)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        const auto it = a->seq_index.find(std::string(name ? name : "", name_len));
        *seq = it == a->seq_index.end() ? 0xFFFFFFFFu : it->second;
        return static_cast<int>(ISSL_OK);
    });
}

int issl_annotation_hits(issl_annotation *a, const uint32_t *seq, const int64_t *start, size_t n, issl_transcript_hits *out)
{
    if (!a || (n && (!seq || !start || !out))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::hits_host(a, seq, start, n, out); });
}

int issl_annotation_hits_device(issl_annotation *a, const uint32_t *d_seq, const int64_t *d_start, size_t n, issl_transcript_hits *d_out,
                                void *stream)
{
    if (!a || (n && (!d_seq || !d_start || !d_out))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::hits_device(a, d_seq, d_start, n, d_out, static_cast<hipStream_t>(stream)); });
}

int issl_annotation_hits_occurrences_device(issl_annotation *a, const issl_genome *g, const issl_occurrence *d_rows, size_t n,
                                            issl_transcript_hits *d_out, void *stream)
{
    if (!a || !g || (n && (!d_rows || !d_out))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::hits_occurrences_device(a, g, d_rows, n, d_out, static_cast<hipStream_t>(stream)); });
}

int issl_annotation_close(issl_annotation *a)
{
    if (!a) return ISSL_OK;
    if (a->device >= 0) (void)hipSetDevice(a->device);
    delete a;
    return ISSL_OK;
}

} // extern "C"
