// Off-target landings (issl_offtarget_landings*, include/issl_hip.h): the off-target records of a batch of guides, the
// places of their sites in a resident genome and the transcript answer at every place, joined on the device.
//
// One batch of guides, everything on one stream:
//   records   the scoring pipeline's record list (issl_pipeline.cpp: records_device / records_host) stays in device
//             memory, 40 bytes per off-target, with the per-guide record offsets of the grouping pass
//   scan      locate's, unchanged (issl_locate.hip: locate_prepare): the query is the `site` field of the records, read
//             with a stride of five words; a piece is 2^22 records.  It leaves the sorted hit words, every record's rank
//             among the piece's distinct sites, every rank's run of words and the records' landing offsets
//   offsets   k_landing_offsets: a guide's first landing is the landing offset of its first record -- a gather
//   join      k_landing_join in k_locate_finish's place: one thread per landing finds its record by a search in the
//             piece's offsets (records without a landing share their offset with the next one and are passed over),
//             its word, the genome record and the position as k_locate_finish does, the annotation's sequence of that
//             record in the record -> sequence table, the answer with answer_at, and writes one 64-byte row.  No array
//             of issl_location exists in between
//   profile   k_landing_profile in the join's place: a guide's records and landings are contiguous ranges of the piece.
//             Per record the landing count goes into located[dist] or, when it is 0, one into absent[dist]; per landing
//             -- only with an annotation -- the answer is looked up as the join does and counted into in_exon[dist].
//             A thread takes a guide: ranges below 64 items are walked by the lane, of up to 4096 by its wave (shuffle
//             reduction), longer ones are listed and walked by a workgroup each (k_landing_profile_long: shuffles, then
//             LDS partials).  Integer sums in registers, no atomic per landing: the result does not depend on order.
//             A guide whose records straddle two pieces of the scan is added to by both, one after the other
// The host waits where locate waits: for the hit words and the total of every piece (locate_prepare), and for the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_annotation_device.hpp"
#include "issl_index.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"
#include "issl_genome.hpp"

namespace issl {
namespace {

static_assert(sizeof(issl_landing) == 64 && sizeof(issl_landing_profile) == 144 && sizeof(issl_offtarget) == 40,
              "landing structs: include/issl_hip.h");
constexpr uint32_t kRecWords = sizeof(issl_offtarget) / 8; // a record as 8-byte words: site | mit | cfd | guide, id | occ, dist, slice
constexpr uint32_t kWaveSpan = 64;    // a guide with this many records or landings or more is walked by its wave
constexpr uint32_t kGroupSpan = 4096; // ... and one with more than this many by a workgroup
constexpr uint32_t kBins = ISSL_PROFILE_BINS;
constexpr uint32_t kLdsRecords = 4096; // record starts k_landing_join keeps in LDS (32 KiB), as k_locate_finish does

// What the kernels read of one piece of the scan.  Record i of the piece is record rec_base + i of the batch.
struct PieceView {
    const uint64_t *words;            // sorted hit words
    const uint32_t *offs, *qrank, *rstart;
    uint32_t n, total;                // records and landings of the piece
    const uint64_t *recs;             // the piece's first record
    const uint32_t *rec_off;          // n_guides + 1 record offsets of the batch
    uint32_t rec_base, n_guides, guide_base;
    const uint64_t *starts;           // the genome's record starts
    uint32_t n_records, pos_bits;
    const uint32_t *rec_seq;          // record -> sequence of the annotation; NULL without one
    View ann;
};

__device__ __forceinline__ uint32_t dist_of(const PieceView &p, uint32_t i)
{
    return static_cast<uint32_t>(p.recs[static_cast<uint64_t>(i) * kRecWords + 4] >> 32) & 0xFFFFu;
}

// ---- offsets -------------------------------------------------------------------------------------------------------

// out[i] = base + the landing offset of guide i's first record, for every boundary i in 0..n_guides whose record lies
// in this piece (the boundary behind the piece's last record belongs to it when `last`).
__global__ __launch_bounds__(256) void k_landing_offsets(PieceView p, uint64_t base, bool last, uint64_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > p.n_guides) return;
    const uint32_t r = p.rec_off[i];
    if (r < p.rec_base || r - p.rec_base > p.n || (r - p.rec_base == p.n && !last)) return;
    out[i] = base + p.offs[r - p.rec_base];
}

// ---- join ----------------------------------------------------------------------------------------------------------

// Landing j of the piece: its record as k_locate_finish finds a location's query, its word, genome record and position
// as k_locate_finish computes them.  The 64-byte rows of a workgroup leave through LDS as one run of 16-byte words, so
// that every store instruction of a wave covers 1 KiB of consecutive bytes (k_report_emit's way out).
template <bool kLds>
__global__ __launch_bounds__(256) void k_landing_join(PieceView p, uint4 *__restrict__ out)
{
    __shared__ uint64_t tab[kLds ? kLdsRecords : 1];
    __shared__ uint4 stage[256 * 4];
    if (kLds) {
        for (uint32_t r = threadIdx.x; r < p.n_records; r += 256) tab[r] = p.starts[r];
        __syncthreads();
    }
    const uint32_t first = blockIdx.x * 256, j = first + threadIdx.x;
    if (j < p.total) {
        const uint32_t qi = last_not_above(p.offs, p.n, j);
        const uint64_t w = p.words[p.rstart[p.qrank[qi]] + (j - p.offs[qi])];
        const uint64_t tpos = (w >> 1) & ((1ull << p.pos_bits) - 1);
        const uint32_t rec = kLds ? last_not_above(tab, p.n_records, tpos) : last_not_above(p.starts, p.n_records, tpos);
        const uint64_t pos = tpos - (kLds ? tab[rec] : p.starts[rec]);
        const uint64_t *__restrict__ r = p.recs + static_cast<uint64_t>(qi) * kRecWords;
        const uint64_t site = r[0], gi = r[3], od = r[4]; // guide | id << 32; occ | dist << 32 | slice << 48
        const uint32_t guide = static_cast<uint32_t>(gi);
        const uint32_t rank = p.rec_base + qi - p.rec_off[guide - p.guide_base];
        uint4 *row = stage + 4u * threadIdx.x;
        row[0] = make_uint4(static_cast<uint32_t>(site), static_cast<uint32_t>(site >> 32), static_cast<uint32_t>(pos),
                            static_cast<uint32_t>(pos >> 32));
        row[1] = make_uint4(rec, static_cast<uint32_t>(w & 1ull), guide, rank);
        row[2] = make_uint4(static_cast<uint32_t>(gi >> 32), static_cast<uint32_t>(od), static_cast<uint32_t>(od >> 32), 0u);
        row[3] = p.rec_seq ? answer_at(p.ann, p.rec_seq[rec], static_cast<long long>(pos + 1)) : make_uint4(0u, 0u, 1u, kNone);
    }
    __syncthreads();
    const uint32_t have = (p.total - first < 256u ? p.total - first : 256u) * 4u;
    uint4 *dst = out + 4ull * first;
    for (uint32_t k = threadIdx.x; k < have; k += 256) dst[k] = stage[k];
}

// ---- profile -------------------------------------------------------------------------------------------------------

struct Bins {
    uint64_t located[kBins] = {}, in_exon[kBins] = {};
    uint32_t absent[kBins] = {};
    __device__ __forceinline__ void record(uint32_t dist, uint32_t landings)
    {
#pragma unroll
        for (uint32_t d = 0; d < kBins; ++d) {
            located[d] += dist == d ? landings : 0u;
            absent[d] += dist == d && landings == 0u ? 1u : 0u;
        }
    }
    __device__ __forceinline__ void exon(uint32_t dist)
    {
#pragma unroll
        for (uint32_t d = 0; d < kBins; ++d) in_exon[d] += dist == d ? 1u : 0u;
    }
};

__device__ __forceinline__ uint32_t wave_sum32(uint32_t x)
{
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(x), d, 64), hi = __shfl_xor(static_cast<uint32_t>(x >> 32), d, 64);
        x += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return x;
}

// The part of guide g's records that lies in the piece, [a, b) in the piece's numbering (a == b: none), and its landings.
struct Range {
    uint32_t a = 0, b = 0, la = 0, lb = 0;
    __device__ __forceinline__ uint32_t work() const { return b - a > lb - la ? b - a : lb - la; } // the longer of the two walks
};
__device__ __forceinline__ Range range_of(const PieceView &p, uint32_t g)
{
    Range r;
    const uint32_t ra = p.rec_off[g], rb = p.rec_off[g + 1];
    const uint32_t lo = ra > p.rec_base ? ra - p.rec_base : 0u;
    const uint32_t hi = rb > p.rec_base ? (rb - p.rec_base < p.n ? rb - p.rec_base : p.n) : 0u;
    if (lo < hi) {
        r.a = lo;
        r.b = hi;
        r.la = p.offs[lo];
        r.lb = p.offs[hi];
    }
    return r;
}

// Records first + k * step < r.b and, with an annotation, landings r.la + first + k * step < r.lb into `bins`.
__device__ __forceinline__ void walk(const PieceView &p, const Range &r, uint32_t first, uint32_t step, Bins &bins)
{
    for (uint32_t i = r.a + first; i < r.b; i += step) bins.record(dist_of(p, i), p.offs[i + 1] - p.offs[i]);
    if (!p.rec_seq) return;
    for (uint32_t j = r.la + first; j < r.lb; j += step) {
        const uint32_t qi = r.a + last_not_above(p.offs + r.a, r.b - r.a, j);
        const uint64_t w = p.words[p.rstart[p.qrank[qi]] + (j - p.offs[qi])];
        const uint64_t tpos = (w >> 1) & ((1ull << p.pos_bits) - 1);
        const uint32_t rec = last_not_above(p.starts, p.n_records, tpos);
        const uint4 hits = answer_at(p.ann, p.rec_seq[rec], static_cast<long long>(tpos - p.starts[rec] + 1));
        if (hits.x) bins.exon(dist_of(p, qi));
    }
}

// out[g] += bins.  A guide is added to by one thread of one launch at a time.
__device__ __forceinline__ void add_to(issl_landing_profile *__restrict__ out, const Bins &bins)
{
#pragma unroll
    for (uint32_t d = 0; d < kBins; ++d) {
        if (bins.located[d]) out->located[d] += bins.located[d];
        if (bins.in_exon[d]) out->in_exon[d] += bins.in_exon[d];
        if (bins.absent[d]) out->absent[d] += bins.absent[d];
    }
}

// One thread per guide.  n_long / long_list: the guides left to k_landing_profile_long (their order does not matter:
// every one of them is reduced by itself).
__global__ __launch_bounds__(256) void k_landing_profile(PieceView p, issl_landing_profile *__restrict__ out, uint32_t *__restrict__ n_long,
                                                         uint32_t *__restrict__ long_list)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    const Range r = g < p.n_guides ? range_of(p, g) : Range();
    const uint32_t work = r.work();
    Bins mine;
    if (work < kWaveSpan) walk(p, r, 0, 1, mine);
    for (uint64_t wide = __ballot(work >= kWaveSpan && work <= kGroupSpan); wide; wide &= wide - 1) {
        const int src = __builtin_ctzll(wide);
        Range wr;
        wr.a = __shfl(r.a, src, 64);
        wr.b = __shfl(r.b, src, 64);
        wr.la = __shfl(r.la, src, 64);
        wr.lb = __shfl(r.lb, src, 64);
        Bins part;
        walk(p, wr, lane, 64, part);
#pragma unroll
        for (uint32_t d = 0; d < kBins; ++d) {
            const uint64_t l = wave_sum64(part.located[d]), e = wave_sum64(part.in_exon[d]);
            const uint32_t a = wave_sum32(part.absent[d]);
            if (static_cast<int>(lane) == src) {
                mine.located[d] = l;
                mine.in_exon[d] = e;
                mine.absent[d] = a;
            }
        }
    }
    if (work > kGroupSpan) long_list[atomicAdd(n_long, 1u)] = g;
    else if (work) add_to(out + g, mine);
}

// One workgroup per listed guide.
__global__ __launch_bounds__(256) void k_landing_profile_long(PieceView p, issl_landing_profile *__restrict__ out,
                                                              const uint32_t *__restrict__ n_long, const uint32_t *__restrict__ long_list)
{
    __shared__ uint64_t part_located[4][kBins], part_exon[4][kBins];
    __shared__ uint32_t part_absent[4][kBins];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = *n_long;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t g = long_list[k];
        const Range r = range_of(p, g);
        Bins part;
        walk(p, r, threadIdx.x, 256, part);
#pragma unroll
        for (uint32_t d = 0; d < kBins; ++d) {
            const uint64_t l = wave_sum64(part.located[d]), e = wave_sum64(part.in_exon[d]);
            const uint32_t a = wave_sum32(part.absent[d]);
            if (lane == d) {
                part_located[wave][d] = l;
                part_exon[wave][d] = e;
                part_absent[wave][d] = a;
            }
        }
        __syncthreads();
        if (threadIdx.x < kBins) {
            const uint32_t d = threadIdx.x;
            uint64_t l = 0, e = 0;
            uint32_t a = 0;
            for (uint32_t v = 0; v < 4; ++v) {
                l += part_located[v][d];
                e += part_exon[v][d];
                a += part_absent[v][d];
            }
            out[g].located[d] += l;
            out[g].in_exon[d] += e;
            out[g].absent[d] += a;
        }
        __syncthreads();
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------

// The three handles of a call, checked, with the record -> sequence table when there is an annotation.
struct Joined {
    issl_genome *g = nullptr;
    issl_annotation *a = nullptr;
    DevBuf rec_seq;
};

int join_handles(issl_index *idx, issl_genome *g, issl_annotation *a, Joined &j)
{
    if (idx->device != g->device || (a && a->device != g->device)) {
        set_error("the index (device " + std::to_string(idx->device) + "), the genome (device " + std::to_string(g->device) + ")" +
                  (a ? " and the annotation (device " + std::to_string(a->device) + ")" : std::string()) + " live on different devices");
        return ISSL_E_ARG;
    }
    HIP_TRY(hipSetDevice(g->device));
    j.g = g;
    j.a = a;
    if (a)
        if (int rc = record_sequences(a, g, j.rec_seq)) return rc;
    return ISSL_OK;
}

int too_many(uint64_t total)
{
    set_error("more than 2^32 - 1 locations in one call (" + std::to_string(total) + "): split the query");
    return ISSL_E_UNSUPPORTED;
}

PieceView view_of_piece(const Joined &j, const RecordBatch &b, size_t at, const Piece &pc)
{
    PieceView p{};
    p.words = pc.words;
    p.offs = pc.offs;
    p.qrank = pc.qrank;
    p.rstart = pc.rstart;
    p.n = pc.n;
    p.total = static_cast<uint32_t>(pc.total);
    p.recs = reinterpret_cast<const uint64_t *>(b.d_recs + at);
    p.rec_off = b.d_rec_off;
    p.rec_base = static_cast<uint32_t>(at);
    p.n_guides = static_cast<uint32_t>(b.n_guides);
    p.guide_base = static_cast<uint32_t>(b.guide_base);
    p.starts = static_cast<const uint64_t *>(j.g->starts.p);
    p.n_records = static_cast<uint32_t>(j.g->records.size());
    p.pos_bits = j.g->pos_bits;
    p.rec_seq = static_cast<const uint32_t *>(j.rec_seq.p);
    if (j.a) p.ann = view_of(j.a);
    return p;
}

// The scan of records [at, at + cnt) of the batch.
int prepare_piece(const Joined &j, const RecordBatch &b, size_t at, size_t cnt, hipStream_t stream, Piece &pc)
{
    return locate_prepare(j.g, reinterpret_cast<const uint64_t *>(b.d_recs + at), kRecWords, cnt, 0, nullptr, stream, pc);
}

void launch_join(const PieceView &p, issl_landing *d_rows, hipStream_t stream)
{
    if (p.total == 0) return;
    const dim3 grid((p.total + 255) / 256);
    if (p.n_records <= kLdsRecords)
        hipLaunchKernelGGL(k_landing_join<true>, grid, dim3(256), 0, stream, p, reinterpret_cast<uint4 *>(d_rows));
    else
        hipLaunchKernelGGL(k_landing_join<false>, grid, dim3(256), 0, stream, p, reinterpret_cast<uint4 *>(d_rows));
}

// The landings of one batch of records.  d_offsets: the n_guides + 1 landing offsets of the batch, counted from `base`.
// d_rows: where the batch's first row goes, when `room` rows fit there; with `own` the rows of a single piece go to a
// buffer of the call instead (the host entry: *own_rows says that they are there).  *total: the batch's landings.
// Several pieces of the scan are counted first and listed by a second round.
int land_batch(const Joined &j, const RecordBatch &b, uint64_t base, uint64_t *d_offsets, issl_landing *d_rows, uint64_t room,
               CallBuffer *own, bool *own_rows, hipStream_t stream, uint64_t *total)
{
    *total = 0;
    if (own_rows) *own_rows = false;
    if (nothing_to_find(j.g, b.n_recs)) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8 * (b.n_guides + 1), stream));
        if (base) { // (a later batch of a host call: every offset is the running total)
            std::vector<uint64_t> fill(b.n_guides + 1, base);
            HIP_TRY(hipMemcpyAsync(d_offsets, fill.data(), 8 * fill.size(), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    const size_t n = b.n_recs;
    const bool one = n <= kPieceSites;
    const uint32_t offset_blocks = static_cast<uint32_t>(b.n_guides / 256 + 1);
    std::vector<uint64_t> bases;
    uint64_t sum = 0;
    for (size_t at = 0; at < n; at += kPieceSites) {
        const size_t cnt = std::min(kPieceSites, n - at);
        Piece pc;
        if (int rc = prepare_piece(j, b, at, cnt, stream, pc)) return rc;
        const PieceView p = view_of_piece(j, b, at, pc);
        hipLaunchKernelGGL(k_landing_offsets, dim3(offset_blocks), dim3(256), 0, stream, p, base + sum, at + cnt == n, d_offsets);
        bases.push_back(sum);
        sum += pc.total;
        if (base + sum > 0xFFFFFFFFull) return too_many(base + sum);
        if (one && sum <= room && sum) {
            if (own) {
                if (int rc = own->reserve(sizeof(issl_landing) * sum)) return rc;
                launch_join(p, static_cast<issl_landing *>(own->p), stream);
                *own_rows = true;
            } else if (d_rows) {
                launch_join(p, d_rows, stream);
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream)); // the piece's memory is released
    }
    *total = sum;
    if (one || own || !d_rows || sum > room) return ISSL_OK;
    for (size_t at = 0, k = 0; at < n; at += kPieceSites, ++k) {
        const size_t cnt = std::min(kPieceSites, n - at);
        Piece pc;
        if (int rc = prepare_piece(j, b, at, cnt, stream, pc)) return rc;
        launch_join(view_of_piece(j, b, at, pc), d_rows + bases[k], stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return ISSL_OK;
}

// The rows of one batch of records into d_rows, piece by piece, whatever the number of pieces (the listing round of a
// host call: the counting round has shown that they fit).
int list_batch(const Joined &j, const RecordBatch &b, CallBuffer &rows, issl_landing *out, uint64_t *total)
{
    *total = 0;
    if (nothing_to_find(j.g, b.n_recs)) return ISSL_OK;
    for (size_t at = 0; at < b.n_recs; at += kPieceSites) {
        const size_t cnt = std::min<size_t>(kPieceSites, b.n_recs - at);
        Piece pc;
        if (int rc = prepare_piece(j, b, at, cnt, nullptr, pc)) return rc;
        if (pc.total) {
            if (int rc = rows.reserve(sizeof(issl_landing) * pc.total)) return rc;
            launch_join(view_of_piece(j, b, at, pc), static_cast<issl_landing *>(rows.p), nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(out + *total, rows.p, sizeof(issl_landing) * pc.total, hipMemcpyDeviceToHost));
        }
        *total += pc.total;
    }
    return ISSL_OK;
}

int landings_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n, int max_dist,
                    uint64_t *d_offsets, issl_landing *d_out, size_t cap, size_t *n_total, hipStream_t stream)
{
    *n_total = 0;
    Joined j;
    if (int rc = join_handles(idx, g, a, j)) return rc;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    CallBuffer recs;
    RecordBatch batch;
    if (int rc = records_device(idx, d_guides, n, max_dist, recs, batch, stream)) return rc;
    uint64_t total = 0;
    if (int rc = land_batch(j, batch, 0, d_offsets, d_out, d_out ? cap : 0, nullptr, nullptr, stream, &total)) return rc;
    *n_total = total;
    return ISSL_OK;
}

int landings_host(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *guides, size_t n, int max_dist,
                  uint64_t *offsets, issl_landing *out, size_t cap, size_t *n_total)
{
    *n_total = 0;
    offsets[0] = 0;
    Joined j;
    if (int rc = join_handles(idx, g, a, j)) return rc;
    if (n == 0) return ISSL_OK;
    CallBuffer recs, rows, d_offs;
    // Counting round; a call of one piece of guides and one piece of the scan is listed from what that round left.
    uint64_t run = 0;
    bool listed = false;
    int rc = records_host(idx, guides, n, max_dist, recs, [&](const RecordBatch &b) -> int {
        if (int prc = d_offs.reserve(8 * (b.n_guides + 1))) return prc;
        uint64_t total = 0;
        bool have = false;
        const bool whole = b.n_guides == n; // (known with the first piece: it is the only one)
        if (int prc = land_batch(j, b, run, static_cast<uint64_t *>(d_offs.p), nullptr, whole && out ? cap : 0, &rows, &have, nullptr, &total))
            return prc;
        HIP_TRY(hipMemcpy(offsets + b.guide_base, d_offs.p, 8 * (b.n_guides + 1), hipMemcpyDeviceToHost));
        if (have) {
            HIP_TRY(hipMemcpy(out, rows.p, sizeof(issl_landing) * total, hipMemcpyDeviceToHost));
            listed = true;
        }
        run += total;
        return ISSL_OK;
    });
    if (rc) return rc;
    *n_total = run;
    if (listed || !out || run > cap || run == 0) return ISSL_OK;
    // Listing round: the rows of every piece behind those of the pieces before it.
    uint64_t at_row = 0;
    return records_host(idx, guides, n, max_dist, recs, [&](const RecordBatch &b) -> int {
        uint64_t total = 0;
        if (int prc = list_batch(j, b, rows, out + at_row, &total)) return prc;
        at_row += total;
        return ISSL_OK;
    });
}

// The profiles of one batch of records, added to d_out (zeroed by the caller).
int profile_batch(const Joined &j, const RecordBatch &b, issl_landing_profile *d_out, CallBuffer &lists, hipStream_t stream)
{
    if (b.n_recs == 0) return ISSL_OK;
    if (int rc = lists.reserve(4 * (b.n_guides + 1))) return rc;
    uint32_t *n_long = static_cast<uint32_t *>(lists.p), *long_list = n_long + 1;
    const uint32_t blocks = static_cast<uint32_t>((b.n_guides + 255) / 256);
    if (nothing_to_find(j.g, b.n_recs)) { // a genome without a possible match: every record is absent
        DevBuf zeros;
        HIP_TRY(hipMalloc(&zeros.p, 4 * (size_t(b.n_recs) + 1)));
        HIP_TRY(hipMemsetAsync(zeros.p, 0, 4 * (size_t(b.n_recs) + 1), stream));
        HIP_TRY(hipMemsetAsync(n_long, 0, 4, stream));
        Piece none;
        none.n = b.n_recs;
        none.offs = static_cast<uint32_t *>(zeros.p);
        PieceView p = view_of_piece(j, b, 0, none);
        p.rec_seq = nullptr; // (no landing to ask about)
        hipLaunchKernelGGL(k_landing_profile, dim3(blocks), dim3(256), 0, stream, p, d_out, n_long, long_list);
        hipLaunchKernelGGL(k_landing_profile_long, dim3(1024), dim3(256), 0, stream, p, d_out, n_long, long_list);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    for (size_t at = 0; at < b.n_recs; at += kPieceSites) {
        const size_t cnt = std::min<size_t>(kPieceSites, b.n_recs - at);
        Piece pc;
        if (int rc = prepare_piece(j, b, at, cnt, stream, pc)) return rc;
        const PieceView p = view_of_piece(j, b, at, pc);
        HIP_TRY(hipMemsetAsync(n_long, 0, 4, stream));
        hipLaunchKernelGGL(k_landing_profile, dim3(blocks), dim3(256), 0, stream, p, d_out, n_long, long_list);
        hipLaunchKernelGGL(k_landing_profile_long, dim3(1024), dim3(256), 0, stream, p, d_out, n_long, long_list);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream)); // the piece's memory is released
    }
    return ISSL_OK;
}

int landing_profile_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n, int max_dist,
                           issl_landing_profile *d_out, hipStream_t stream)
{
    Joined j;
    if (int rc = join_handles(idx, g, a, j)) return rc;
    if (n == 0) return ISSL_OK;
    CallBuffer recs, lists;
    RecordBatch batch;
    if (int rc = records_device(idx, d_guides, n, max_dist, recs, batch, stream)) return rc;
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(issl_landing_profile) * n, stream));
    if (int rc = profile_batch(j, batch, d_out, lists, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return ISSL_OK;
}

int landing_profile_host(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *guides, size_t n, int max_dist,
                         issl_landing_profile *out)
{
    Joined j;
    if (int rc = join_handles(idx, g, a, j)) return rc;
    if (n == 0) return ISSL_OK;
    CallBuffer recs, lists, prof;
    return records_host(idx, guides, n, max_dist, recs, [&](const RecordBatch &b) -> int {
        const size_t bytes = sizeof(issl_landing_profile) * b.n_guides;
        if (int rc = prof.reserve(bytes)) return rc;
        HIP_TRY(hipMemsetAsync(prof.p, 0, bytes, nullptr));
        if (int rc = profile_batch(j, b, static_cast<issl_landing_profile *>(prof.p), lists, nullptr)) return rc;
        HIP_TRY(hipMemcpy(out + b.guide_base, prof.p, bytes, hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

// Arguments first (without a device), then the state of the index: the order of the off-target report.
int landing_args(const issl_index *idx, const issl_genome *g, bool pointers, int max_dist)
{
    if (!idx || !g || !pointers) return fail(ISSL_E_ARG, "null argument");
    if (max_dist < 0 || max_dist >= ISSL_PROFILE_BINS) {
        set_error("max_dist must lie in 0..6 for the off-target report");
        return ISSL_E_ARG;
    }
    if (!idx->d_image) {
        set_error("index has no device image: call issl_index_upload first");
        return ISSL_E_STATE;
    }
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_offtarget_landings(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *guides, size_t n, int max_dist,
                            uint64_t *offsets, issl_landing *out, size_t cap, size_t *n_total)
{
    if (int rc = issl::landing_args(idx, g, offsets && n_total && (!n || guides) && (!cap || out), max_dist)) return rc;
    return issl::abi_call([&] { return issl::landings_host(idx, g, a, guides, n, max_dist, offsets, out, out ? cap : 0, n_total); });
}

int issl_offtarget_landings_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n, int max_dist,
                                   uint64_t *d_offsets, issl_landing *d_out, size_t cap, size_t *n_total, void *stream)
{
    if (int rc = issl::landing_args(idx, g, d_offsets && n_total && (!n || d_guides) && (!cap || d_out), max_dist)) return rc;
    return issl::abi_call([&] {
        return issl::landings_device(idx, g, a, d_guides, n, max_dist, d_offsets, d_out, d_out ? cap : 0, n_total,
                                     static_cast<hipStream_t>(stream));
    });
}

int issl_offtarget_landing_profile(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *guides, size_t n, int max_dist,
                                   issl_landing_profile *out)
{
    if (int rc = issl::landing_args(idx, g, !n || (guides && out), max_dist)) return rc;
    return issl::abi_call([&] { return issl::landing_profile_host(idx, g, a, guides, n, max_dist, out); });
}

int issl_offtarget_landing_profile_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n,
                                          int max_dist, issl_landing_profile *d_out, void *stream)
{
    if (int rc = issl::landing_args(idx, g, !n || (d_guides && d_out), max_dist)) return rc;
    return issl::abi_call(
        [&] { return issl::landing_profile_device(idx, g, a, d_guides, n, max_dist, d_out, static_cast<hipStream_t>(stream)); });
}

} // extern "C"
