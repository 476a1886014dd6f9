// Where in the genome an off-target site lies: record, position, strand (issl_genome_*, include/issl_hip.h).
//
// A genome handle keeps the text the extraction would scan (append_records: upper-cased records, '\n' behind each) in
// device memory at 1 B per base, with the table of record starts.  A location of a site is a match of the extraction
// (match_at: forward pattern = strand 0, reverse pattern = strand 1) whose site -- the first 20 of the 23 matched
// characters, reverse-complemented for the reverse pattern (extractOfftargets.py:97-110) -- is the queried one.
//
// One call, for a piece of up to 2^22 query sites, everything on one stream:
//   query prep   signatures -> the extraction's text-order keys, radix-sorted with their query index; runs of equal keys
//                collapsed to ranks (k_query_heads, launch_scan, k_query_ranks), which also sets one bit per distinct
//                key in a bitmap over a multiplicative hash of the key (>= 32 bits per query site)
//   scan         k_locate_count / k_locate_emit on the grid of k_match_*: match_at, then the bitmap, and only on a set
//                bit the binary search in the sorted distinct keys; a true hit is one word rank | position | strand,
//                room reserved with one atomic per workgroup.  No per-site counter anywhere: 200 000 matches of one
//                site are 200 000 words, not 200 000 atomics on one address
//   order        radix sort of the words over the bits in use: rank-major, then position, then strand -- which is
//                (record, pos, strand), records being laid out in ascending order
//   counts       k_rank_bounds: every word looks at its two neighbours and the head and the tail of a run of equal rank
//                write the run's bounds (plain stores, each address written once); k_query_counts gives every query --
//                a repeated one too -- the length of its rank's run, launch_scan turns them into offsets
//   finish       k_locate_finish: one thread per location to write: its query by a search in the offsets, its word, the
//                record by a search in the start table (in LDS up to 4096 records), one 16-byte store
//                (issl_landing.hip puts its join in this place: locate_prepare and Piece are declared in issl_genome.hpp)
// The host waits three times: for the number of hit words (sizes the buffers of the sort), for the number of
// locations (the capacity rule is the host's: nothing is launched when they do not fit) and for the end.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "cli_inputs.hpp"
#include "issl_genome.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"

namespace issl {
namespace {

constexpr uint32_t kLdsRecords = 4096;              // record starts k_locate_finish keeps in LDS (32 KiB)

static_assert(sizeof(issl_location) == 16, "issl_location is 16 bytes");

// ---- the scan of the text (query prep and the probe: issl_genome.hpp) --------------------------------------------

// ctr[0]: hit words; ctr[2], ctr[3]: matches of the patterns and those of them the bitmap let through (the figures of
// the timing line).  One atomic per counter and workgroup.
__global__ __launch_bounds__(256) void k_locate_count(const uint8_t *__restrict__ s, uint64_t len, Probe q,
                                                      unsigned long long *__restrict__ ctr)
{
    __shared__ uint32_t wave_cnt[3][4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t nr = *q.n_ranks;
    uint32_t cnt = 0, matches = 0, passed = 0;
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a, b;
        const uint32_t m = match_at(s, base + k, len, a, b);
        matches += (m & 1u) + (m >> 1);
        if ((m & 1u) && probe_key(q, nr, a, passed) >= 0) ++cnt;
        if ((m & 2u) && probe_key(q, nr, b, passed) >= 0) ++cnt;
    }
    for (int d = 32; d > 0; d >>= 1) {
        cnt += __shfl_down(cnt, d, 64);
        matches += __shfl_down(matches, d, 64);
        passed += __shfl_down(passed, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_cnt[0][threadIdx.x >> 6] = cnt;
        wave_cnt[1][threadIdx.x >> 6] = matches;
        wave_cnt[2][threadIdx.x >> 6] = passed;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t t = wave_cnt[threadIdx.x][0] + wave_cnt[threadIdx.x][1] + wave_cnt[threadIdx.x][2] + wave_cnt[threadIdx.x][3];
        if (t) atomicAdd(&ctr[threadIdx.x ? threadIdx.x + 1 : 0], static_cast<unsigned long long>(t));
    }
}

// Second pass.  A thread keeps which of its 16 positions hit, on which strand, as 32 bits; after the workgroup has
// reserved its room with one atomic, only those positions are looked at again.  word = rank << (pos_bits + 1) |
// position << 1 | strand; the order inside the buffer does not matter, the words are sorted afterwards.
__global__ __launch_bounds__(256) void k_locate_emit(const uint8_t *__restrict__ s, uint64_t len, Probe q, uint32_t pos_bits,
                                                     unsigned long long *__restrict__ cursor, uint64_t *__restrict__ words,
                                                     uint64_t cap)
{
    __shared__ uint32_t wave_cnt[4];
    __shared__ unsigned long long block_base;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nr = *q.n_ranks;
    uint32_t hits = 0, unused = 0;
    static_assert(kPosPerBlock / 256 == 16, "two bits per position of a thread in one 32-bit mask");
    for (uint32_t r = 0; r < kPosPerBlock / 256; ++r) {
        uint64_t a, b;
        const uint32_t m = match_at(s, base + r * 256 + threadIdx.x, len, a, b);
        if ((m & 1u) && probe_key(q, nr, a, unused) >= 0) hits |= 1u << (2 * r);
        if ((m & 2u) && probe_key(q, nr, b, unused) >= 0) hits |= 2u << (2 * r);
    }
    const uint32_t cnt = static_cast<uint32_t>(__builtin_popcount(hits));
    uint32_t incl = cnt; // inclusive scan inside the wave
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        block_base = t ? atomicAdd(cursor, static_cast<unsigned long long>(t)) : 0ull;
    }
    __syncthreads();
    if (!hits) return;
    uint64_t at = block_base + (incl - cnt);
    for (uint32_t v = 0; v < wave; ++v) at += wave_cnt[v];
    for (uint32_t r = 0; r < kPosPerBlock / 256; ++r) {
        const uint32_t two = (hits >> (2 * r)) & 3u;
        if (!two) continue;
        const uint64_t pos = base + r * 256 + threadIdx.x;
        uint64_t a = 0, b = 0;
        (void)match_at(s, pos, len, a, b);
        if (two & 1u) {
            const int rank = probe_key(q, nr, a, unused);
            if (rank >= 0 && at < cap) words[at++] = (static_cast<uint64_t>(rank) << (pos_bits + 1)) | (pos << 1);
        }
        if (two & 2u) {
            const int rank = probe_key(q, nr, b, unused);
            if (rank >= 0 && at < cap) words[at++] = (static_cast<uint64_t>(rank) << (pos_bits + 1)) | (pos << 1) | 1ull;
        }
    }
}

// ---- counts and offsets ------------------------------------------------------------------------------------------

// Sorted words: the head of a run of equal rank writes where it starts, the tail where it ends.  rstart / rend are
// zeroed before the launch, so a rank without a hit has an empty run.
__global__ __launch_bounds__(256) void k_rank_bounds(const uint64_t *__restrict__ words, uint32_t n, uint32_t rank_shift,
                                                     uint32_t *__restrict__ rstart, uint32_t *__restrict__ rend)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t rank = words[i] >> rank_shift;
    if (i == 0 || (words[i - 1] >> rank_shift) != rank) rstart[rank] = i;
    if (i + 1 == n || (words[i + 1] >> rank_shift) != rank) rend[rank] = i + 1;
}

// cnt[q]: locations of query q (cnt[n] = 0 closes the scan); *total: their sum in 64 bits, one atomic per workgroup.
__global__ __launch_bounds__(256) void k_query_counts(const uint32_t *__restrict__ qrank, const uint32_t *__restrict__ rstart,
                                                      const uint32_t *__restrict__ rend, uint32_t n, uint32_t *__restrict__ cnt,
                                                      unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long wave_sum[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t c = 0;
    if (i < n) {
        const uint32_t r = qrank[i];
        c = rend[r] - rstart[r];
        cnt[i] = c;
    } else if (i == n) {
        cnt[i] = 0;
    }
    unsigned long long sum = c;
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (t) atomicAdd(total, t);
    }
}

__global__ __launch_bounds__(256) void k_write_offsets(const uint32_t *__restrict__ offs, uint32_t n1, uint64_t base,
                                                       uint64_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n1) out[i] = base + offs[i];
}

// ---- finish ------------------------------------------------------------------------------------------------------

// Location j of the piece (j < total = offs[n]): query = the last one whose offset is <= j (queries without a location
// share their offset with the next one and are passed over), its word the (j - offset)-th of its rank's run.
template <bool kLds>
__global__ __launch_bounds__(256) void k_locate_finish(const uint64_t *__restrict__ words, const uint32_t *__restrict__ offs, uint32_t n,
                                                       uint32_t total, const uint32_t *__restrict__ qrank,
                                                       const uint32_t *__restrict__ rstart, const uint64_t *__restrict__ starts,
                                                       uint32_t n_records, uint32_t pos_bits, ulonglong2 *__restrict__ locs)
{
    __shared__ uint64_t tab[kLds ? kLdsRecords : 1];
    if (kLds) {
        for (uint32_t r = threadIdx.x; r < n_records; r += 256) tab[r] = starts[r];
        __syncthreads();
    }
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint32_t qi = last_not_above(offs, n, j);
    const uint64_t w = words[rstart[qrank[qi]] + (j - offs[qi])];
    const uint64_t pos = (w >> 1) & ((1ull << pos_bits) - 1);
    const uint32_t rec = kLds ? last_not_above(tab, n_records, pos) : last_not_above(starts, n_records, pos);
    const uint64_t start = kLds ? tab[rec] : starts[rec];
    locs[j] = make_ulonglong2(pos - start, static_cast<uint64_t>(rec) | ((w & 1ull) << 32)); // {pos, record, strand}
}

// ---- host --------------------------------------------------------------------------------------------------------

} // namespace

// Everything of a piece but the locations: d_offsets[0..n] = base + the piece's offsets (when asked for), pc.total = its
// locations.  Declared in issl_genome.hpp: issl_landing.hip joins the same pieces with the off-target records.
int locate_prepare(const issl_genome *g, const uint64_t *d_sites, size_t site_stride, size_t n_sites, uint64_t base,
                   uint64_t *d_offsets, hipStream_t stream, Piece &pc)
{
    const uint32_t n = static_cast<uint32_t>(n_sites);
    pc.n = n;
    StageTimer clock(g->timing, stream);
    // -- buffers whose size the query fixes
    Arena &qa = pc.query;
    QueryPrep prep;
    const size_t o_wa = qa.reserve(8ull * n);
    prep.reserve(qa, n);
    const size_t o_rstart = qa.reserve(4ull * n), o_rend = qa.reserve(4ull * n), o_cnt = qa.reserve(4 * scan_words(n + 1ull));
    HIP_TRY(hipMalloc(&qa.buf.p, qa.size));
    uint32_t *rstart = qa.at<uint32_t>(o_rstart), *rend = qa.at<uint32_t>(o_rend), *cnt = qa.at<uint32_t>(o_cnt);
    HIP_TRY(hipMemsetAsync(rstart, 0, static_cast<size_t>(o_cnt - o_rstart), stream)); // rstart and rend
    // -- query prep: the sorted words are read where the sort left them
    if (int rc = prep.enqueue(qa, d_sites, qa.at<uint64_t>(o_wa), false, stream, static_cast<uint32_t>(site_stride))) return rc;
    const Probe &probe = prep.probe;
    uint32_t *qrank = prep.qrank;
    unsigned long long *ctr = prep.ctr; // 0 hit words, 1 emit cursor, 2 matches, 3 passed, 4 locations
    clock.note("prep");
    // -- count
    const uint8_t *d_seq = static_cast<const uint8_t *>(g->seq.p);
    const uint32_t blocks = static_cast<uint32_t>((g->len + kPosPerBlock - 1) / kPosPerBlock);
    hipLaunchKernelGGL(k_locate_count, dim3(blocks), dim3(256), 0, stream, d_seq, g->len, probe, ctr);
    unsigned long long seen[4] = {};
    HIP_TRY(hipMemcpyAsync(seen, ctr, sizeof seen, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("count");
    const uint64_t n_words = seen[0];
    if (n_words > 0xFFFFFFFFull) { // the radix passes count and place with 32-bit offsets (issl_radix.hpp)
        set_error("more than 2^32 - 1 locations in one call (" + std::to_string(n_words) + "): split the query");
        return ISSL_E_UNSUPPORTED;
    }
    pc.n_words = n_words;
    const uint32_t rank_shift = g->pos_bits + 1;
    if (n_words) {
        // -- emit and sort
        Arena &ha = pc.hit;
        const size_t o_ha = ha.reserve(8 * n_words), o_hb = ha.reserve(8 * n_words),
                     o_hh = ha.reserve(4 * radix_hist_words(radix_sort_blocks(n_words)));
        HIP_TRY(hipMalloc(&ha.buf.p, ha.size));
        uint64_t *ha_w = ha.at<uint64_t>(o_ha), *hb_w = ha.at<uint64_t>(o_hb);
        hipLaunchKernelGGL(k_locate_emit, dim3(blocks), dim3(256), 0, stream, d_seq, g->len, probe, g->pos_bits, ctr + 1, ha_w,
                           n_words);
        clock.note("emit");
        pc.words = radix_sort_async(ha_w, hb_w, n_words, 0, rank_shift + bits_for(n), ha.at<uint32_t>(o_hh), stream);
        clock.note("sort");
        hipLaunchKernelGGL(k_rank_bounds, dim3(static_cast<uint32_t>((n_words + 255) / 256)), dim3(256), 0, stream, pc.words,
                           static_cast<uint32_t>(n_words), rank_shift, rstart, rend);
    }
    // -- per-query counts -> offsets
    hipLaunchKernelGGL(k_query_counts, dim3(n / 256 + 1), dim3(256), 0, stream, qrank, rstart, rend, n, cnt, ctr + 4);
    launch_scan(cnt, n + 1ull, stream);
    if (d_offsets)
        hipLaunchKernelGGL(k_write_offsets, dim3(n / 256 + 1), dim3(256), 0, stream, cnt, n + 1, base, d_offsets);
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, ctr + 4, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("offsets");
    if (g->timing)
        std::fprintf(stderr, "[issl locate] %u sites:%s | matches %llu filter passed %llu hits %llu locations %llu\n", n,
                     clock.line.c_str(), seen[2], seen[3], seen[0], total);
    if (total > 0xFFFFFFFFull) { // a site named many times multiplies its run; the offsets of a piece are scanned in 32 bits
        set_error("more than 2^32 - 1 locations in one call (" + std::to_string(total) + "): split the query");
        return ISSL_E_UNSUPPORTED;
    }
    pc.total = total;
    pc.offs = cnt;
    pc.qrank = qrank;
    pc.rstart = rstart;
    return ISSL_OK;
}

// A genome without a possible match, or an empty query: offsets of zeros.
bool nothing_to_find(const issl_genome *g, size_t n) { return n == 0 || g->len < 23; }

namespace {

// The piece's locations to d_locs[0 .. pc.total).  Returns when they are written.
int locate_finish(const issl_genome *g, const Piece &pc, issl_location *d_locs, hipStream_t stream)
{
    if (pc.total == 0) return ISSL_OK;
    StageTimer clock(g->timing, stream);
    const uint32_t total = static_cast<uint32_t>(pc.total), n_records = static_cast<uint32_t>(g->records.size());
    const uint64_t *starts = static_cast<const uint64_t *>(g->starts.p);
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(d_locs);
    const dim3 grid((total + 255) / 256);
    if (n_records <= kLdsRecords)
        hipLaunchKernelGGL(k_locate_finish<true>, grid, dim3(256), 0, stream, pc.words, pc.offs, pc.n, total, pc.qrank, pc.rstart,
                           starts, n_records, g->pos_bits, out);
    else
        hipLaunchKernelGGL(k_locate_finish<false>, grid, dim3(256), 0, stream, pc.words, pc.offs, pc.n, total, pc.qrank, pc.rstart,
                           starts, n_records, g->pos_bits, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("finish");
    if (g->timing) std::fprintf(stderr, "[issl locate]%s\n", clock.line.c_str());
    return ISSL_OK;
}

int locate_device(issl_genome *g, const uint64_t *d_sites, size_t n, uint64_t *d_offsets, issl_location *d_locs, size_t cap,
                  size_t *n_total, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(g->device));
    *n_total = 0;
    if (nothing_to_find(g, n)) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8 * (n + 1), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    // Counting pass over the pieces; a single piece is finished from what that pass left, several are run once more.
    std::vector<uint64_t> bases;
    uint64_t total = 0;
    for (size_t at = 0; at < n; at += kPieceSites) {
        const size_t cnt = std::min(kPieceSites, n - at);
        Piece pc;
        bases.push_back(total);
        if (int rc = locate_prepare(g, d_sites + at, 1, cnt, total, d_offsets + at, stream, pc)) return rc;
        total += pc.total;
        if (total > 0xFFFFFFFFull) {
            set_error("more than 2^32 - 1 locations in one call (" + std::to_string(total) + "): split the query");
            return ISSL_E_UNSUPPORTED;
        }
        if (n <= kPieceSites && d_locs && total <= cap)
            if (int rc = locate_finish(g, pc, d_locs, stream)) return rc;
    }
    *n_total = total;
    if (n <= kPieceSites || !d_locs || total > cap) return ISSL_OK;
    for (size_t at = 0, k = 0; at < n; at += kPieceSites, ++k) {
        const size_t cnt = std::min(kPieceSites, n - at);
        Piece pc;
        if (int rc = locate_prepare(g, d_sites + at, 1, cnt, bases[k], d_offsets + at, stream, pc)) return rc;
        if (int rc = locate_finish(g, pc, d_locs + bases[k], stream)) return rc;
    }
    return ISSL_OK;
}

int locate_host(issl_genome *g, const uint64_t *sites, size_t n, uint64_t *offsets, issl_location *locs, size_t cap, size_t *n_total)
{
    HIP_TRY(hipSetDevice(g->device));
    *n_total = 0;
    if (nothing_to_find(g, n)) {
        std::memset(offsets, 0, 8 * (n + 1));
        return ISSL_OK;
    }
    // At most one piece of sites, offsets and locations is on the device at a time.
    const size_t piece = std::min(kPieceSites, n);
    DevBuf d_sites, d_offs, d_locs;
    HIP_TRY(hipMalloc(&d_sites.p, 8 * piece));
    HIP_TRY(hipMalloc(&d_offs.p, 8 * (piece + 1)));
    uint64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t base = 0;
        for (size_t at = 0; at < n; at += kPieceSites) {
            const size_t cnt = std::min(kPieceSites, n - at);
            Piece pc;
            HIP_TRY(hipMemcpy(d_sites.p, sites + at, 8 * cnt, hipMemcpyHostToDevice));
            if (int rc = locate_prepare(g, static_cast<const uint64_t *>(d_sites.p), 1, cnt, base, static_cast<uint64_t *>(d_offs.p),
                                        nullptr, pc))
                return rc;
            if (pass == 0) HIP_TRY(hipMemcpy(offsets + at, d_offs.p, 8 * (cnt + 1), hipMemcpyDeviceToHost));
            // pass 1 (several pieces, everything fits), or the one piece of a call at once
            if ((pass == 1 || (n <= kPieceSites && locs && base + pc.total <= cap)) && pc.total) {
                d_locs.release();
                HIP_TRY(hipMalloc(&d_locs.p, 16 * pc.total));
                if (int rc = locate_finish(g, pc, static_cast<issl_location *>(d_locs.p), nullptr)) return rc;
                HIP_TRY(hipMemcpy(locs + base, d_locs.p, 16 * pc.total, hipMemcpyDeviceToHost));
            }
            base += pc.total;
            if (base > 0xFFFFFFFFull) {
                set_error("more than 2^32 - 1 locations in one call (" + std::to_string(base) + "): split the query");
                return ISSL_E_UNSUPPORTED;
            }
        }
        total = base;
        if (n <= kPieceSites || !locs || total > cap) break;
    }
    *n_total = total;
    return ISSL_OK;
}

// seq and its records -> the handle on `device`.
int open_genome(std::string &seq, std::vector<FastaRecord> &records, int device, issl_genome **out)
{
    if (int rc = select_device(device, "the extraction")) return rc;
    if (seq.size() >> 41) {
        set_error("genome text of " + std::to_string(seq.size()) + " bytes: a locate word holds positions below 2^41");
        return ISSL_E_UNSUPPORTED;
    }
    if (records.size() > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 records");
        return ISSL_E_UNSUPPORTED;
    }
    std::unique_ptr<issl_genome> g(new issl_genome());
    g->device = device;
    g->len = seq.size();
    g->pos_bits = bits_for(std::max<uint64_t>(2, g->len));
    const char *t = std::getenv("ISSL_LOCATE_TIMING");
    g->timing = t && t[0] == '1';
    std::vector<uint64_t> starts(records.size());
    for (size_t r = 0; r < records.size(); ++r) {
        starts[r] = records[r].start;
        g->n_bases += records[r].length;
    }
    if (g->len) {
        HIP_TRY(hipMalloc(&g->seq.p, g->len));
        HIP_TRY(hipMemcpy(g->seq.p, seq.data(), g->len, hipMemcpyHostToDevice));
    }
    if (!starts.empty()) {
        HIP_TRY(hipMalloc(&g->starts.p, 8 * starts.size()));
        HIP_TRY(hipMemcpy(g->starts.p, starts.data(), 8 * starts.size(), hipMemcpyHostToDevice));
    }
    g->records = std::move(records);
    *out = g.release();
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_genome_open(const char *const *files, const size_t *lens, int n_files, int device, issl_genome **out)
{
    if (out) *out = nullptr;
    if (!files || !lens || n_files <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    for (int f = 0; f < n_files; ++f)
        if (!files[f] && lens[f]) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        std::string seq;
        std::vector<issl::FastaRecord> records;
        for (int f = 0; f < n_files; ++f) issl::append_records(files[f], lens[f], n_files > 1, seq, &records);
        return issl::open_genome(seq, records, device, out);
    });
}

int issl_genome_open_files(const char *const *paths, int n_paths, int device, issl_genome **out)
{
    if (out) *out = nullptr;
    if (!paths || n_paths <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    for (int f = 0; f < n_paths; ++f)
        if (!paths[f]) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        const std::vector<std::string> inputs = expand_fasta_inputs(std::vector<std::string>(paths, paths + n_paths));
        if (inputs.empty()) {
            issl::set_error(std::string("no FASTA file in '") + paths[0] + "'");
            return ISSL_E_IO;
        }
        std::vector<const char *> ptrs;
        for (const auto &s : inputs) ptrs.push_back(s.c_str());
        std::string seq;
        std::vector<issl::FastaRecord> records;
        if (int rc = issl::read_fasta_files(ptrs.data(), static_cast<int>(ptrs.size()), seq, &records)) return rc;
        return issl::open_genome(seq, records, device, out);
    });
}

int issl_genome_info(const issl_genome *g, uint64_t *n_records, uint64_t *n_bases)
{
    if (!g || !n_records || !n_bases) return issl::fail(ISSL_E_ARG, "null argument");
    *n_records = g->records.size();
    *n_bases = g->n_bases;
    return ISSL_OK;
}

int issl_genome_record(const issl_genome *g, uint64_t r, const char **name, size_t *name_len, uint64_t *length)
{
    if (!g || !name || !name_len || !length) return issl::fail(ISSL_E_ARG, "null argument");
    if (r >= g->records.size()) {
        issl::set_error("record out of range");
        return ISSL_E_ARG;
    }
    *name = g->records[r].name.data();
    *name_len = g->records[r].name.size();
    *length = g->records[r].length;
    return ISSL_OK;
}

int issl_genome_locate(issl_genome *g, const uint64_t *sites, size_t n, uint64_t *offsets, issl_location *locs, size_t cap,
                       size_t *n_total)
{
    if (!g || (!sites && n) || !offsets || !n_total || (!locs && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::locate_host(g, sites, n, offsets, locs, cap, n_total); });
}

int issl_genome_locate_device(issl_genome *g, const uint64_t *d_sites, size_t n, uint64_t *d_offsets, issl_location *d_locs,
                              size_t cap, size_t *n_total, void *stream)
{
    if (!g || (!d_sites && n) || !d_offsets || !n_total || (!d_locs && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call(
        [&] { return issl::locate_device(g, d_sites, n, d_offsets, d_locs, cap, n_total, static_cast<hipStream_t>(stream)); });
}

int issl_genome_close(issl_genome *g)
{
    if (!g) return ISSL_OK;
    if (g->device >= 0) (void)hipSetDevice(g->device);
    delete g;
    return ISSL_OK;
}

} // extern "C"
