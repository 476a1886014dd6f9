// Variant-aware genome search: issl_genome_search with IUPAC ambiguity codes in the text read as sets of bases
// (issl_genome_search_variants*, include/issl_hip.h), and SNPs written onto a resident genome (issl_vcf_snps,
// issl_genome_apply_snps, issl_genome_apply_vcf).  The third unit of SearchDriver (issl_search_device.hpp) beside
// issl_search.hip and issl_bulge.hip, with the protocol of issl_search_core.hpp: count, emit, sort, offsets, finish, and
// the one-pass profile.  This unit's own: bit planes in place of 2-bit codes.  The tile goes to LDS as four planes (A C G
// T; plane b bit i: base b is in the set of text position i) and a validity bit per base, 32 bases per word; a window is
// four words cut out with a funnel shift; the pattern is four plane masks, and strand 1 is tested on the forward window
// with the reversed, complemented pattern, so no window is reversed in the front.  A piece's queries are expanded once
// into 16-byte records of planes (k_variant_queries), the same 16 B and the same group loads as the plain search's.  The
// comparison is four ANDs ORed together for all 32 positions, five instructions and a popcount.  The plane arithmetic is issl_variants_text.hpp's, which
// tools/variants_sanitize.cpp checks on the CPU.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_search_core.hpp"
#include "issl_variants_text.hpp"

namespace issl {
namespace {

namespace vt = variants_text;
using vt::Planes;
using vt::VariantArgs;

constexpr uint32_t kPlaneWords = kPosPerBlock / 32 + 1; // 32 bases per word; the halo of up to 31 bases is one more word
static_assert(sizeof(issl_variant_hit) == 40 && sizeof(issl_snp) == 16 && sizeof(vt::SnpPlace) == 16 && sizeof(Planes) == 16,
              "the layouts of include/issl_hip.h");

// What a checked call carries to the launches: the pattern and limits, and room for the planes of a piece's queries.
struct VariantCall {
    VariantArgs a;
    Planes *q_planes;
};

// 16 bytes of text at `at` (a multiple of 16) -> 16 bits of every plane and one bit per base that is none of the 14
// codes; what lies behind the text is such a base.
__device__ __forceinline__ void planes16(const uint8_t *__restrict__ s, uint64_t at, uint64_t len, uint32_t (&plane)[4], uint32_t &bad)
{
    plane[0] = plane[1] = plane[2] = plane[3] = 0;
    bad = 0;
    uint32_t w[4] = {0, 0, 0, 0}; // (a zero byte is no code)
    if (at + 16 <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(s + at);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        for (uint32_t i = 0; i < 16; ++i)
            if (at + i < len) w[i >> 2] |= static_cast<uint32_t>(s[at + i]) << (8 * (i & 3));
    }
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t set = vt::text_set(static_cast<uint8_t>(w[i >> 2] >> (8 * (i & 3))));
        plane[0] |= (set & 1u) << i;
        plane[1] |= (set >> 1 & 1u) << i;
        plane[2] |= (set >> 2 & 1u) << i;
        plane[3] |= (set >> 3) << i;
        bad |= (set ? 0u : 1u) << i;
    }
}

// The queries of a piece as planes: a compared position in its base's plane alone, an N position in all four.
__global__ __launch_bounds__(256) void k_variant_queries(const issl_search_query *__restrict__ q, uint32_t n, uint32_t win_mask,
                                                         Planes *__restrict__ out)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = vt::query_planes(q[k].sig, q[k].care, win_mask);
}

struct PlaneGroup { Planes q[kQueryGroup]; };

// ctr[0]: hits; ctr[1]: the cursor of k_variants<kEmit>; ctr[2]: window-strands the pattern admits; ctr[3]: windows of L
// codes with at most max_variants ambiguous positions (the figures of the timing line, kCount only).
template <int kMode>
__global__ __launch_bounds__(256) void k_variants(const uint8_t *__restrict__ s, uint64_t len, VariantArgs a,
                                                  const Planes *__restrict__ q, uint32_t n, uint32_t pos_bits,
                                                  unsigned long long *__restrict__ ctr, uint64_t *__restrict__ words, uint64_t cap,
                                                  unsigned long long *__restrict__ counts)
{
    // plane b and the validity bits as 32-bit words; a thread writes the 16-bit half of its 16 bases
    __shared__ uint32_t tile[5][kPlaneWords];
    __shared__ uint16_t queue[2 * kPosPerBlock]; // tag = position in the tile << 1 | strand
    __shared__ uint32_t q_count;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) q_count = 0;
    {
        uint32_t plane[4], bad;
        planes16(s, base + 16ull * threadIdx.x, len, plane, bad);
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) reinterpret_cast<uint16_t *>(tile[b])[threadIdx.x] = static_cast<uint16_t>(plane[b]);
        reinterpret_cast<uint16_t *>(tile[4])[threadIdx.x] = static_cast<uint16_t>(bad);
        if (threadIdx.x < 2) {
            planes16(s, base + kPosPerBlock + 16ull * threadIdx.x, len, plane, bad);
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) reinterpret_cast<uint16_t *>(tile[b])[256 + threadIdx.x] = static_cast<uint16_t>(plane[b]);
            reinterpret_cast<uint16_t *>(tile[4])[256 + threadIdx.x] = static_cast<uint16_t>(bad);
        }
    }
    __syncthreads();

    // -- the pattern on the thread's 16 windows, both strands: two bits per window
    uint32_t pass = 0, windows = 0;
    {
        const uint32_t wi = threadIdx.x >> 1, s0 = (threadIdx.x & 1u) << 4;
        uint32_t lo[5], hi[5];
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) lo[b] = tile[b][wi], hi[b] = tile[b][wi + 1];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            if (vt::funnel(lo[4], hi[4], s0 + k) & a.win_mask) continue;
            const Planes f{{vt::funnel(lo[0], hi[0], s0 + k) & a.win_mask, vt::funnel(lo[1], hi[1], s0 + k) & a.win_mask,
                            vt::funnel(lo[2], hi[2], s0 + k) & a.win_mask, vt::funnel(lo[3], hi[3], s0 + k) & a.win_mask}};
            if (static_cast<uint32_t>(__builtin_popcount(vt::ambiguous(f))) > a.max_variants) continue;
            ++windows;
            if (vt::admits(f, a.allow, a.win_mask)) pass |= 1u << (2 * k);
            if (vt::admits(f, a.allow_rc, a.win_mask)) pass |= 2u << (2 * k);
        }
    }
    // -- the survivors into the queue: a scan inside the wave, one LDS atomic per wave
    {
        const uint32_t cnt = static_cast<uint32_t>(__builtin_popcount(pass));
        uint32_t incl = cnt;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        uint32_t wave_base = 0;
        if (lane == 63 && incl) wave_base = atomicAdd(&q_count, incl);
        wave_base = __shfl(wave_base, 63, 64);
        uint32_t at = wave_base + incl - cnt;
        for (uint32_t m = pass; m; m &= m - 1) {
            const uint32_t bit = static_cast<uint32_t>(__builtin_ctz(m));
            queue[at++] = static_cast<uint16_t>(((threadIdx.x * 16 + (bit >> 1)) << 1) | (bit & 1u));
        }
    }
    __syncthreads();
    const uint32_t n_q = q_count;

    // -- every survivor against every query: a lane holds one survivor's A planes, a wave its quarter of the queries
    const QueryRange mine_q = wave_queries(n);
    unsigned long long found = 0; // kCount: the hits of this lane's survivors
    for (uint32_t j0 = 0; j0 < n_q && mine_q.lo < mine_q.hi; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool valid = j < n_q;
        uint32_t tag = 0;
        Planes t{{0, 0, 0, 0}}; // what the strand reads, cut by the pattern: nothing matches where there is no survivor
        if (valid) {
            tag = queue[j];
            const uint32_t p = tag >> 1, wi = p >> 5, sh = p & 31u;
            const Planes f{{vt::funnel(tile[0][wi], tile[0][wi + 1], sh) & a.win_mask, vt::funnel(tile[1][wi], tile[1][wi + 1], sh) & a.win_mask,
                            vt::funnel(tile[2][wi], tile[2][wi + 1], sh) & a.win_mask, vt::funnel(tile[3][wi], tile[3][wi + 1], sh) & a.win_mask}};
            t = vt::intersect((tag & 1u) ? vt::strand1(f, a.rev_shift) : f, a.allow);
        }
        const uint64_t live = __ballot(valid);
        uint32_t mine = 0; // kCount: at most 2^22 hits of this lane's survivor
        // one query against the wave's survivors; everything about the query is wave-uniform
        auto compare = [&](const Planes &one, uint32_t qi) {
            const uint32_t same = static_cast<uint32_t>(__builtin_popcount(vt::matches(t, one)));
            if (kMode == kCount) { // a lane counts its own hits; what a lane without a survivor counts is dropped below
                mine += same >= a.need ? 1u : 0u;
                return;
            }
            const uint64_t who = __ballot(same >= a.need) & live;
            if (!who) return;
            const bool hit = (who >> lane) & 1u;
            if (kMode == kEmit) emit_hits<0>(who, hit, lane, ctr, words, cap, qi, pos_bits, base, tag, 0);
            else profile_hits(who, hit, a.length - same, lane, counts, qi, a.max_dist + 1);
        };
        // kQueryGroup queries come in with one wait, the group behind the one being compared is on its way (k_search)
        uint32_t qi = mine_q.lo;
        if (mine_q.hi - mine_q.lo >= kQueryGroup) {
            PlaneGroup next = *reinterpret_cast<const PlaneGroup *>(q + qi);
            for (; qi + kQueryGroup <= mine_q.hi; qi += kQueryGroup) {
                const PlaneGroup group = next;
                if (qi + 2 * kQueryGroup <= mine_q.hi) next = *reinterpret_cast<const PlaneGroup *>(q + qi + kQueryGroup);
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) compare(group.q[u], qi + u);
            }
        }
        for (; qi < mine_q.hi; ++qi) compare(q[qi], qi);
        if (kMode == kCount && valid) found += mine;
    }
    if (kMode == kCount) {
        for (int d = 32; d > 0; d >>= 1) {
            windows += __shfl_down(windows, d, 64);
            found += __shfl_down(found, d, 64);
        }
        if (lane == 0) {
            if (found) atomicAdd(ctr, found);
            if (windows) atomicAdd(ctr + 3, static_cast<unsigned long long>(windows));
        }
        if (threadIdx.x == 0 && n_q) atomicAdd(ctr + 2, static_cast<unsigned long long>(n_q));
    }
}

// Row j is sorted word j: the window is read again, as text.
__global__ __launch_bounds__(256) void k_variants_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                         VariantArgs a, const issl_search_query *__restrict__ q, uint32_t q_base,
                                                         const uint64_t *__restrict__ starts, uint32_t n_records, uint32_t pos_bits,
                                                         uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t w = words[j];
    const uint32_t strand = static_cast<uint32_t>(w & 1u);
    const uint64_t pos = (w >> 1) & ((1ull << pos_bits) - 1);
    const uint32_t qi = static_cast<uint32_t>(w >> (pos_bits + 1));
    vt::RowFields f{};
    vt::window_row(s + pos, a, strand, q[qi].sig, q[qi].care, f);
    const uint32_t rec = last_not_above(starts, n_records, pos);
    uint64_t *row = rows + 5ull * j; // issl_variant_hit: pos, site[4], record | query, mism | strand | dist | n_var | reserved
    row[0] = pos - starts[rec];
    row[1] = f.site.p[0] | (static_cast<uint64_t>(f.site.p[1]) << 32);
    row[2] = f.site.p[2] | (static_cast<uint64_t>(f.site.p[3]) << 32);
    row[3] = rec | (static_cast<uint64_t>(q_base + qi) << 32);
    row[4] = f.mism | (static_cast<uint64_t>(strand) << 32) | (static_cast<uint64_t>(f.dist) << 40) | (static_cast<uint64_t>(f.n_var) << 48);
}

// ---- SNPs onto the text --------------------------------------------------------------------------------------------

// One thread per place: the byte is one of the 14 codes, holds ref, and its set united with alt is not all four bases
// (N, which no window may hold) -- or *failed becomes the smallest input index of such a place.  Nothing is written to
// the text.
__global__ __launch_bounds__(256) void k_snp_check(const uint8_t *__restrict__ s, const vt::SnpPlace *__restrict__ places, uint32_t n,
                                                   uint32_t *__restrict__ failed)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t set = vt::text_set(s[places[k].at]);
    if (!(set & places[k].ref) || (set | places[k].alt) == 15u) atomicMin(failed, places[k].index);
}

// One thread per place, after every check has passed: the byte becomes the letter of its set united with alt.
__global__ __launch_bounds__(256) void k_snp_apply(uint8_t *__restrict__ s, const vt::SnpPlace *__restrict__ places, uint32_t n,
                                                   unsigned long long *__restrict__ changed)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t set = vt::text_set(s[places[k].at]), next = set | places[k].alt;
    if (next == set) return;
    s[places[k].at] = static_cast<uint8_t>(vt::set_letter(next));
    atomicAdd(changed, 1ull);
}

// ---- host: the unit as SearchDriver takes it (issl_search_device.hpp) ----------------------------------------------------

struct VariantSearch {
    using Row = issl_variant_hit;
    using Call = VariantCall;
    static constexpr size_t kPieceQueries = size_t(1) << 22; // 22 bits of query + 41 of position + 1 of strand = one word
    static constexpr uint32_t kLowBits = 0;
    static constexpr const char *kTag = "[issl variants]", *kRows = "hits";
    static std::string counted(const Call &c) { return ", at most " + std::to_string(c.a.max_variants) + " variants"; }
    static bool nothing(const issl_genome *g, const Call &c, size_t n) { return n == 0 || g->len < c.a.length; }
    static size_t bins(const Call &c) { return c.a.max_dist + 1; }

    // The first launch of a piece (kCount, or kProfile alone) expands its queries; kEmit follows kCount on the same piece.
    template <int kMode>
    static void launch(const issl_genome *g, const Call &c, const issl_search_query *d_q, uint32_t n, unsigned long long *ctr, uint64_t *words,
                       uint64_t cap, unsigned long long *counts, hipStream_t stream)
    {
        if (kMode != kEmit)
            hipLaunchKernelGGL(k_variant_queries, dim3((n + 255) / 256), dim3(256), 0, stream, d_q, n, c.a.win_mask, c.q_planes);
        hipLaunchKernelGGL(k_variants<kMode>, dim3(text_blocks(g)), dim3(256), 0, stream, static_cast<const uint8_t *>(g->seq.p), g->len, c.a,
                           static_cast<const Planes *>(c.q_planes), n, g->pos_bits, ctr, words, cap, counts);
    }

    static void finish(const issl_genome *g, const Call &c, const uint64_t *words, uint32_t total, const issl_search_query *d_q,
                       uint32_t q_base, uint64_t *rows, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_variants_finish, dim3((total + 255) / 256), dim3(256), 0, stream, words, total,
                           static_cast<const uint8_t *>(g->seq.p), c.a, d_q, q_base, static_cast<const uint64_t *>(g->starts.p),
                           static_cast<uint32_t>(g->records.size()), g->pos_bits, rows);
    }
};
using Variants = SearchDriver<VariantSearch>;

// The checks of a call before any device work.  ISSL_OK: c->a is what the kernels take.
int check_variant_call(const issl_search_pattern *pat, int max_dist, int max_variants, size_t n, VariantCall *c)
{
    SearchArgs plain;
    if (int rc = check_call(pat, max_dist, n, &plain)) return rc;
    std::string err;
    if (!vt::check_max_variants(pat, max_variants, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    c->a = vt::make_args(*pat, max_dist, max_variants);
    c->q_planes = nullptr;
    return ISSL_OK;
}

// Room for the planes of one piece's queries, on the handle's device.
int piece_planes(issl_genome *g, size_t n, DevBuf &buf, VariantCall *c)
{
    HIP_TRY(hipSetDevice(g->device));
    const size_t piece = std::min(n, VariantSearch::kPieceQueries);
    if (piece) HIP_TRY(hipMalloc(&buf.p, sizeof(Planes) * piece));
    c->q_planes = static_cast<Planes *>(buf.p);
    return ISSL_OK;
}

int apply_snps(issl_genome *g, const issl_snp *snps, size_t n, uint64_t *n_changed)
{
    if (n_changed) *n_changed = 0;
    if (n > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 snps in one call");
        return ISSL_E_UNSUPPORTED;
    }
    std::vector<uint64_t> starts(g->records.size()), lengths(g->records.size());
    for (size_t r = 0; r < g->records.size(); ++r) starts[r] = g->records[r].start, lengths[r] = g->records[r].length;
    std::vector<vt::SnpPlace> places;
    std::string err;
    if (!vt::merge_snps(snps, n, starts.data(), lengths.data(), starts.size(), places, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    if (places.empty()) return ISSL_OK;
    HIP_TRY(hipSetDevice(g->device));
    const uint32_t count = static_cast<uint32_t>(places.size());
    DevBuf d_places, d_state; // state: failed (uint32, in a word of its own), then changed
    HIP_TRY(hipMalloc(&d_places.p, sizeof(vt::SnpPlace) * places.size()));
    HIP_TRY(hipMalloc(&d_state.p, 16));
    HIP_TRY(hipMemcpy(d_places.p, places.data(), sizeof(vt::SnpPlace) * places.size(), hipMemcpyHostToDevice));
    unsigned long long state[2] = {0xFFFFFFFFull, 0};
    HIP_TRY(hipMemcpy(d_state.p, state, sizeof state, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_snp_check, dim3((count + 255) / 256), dim3(256), 0, nullptr, static_cast<const uint8_t *>(g->seq.p),
                       static_cast<const vt::SnpPlace *>(d_places.p), count, static_cast<uint32_t *>(d_state.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(state, d_state.p, sizeof state, hipMemcpyDeviceToHost));
    if (static_cast<uint32_t>(state[0]) != 0xFFFFFFFFu) {
        set_error("snp " + std::to_string(static_cast<uint32_t>(state[0])) +
                  ": the text there is none of the 14 codes ACGTRYSWKMBDHV, does not hold ref, or would stand for all four bases; nothing was changed");
        return ISSL_E_ARG;
    }
    hipLaunchKernelGGL(k_snp_apply, dim3((count + 255) / 256), dim3(256), 0, nullptr, static_cast<uint8_t *>(g->seq.p),
                       static_cast<const vt::SnpPlace *>(d_places.p), count, static_cast<unsigned long long *>(d_state.p) + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(state, d_state.p, sizeof state, hipMemcpyDeviceToHost));
    if (n_changed) *n_changed = state[1];
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_genome_search_variants(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                                int max_variants, uint64_t *offsets, issl_variant_hit *hits, size_t cap, size_t *n_total)
{
    if (!g || !pat || (!queries && n) || !offsets || !n_total || (!hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantCall c;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &c)) return rc;
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        issl::DevBuf planes;
        if (int rc = issl::piece_planes(g, n, planes, &c)) return rc;
        return issl::Variants::host_rows(g, c, pat->length, queries, n, offsets, hits, cap, n_total);
    });
}

int issl_genome_search_variants_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                       int max_dist, int max_variants, uint64_t *d_offsets, issl_variant_hit *d_hits, size_t cap,
                                       size_t *n_total, void *stream)
{
    if (!g || !pat || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantCall c;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &c)) return rc;
        issl::DevBuf planes;
        if (int rc = issl::piece_planes(g, n, planes, &c)) return rc;
        return issl::Variants::device_rows(g, c, d_queries, n, d_offsets, d_hits, cap, n_total, stream);
    });
}

int issl_genome_search_variants_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n,
                                        int max_dist, int max_variants, uint64_t *counts)
{
    if (!g || !pat || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantCall c;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &c)) return rc;
        if (int rc = issl::check_host_queries(queries, n, pat->length)) return rc;
        issl::DevBuf planes;
        if (int rc = issl::piece_planes(g, n, planes, &c)) return rc;
        return issl::Variants::host_profile(g, c, pat->length, queries, n, counts);
    });
}

int issl_genome_search_variants_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries,
                                               size_t n, int max_dist, int max_variants, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantCall c;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &c)) return rc;
        issl::DevBuf planes;
        if (int rc = issl::piece_planes(g, n, planes, &c)) return rc;
        return issl::Variants::device_profile(g, c, d_queries, n, d_counts, stream);
    });
}

int issl_vcf_snps(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                  size_t n_records, issl_snp *out, size_t cap, size_t *n, issl_vcf_counts *counts)
{
    if ((!vcf && len) || (n_records && (!names || !name_lens || !lengths)) || !n || (!out && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        std::string err;
        if (issl::variants_text::vcf_snps(vcf, len, names, name_lens, lengths, n_records, out, cap, n, counts, err)) return ISSL_OK;
        issl::set_error(err);
        return ISSL_E_ARG;
    });
}

int issl_genome_apply_snps(issl_genome *g, const issl_snp *snps, size_t n, uint64_t *n_changed)
{
    if (!g || (!snps && n)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int { return issl::apply_snps(g, snps, n, n_changed); });
}

int issl_genome_apply_vcf(issl_genome *g, const char *vcf, size_t len, issl_vcf_counts *counts, uint64_t *n_changed)
{
    if (!g || (!vcf && len)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        const size_t n_records = g->records.size();
        std::vector<const char *> names(n_records);
        std::vector<size_t> name_lens(n_records);
        std::vector<uint64_t> lengths(n_records);
        for (size_t r = 0; r < n_records; ++r) {
            names[r] = g->records[r].name.data();
            name_lens[r] = g->records[r].name.size();
            lengths[r] = g->records[r].length;
        }
        std::string err;
        std::vector<issl_snp> snps;
        issl_vcf_counts c{};
        if (!issl::variants_text::read_vcf(vcf, len, names.data(), name_lens.data(), lengths.data(), n_records, snps, c, err)) {
            issl::set_error(err);
            return ISSL_E_ARG;
        }
        if (counts) *counts = c;
        return issl::apply_snps(g, snps.data(), snps.size(), n_changed);
    });
}

} // extern "C"
