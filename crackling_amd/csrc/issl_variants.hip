// Variant-aware genome search: issl_genome_search with IUPAC ambiguity codes in the text read as sets of bases
// (issl_genome_search_variants*, include/issl_hip.h), and SNPs written onto a resident genome (issl_vcf_snps,
// issl_genome_apply_snps, issl_genome_apply_vcf).  The third unit of SearchDriver (issl_search_device.hpp) with the
// protocol of issl_search_core.hpp; the text as bit planes in place of 2-bit codes, and the front on them, is
// issl_planes_device.hpp's, which issl_bulge_variants.hip includes as well.  This unit's own: a piece's queries are
// expanded once into 16-byte records of planes (k_variant_queries, into the driver's scratch), the same 16 B and the same
// group loads as the plain search's; the comparison is four ANDs ORed together for all 32 positions, five instructions
// and a popcount; k_variants_finish; the SNP kernels.  The plane arithmetic is issl_variants_text.hpp's, which
// tools/variants_sanitize.cpp checks on the CPU.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_planes_device.hpp"

namespace issl {
namespace {

static_assert(sizeof(issl_variant_hit) == 40 && sizeof(issl_snp) == 16 && sizeof(vt::SnpPlace) == 16, "the layouts of include/issl_hip.h");

// The queries of a piece as planes: a compared position in its base's plane alone, an N position in all four.
__global__ __launch_bounds__(256) void k_variant_queries(const issl_search_query *__restrict__ q, uint32_t n, uint32_t win_mask,
                                                         Planes *__restrict__ out)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = vt::query_planes(q[k].sig, q[k].care, win_mask);
}

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
    fill_planes16(s, base + 16ull * threadIdx.x, len, tile, threadIdx.x);
    if (threadIdx.x < 2) fill_planes16(s, base + kPosPerBlock + 16ull * threadIdx.x, len, tile, 256 + threadIdx.x); // the halo
    __syncthreads();
    uint32_t pass, windows;
    test_plane_windows(a, tile, pass, windows);
    queue_survivors(pass, lane, queue, q_count);
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
            t = survivor_planes(tag, tile, a);
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
    if (kMode == kCount) count_totals(windows, found, n_q, lane, ctr);
}

// Row j is sorted word j: the window is read again, as text.
__global__ __launch_bounds__(256) void k_variants_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                         VariantArgs a, const issl_search_query *__restrict__ q, uint32_t q_base,
                                                         const uint64_t *__restrict__ starts, uint32_t n_records, uint32_t pos_bits,
                                                         uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    uint32_t qi, strand, low;
    uint64_t pos;
    decode_hit<0>(words[j], pos_bits, qi, pos, strand, low);
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
    using Call = VariantArgs;
    static constexpr size_t kPieceQueries = size_t(1) << 22; // 22 bits of query + 41 of position + 1 of strand = one word
    static constexpr uint32_t kLowBits = 0;
    static constexpr const char *kTag = "[issl variants]", *kRows = "hits";
    static std::string counted(const Call &a) { return ", at most " + std::to_string(a.max_variants) + " variants"; }
    static bool nothing(const issl_genome *g, const Call &a, size_t n) { return n == 0 || g->len < a.length; }
    static size_t bins(const Call &a) { return a.max_dist + 1; }
    static size_t scratch_bytes(const Call &, size_t n) { return sizeof(Planes) * n; } // the planes of a piece's queries

    // The first launch of a piece (kCount, or kProfile alone) expands its queries; kEmit follows kCount on the same piece.
    template <int kMode>
    static void launch(const issl_genome *g, const Call &a, const issl_search_query *d_q, uint32_t n, void *scratch, unsigned long long *ctr,
                       uint64_t *words, uint64_t cap, unsigned long long *counts, hipStream_t stream)
    {
        Planes *q_planes = static_cast<Planes *>(scratch);
        if (kMode != kEmit) hipLaunchKernelGGL(k_variant_queries, dim3((n + 255) / 256), dim3(256), 0, stream, d_q, n, a.win_mask, q_planes);
        hipLaunchKernelGGL(k_variants<kMode>, dim3(text_blocks(g)), dim3(256), 0, stream, static_cast<const uint8_t *>(g->seq.p), g->len, a,
                           static_cast<const Planes *>(q_planes), n, g->pos_bits, ctr, words, cap, counts);
    }

    static void finish(const issl_genome *g, const Call &a, const uint64_t *words, uint32_t total, const issl_search_query *d_q,
                       uint32_t q_base, uint64_t *rows, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_variants_finish, dim3((total + 255) / 256), dim3(256), 0, stream, words, total,
                           static_cast<const uint8_t *>(g->seq.p), a, d_q, q_base, static_cast<const uint64_t *>(g->starts.p),
                           static_cast<uint32_t>(g->records.size()), g->pos_bits, rows);
    }
};
using Variants = SearchDriver<VariantSearch>;

// The checks of a call before any device work.  ISSL_OK: *a is what the kernels take.
int check_variant_call(const issl_search_pattern *pat, int max_dist, int max_variants, size_t n, VariantArgs *a)
{
    SearchArgs plain;
    if (int rc = check_call(pat, max_dist, n, &plain)) return rc;
    std::string err;
    if (!vt::check_max_variants(pat, max_variants, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    *a = vt::make_args(*pat, max_dist, max_variants);
    return ISSL_OK;
}

int apply_snps(issl_genome *g, const issl_snp *snps, size_t n, uint64_t *n_changed)
{
    if (n_changed) *n_changed = 0;
    if (n > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 snps in one call");
        return ISSL_E_UNSUPPORTED;
    }
    const RecordTable table(g);
    std::vector<vt::SnpPlace> places;
    std::string err;
    if (!vt::merge_snps(snps, n, table.starts.data(), table.lengths.data(), table.size(), places, err)) {
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
        issl::VariantArgs a;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &a)) return rc;
        return issl::Variants::host_rows(g, a, pat->length, queries, n, offsets, hits, cap, n_total);
    });
}

int issl_genome_search_variants_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                       int max_dist, int max_variants, uint64_t *d_offsets, issl_variant_hit *d_hits, size_t cap,
                                       size_t *n_total, void *stream)
{
    if (!g || !pat || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantArgs a;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &a)) return rc;
        return issl::Variants::device_rows(g, a, d_queries, n, d_offsets, d_hits, cap, n_total, stream);
    });
}

int issl_genome_search_variants_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n,
                                        int max_dist, int max_variants, uint64_t *counts)
{
    if (!g || !pat || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantArgs a;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &a)) return rc;
        return issl::Variants::host_profile(g, a, pat->length, queries, n, counts);
    });
}

int issl_genome_search_variants_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries,
                                               size_t n, int max_dist, int max_variants, uint64_t *d_counts, void *stream)
{
    if (!g || !pat || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::VariantArgs a;
        if (int rc = issl::check_variant_call(pat, max_dist, max_variants, n, &a)) return rc;
        return issl::Variants::device_profile(g, a, d_queries, n, d_counts, stream);
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
        const issl::RecordTable table(g);
        std::string err;
        std::vector<issl_snp> snps;
        issl_vcf_counts c{};
        if (!issl::variants_text::read_vcf(vcf, len, table.names.data(), table.name_lens.data(), table.lengths.data(), table.size(), snps, c, err)) {
            issl::set_error(err);
            return ISSL_E_ARG;
        }
        if (counts) *counts = c;
        return issl::apply_snps(g, snps.data(), snps.size(), n_changed);
    });
}

} // extern "C"
