// Genome search with DNA and RNA bulges on a variant-aware text (issl_genome_search_bulges_variants*, include/issl_hip.h):
// the bulge search with IUPAC ambiguity codes in the text read as sets of bases.  The fourth unit of SearchDriver
// (issl_search_device.hpp) with the protocol of issl_search_core.hpp; a piece has up to 2^19 queries.  The front is
// k_variants', from issl_planes_device.hpp, for windows of W = L + b codes: planes and validity plane of the tile in LDS,
// the ambiguity count over all W codes, both strands tested on the forward window against P' and its reversed
// complement, the survivors compacted into the queue of 13-bit tags.  This unit's own:
//   count    k_bulge_variants<kCount>, one launch per bulge b = -R..D (at most seven) with that b's P' and window.  A lane
//            holds one survivor's planes cut by P' and, for a DNA bulge, the same planes shifted down by b; for an RNA
//            bulge the wave-uniform query planes are shifted instead (k_bulge_variants<, kRna>).  Against a query it forms
//            the positions that match at one shift or the other; the rest, A & B, is a lower bound of the distance at every
//            break point (issl_bulge_variants_text.hpp: site coordinates for an RNA bulge).  (t & q) | (tb & q) is
//            (t | tb) & q and (t & q) | (t & qb) is t & (q | qb), so the loop sees one united operand and costs what
//            k_variants' comparison costs.  A wave takes kQueryGroup such
//            words, keeps the greatest count and asks once per group whether any lane is within max_dist; only then the
//            group's queries are taken one by one, and only a query whose own ballot is non-zero walks the break points,
//            incrementally (walk_min)
//   queries  a piece's queries are expanded once into 16-byte records of planes (k_bulge_variant_queries), over the L
//            positions of the query, which every b of the piece reads; behind them one more set per r = 1..R, the planes
//            united with themselves shifted down by r, which is all the bound of an RNA bulge needs of a query
//   emit     a row is one word query | text position | strand | b + R; all b of a piece share one buffer and one sort
//   finish   k_bulge_variants_finish: one thread per row reads the window as text again and recomputes minimum, break
//            point, mism, site and n_var with the functions the hot loop's decision came from (window_row)
//   profile  counts[query][b + R][min dist]
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/issl_hip.h"
#include "issl_bulge_variants_text.hpp"
#include "issl_genome_handle.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_planes_device.hpp"

namespace issl {
namespace {

namespace bvt = bulge_variants_text;
using bvt::BulgeVariantArgs;

constexpr uint32_t kSlotBits = 3; // b + R: 0..6
static_assert(sizeof(issl_bulge_variant_hit) == 48 && sizeof(issl_search_bulges) == 16, "the layouts of include/issl_hip.h");

// The queries of a piece as planes over their own L positions: out[k], and behind them for every r = 1..max_rna the planes
// the bound of an RNA bulge of r bases takes, out[r * n + k] = the query's planes united with the same shifted down by r.
__global__ __launch_bounds__(256) void k_bulge_variant_queries(const issl_search_query *__restrict__ q, uint32_t n, uint32_t query_mask,
                                                               uint32_t max_rna, Planes *__restrict__ out)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const Planes one = vt::query_planes(q[k].sig, q[k].care, query_mask);
    out[k] = one;
    for (uint32_t r = 1; r <= max_rna; ++r) out[static_cast<size_t>(r) * n + k] = bvt::united(one, bvt::shifted_query(one, r));
}

// ctr[0]: rows; ctr[1]: the cursor of k_bulge_variants<kEmit>; ctr[2]: window-strands the patterns admit; ctr[3]: windows
// of codes with at most max_variants ambiguous positions, summed over the launches of a piece (the figures of the timing
// line, kCount only).
template <int kMode, bool kRna>
__global__ __launch_bounds__(256) void k_bulge_variants(const uint8_t *__restrict__ s, uint64_t len, BulgeVariantArgs v,
                                                        const Planes *__restrict__ q, uint32_t n, uint32_t pos_bits,
                                                        unsigned long long *__restrict__ ctr, uint64_t *__restrict__ words, uint64_t cap,
                                                        unsigned long long *__restrict__ counts)
{
    // plane b and the validity bits as 32-bit words; a thread writes the 16-bit half of its 16 positions
    __shared__ uint32_t tile[5][kPlaneWords];
    __shared__ uint16_t queue[2 * kPosPerBlock]; // tag = position in the tile << 1 | strand
    __shared__ uint32_t q_count;
    const vt::VariantArgs &a = v.a;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) q_count = 0;
    fill_planes16(s, base + 16ull * threadIdx.x, len, tile, threadIdx.x);
    if (threadIdx.x < 2) fill_planes16(s, base + kPosPerBlock + 16ull * threadIdx.x, len, tile, 256 + threadIdx.x); // the halo
    __syncthreads();
    uint32_t pass, windows; // the pattern P' on the windows of W codes
    test_plane_windows(a, tile, pass, windows);
    queue_survivors(pass, lane, queue, q_count);
    __syncthreads();
    const uint32_t n_q = q_count;

    // -- every survivor against every query: a lane holds one survivor's planes at both shifts, a wave its quarter of the
    // queries
    const QueryRange mine_q = wave_queries(n);
    const Planes *__restrict__ qs = kRna ? q + static_cast<size_t>(v.g.r) * n : q; // the planes the bound takes
    const uint32_t need = v.both_bits - min(a.max_dist, v.both_bits); // positions that match at either shift, at least
    unsigned long long found = 0; // kCount: the rows of this lane's survivors
    for (uint32_t j0 = 0; j0 < n_q && mine_q.lo < mine_q.hi; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool valid = j < n_q;
        uint32_t tag = 0;
        Planes t{{0, 0, 0, 0}}; // what the strand reads, cut by P': nothing matches where there is no survivor
        if (valid) {
            tag = queue[j];
            t = survivor_planes(tag, tile, a);
        }
        const Planes tb = bvt::shifted_text(t, v.g.b); // (an RNA bulge: t itself, no further registers)
        // the positions of one query that match at either shift (match_either), the two shifts folded into one operand: the
        // lane's planes united here for a DNA bulge, the query's by k_bulge_variant_queries for an RNA bulge (qs).  Five
        // vector instructions and a popcount per query either way
        const Planes te = kRna ? t : bvt::united(t, tb);
        auto either = [&](const Planes &folded) { return vt::matches(te, folded); };
        const uint64_t live = __ballot(valid);
        uint32_t mine = 0; // kCount
        // one query whose bound some lane meets: the break points, for the whole wave (the query's planes are wave-uniform)
        auto walk = [&](const Planes &folded, uint32_t qi) {
            if (!(__ballot(static_cast<uint32_t>(__builtin_popcount(either(folded))) >= need) & live)) return;
            const Planes one = kRna ? q[qi] : folded; // (an RNA bulge: the query's own planes, fetched for the few that walk)
            const Planes qb = kRna ? bvt::shifted_query(one, v.g.r) : one;
            uint32_t brk;
            const uint32_t dist = bvt::walk_min(bvt::mismatch_a(t, one, v.both_mask), bvt::mismatch_b(kRna ? t : tb, qb, v.both_mask), v.g, brk);
            const bool hit = valid && dist <= a.max_dist;
            if (kMode == kCount) {
                mine += hit ? 1u : 0u;
                return;
            }
            const uint64_t who = __ballot(hit);
            if (!who) return;
            if (kMode == kEmit) emit_hits<kSlotBits>(who, hit, lane, ctr, words, cap, qi, pos_bits, base, tag, v.g.slot);
            else profile_hits(who, hit, dist, lane, counts, static_cast<uint64_t>(qi) * v.g.slots + v.g.slot, a.max_dist + 1);
        };
        // the group's bounds share one comparison and one branch
        uint32_t qi = mine_q.lo;
        if (mine_q.hi - mine_q.lo >= kQueryGroup) {
            PlaneGroup next = *reinterpret_cast<const PlaneGroup *>(qs + qi);
            for (; qi + kQueryGroup <= mine_q.hi; qi += kQueryGroup) {
                const PlaneGroup group = next;
                if (qi + 2 * kQueryGroup <= mine_q.hi) next = *reinterpret_cast<const PlaneGroup *>(qs + qi + kQueryGroup);
                uint32_t most = 0;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) most = max(most, static_cast<uint32_t>(__builtin_popcount(either(group.q[u]))));
                if (!(__ballot(most >= need) & live)) continue;
#pragma unroll
                for (uint32_t u = 0; u < kQueryGroup; ++u) walk(group.q[u], qi + u);
            }
        }
        for (; qi < mine_q.hi; ++qi) walk(qs[qi], qi);
        if (kMode == kCount && valid) found += mine;
    }
    if (kMode == kCount) count_totals(windows, found, n_q, lane, ctr);
}

// What the finish kernel takes: the launches of a call by slot b + R.
struct BulgeVariantSlots { BulgeVariantArgs v[7]; };

// Row j is sorted word j: the window of L + b codes is read again, as text.
__global__ __launch_bounds__(256) void k_bulge_variants_finish(const uint64_t *__restrict__ words, uint32_t total, const uint8_t *__restrict__ s,
                                                               BulgeVariantSlots slots, const issl_search_query *__restrict__ q,
                                                               uint32_t q_base, const uint64_t *__restrict__ starts, uint32_t n_records,
                                                               uint32_t pos_bits, uint64_t *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    uint32_t qi, strand, slot;
    uint64_t pos;
    decode_hit<kSlotBits>(words[j], pos_bits, qi, pos, strand, slot);
    const BulgeVariantArgs &v = slots.v[slot < 7 ? slot : 0];
    bvt::RowFields f{};
    (void)bvt::window_row(s + pos, v, strand, q[qi].sig, q[qi].care, f);
    const uint32_t rec = last_not_above(starts, n_records, pos);
    // issl_bulge_variant_hit: pos, site[4], record | query, mism | strand | dist | n_var | bulge, at | reserved
    uint64_t *row = rows + 6ull * j;
    row[0] = pos - starts[rec];
    row[1] = f.site.p[0] | (static_cast<uint64_t>(f.site.p[1]) << 32);
    row[2] = f.site.p[2] | (static_cast<uint64_t>(f.site.p[3]) << 32);
    row[3] = rec | (static_cast<uint64_t>(q_base + qi) << 32);
    row[4] = f.mism | (static_cast<uint64_t>(strand) << 32) | (static_cast<uint64_t>(f.dist) << 40) | (static_cast<uint64_t>(f.n_var) << 48) |
             (static_cast<uint64_t>(static_cast<uint8_t>(v.g.b)) << 56);
    row[5] = f.at;
}

// ---- host --------------------------------------------------------------------------------------------------------

// k_bulge_variants<kMode, kRna> on the text grid.
template <int kMode, class... Args> void launch_bulge_variants(bool rna, uint32_t blocks, hipStream_t stream, Args... args)
{
    if (rna) hipLaunchKernelGGL((k_bulge_variants<kMode, true>), dim3(blocks), dim3(256), 0, stream, args...);
    else hipLaunchKernelGGL((k_bulge_variants<kMode, false>), dim3(blocks), dim3(256), 0, stream, args...);
}

// One call: the launches of its b in ascending order (launch k has slot k).
struct BulgeVariantCall {
    issl_search_bulges bg{};
    uint32_t max_dist = 0, max_variants = 0, query_mask = 0, n_launches = 0;
    BulgeVariantSlots s{};
};

// The launches whose window fits the text.
template <class F> void for_each_launch(const issl_genome *g, const BulgeVariantCall &c, F &&f)
{
    for (uint32_t k = 0; k < c.n_launches; ++k)
        if (g->len >= c.s.v[k].a.length) f(c.s.v[k]);
}

// The unit as SearchDriver takes it (issl_search_device.hpp).
struct BulgeVariantSearch {
    using Row = issl_bulge_variant_hit;
    using Call = BulgeVariantCall;
    static constexpr size_t kPieceQueries = size_t(1) << 19; // 19 bits of query + 41 of position + 1 of strand + 3 of bulge = one word
    static constexpr uint32_t kLowBits = kSlotBits;
    static constexpr const char *kTag = "[issl bulges+variants]", *kRows = "rows";
    static std::string counted(const Call &c)
    {
        return ", " + std::to_string(c.n_launches) + " bulges, at most " + std::to_string(c.max_variants) + " variants";
    }
    static bool nothing(const issl_genome *g, const Call &c, size_t n)
    {
        bool any = false;
        for_each_launch(g, c, [&](const BulgeVariantArgs &) { any = true; });
        return n == 0 || !any;
    }
    static size_t bins(const Call &c) { return static_cast<size_t>(c.bg.max_rna + c.bg.max_dna + 1) * (c.max_dist + 1); }
    // the planes of a piece's queries and one more set per r
    static size_t scratch_bytes(const Call &c, size_t n) { return sizeof(Planes) * n * (1 + c.bg.max_rna); }

    // The first launch of a piece (kCount, or kProfile alone) expands its queries; kEmit follows kCount on the same piece.
    template <int kMode>
    static void launch(const issl_genome *g, const Call &c, const issl_search_query *d_q, uint32_t n, void *scratch, unsigned long long *ctr,
                       uint64_t *words, uint64_t cap, unsigned long long *counts, hipStream_t stream)
    {
        Planes *q_planes = static_cast<Planes *>(scratch);
        if (kMode != kEmit)
            hipLaunchKernelGGL(k_bulge_variant_queries, dim3((n + 255) / 256), dim3(256), 0, stream, d_q, n, c.query_mask, c.bg.max_rna, q_planes);
        for_each_launch(g, c, [&](const BulgeVariantArgs &v) {
            launch_bulge_variants<kMode>(v.g.r != 0, text_blocks(g), stream, static_cast<const uint8_t *>(g->seq.p), g->len, v,
                                         static_cast<const Planes *>(q_planes), n, g->pos_bits, ctr, words, cap, counts);
        });
    }

    static void finish(const issl_genome *g, const Call &c, const uint64_t *words, uint32_t total, const issl_search_query *d_q,
                       uint32_t q_base, uint64_t *rows, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_bulge_variants_finish, dim3((total + 255) / 256), dim3(256), 0, stream, words, total,
                           static_cast<const uint8_t *>(g->seq.p), c.s, d_q, q_base, static_cast<const uint64_t *>(g->starts.p),
                           static_cast<uint32_t>(g->records.size()), g->pos_bits, rows);
    }
};
using BulgedVariants = SearchDriver<BulgeVariantSearch>;

// The checks every entry point makes before any device work.  ISSL_OK: *c holds the launches.
int check_bulge_variant_call(const issl_search_pattern *pat, const issl_search_bulges *bg, int max_dist, int max_variants, size_t n,
                             BulgeVariantCall *c)
{
    SearchArgs plain;
    if (int rc = check_call(pat, max_dist, n, &plain)) return rc;
    std::string err;
    if (!search_text::check_bulges(pat, bg, err) || !vt::check_max_variants(pat, max_variants, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    c->bg = *bg;
    c->max_dist = static_cast<uint32_t>(max_dist);
    c->max_variants = static_cast<uint32_t>(max_variants);
    c->query_mask = search_text::low_bits32(pat->length);
    c->n_launches = 0;
    for (int32_t b = -static_cast<int32_t>(bg->max_rna); b <= static_cast<int32_t>(bg->max_dna); ++b)
        c->s.v[c->n_launches++] = bvt::make_args(*pat, *bg, b, max_dist, max_variants);
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_genome_search_bulges_variants(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                       const issl_search_query *queries, size_t n, int max_dist, int max_variants, uint64_t *offsets,
                                       issl_bulge_variant_hit *hits, size_t cap, size_t *n_total)
{
    if (!g || !pat || !bulges || (!queries && n) || !offsets || !n_total || (!hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeVariantCall c;
        if (int rc = issl::check_bulge_variant_call(pat, bulges, max_dist, max_variants, n, &c)) return rc;
        return issl::BulgedVariants::host_rows(g, c, pat->length, queries, n, offsets, hits, cap, n_total);
    });
}

int issl_genome_search_bulges_variants_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                              const issl_search_query *d_queries, size_t n, int max_dist, int max_variants,
                                              uint64_t *d_offsets, issl_bulge_variant_hit *d_hits, size_t cap, size_t *n_total,
                                              void *stream)
{
    if (!g || !pat || !bulges || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap))
        return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeVariantCall c;
        if (int rc = issl::check_bulge_variant_call(pat, bulges, max_dist, max_variants, n, &c)) return rc;
        return issl::BulgedVariants::device_rows(g, c, d_queries, n, d_offsets, d_hits, cap, n_total, stream);
    });
}

int issl_genome_search_bulges_variants_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                               const issl_search_query *queries, size_t n, int max_dist, int max_variants,
                                               uint64_t *counts)
{
    if (!g || !pat || !bulges || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeVariantCall c;
        if (int rc = issl::check_bulge_variant_call(pat, bulges, max_dist, max_variants, n, &c)) return rc;
        return issl::BulgedVariants::host_profile(g, c, pat->length, queries, n, counts);
    });
}

int issl_genome_search_bulges_variants_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                                      const issl_search_query *d_queries, size_t n, int max_dist, int max_variants,
                                                      uint64_t *d_counts, void *stream)
{
    if (!g || !pat || !bulges || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::BulgeVariantCall c;
        if (int rc = issl::check_bulge_variant_call(pat, bulges, max_dist, max_variants, n, &c)) return rc;
        return issl::BulgedVariants::device_profile(g, c, d_queries, n, d_counts, stream);
    });
}

} // extern "C"
