// The text side of the bulge search on a variant-aware text (issl_genome_search_bulges_variants*, include/issl_hip.h),
// built on issl_search_text.hpp (the span, the limits, the derived patterns, BulgeArgs) and issl_variants_text.hpp (bit
// planes, the 14 codes) and in their style: host code that g++ alone compiles, no HIP and no library call.  The library
// (issl_bulge_variants.hip), the executable (cli_search.cpp) and tools/bulge_variants_sanitize.cpp (a CPU program under
// AddressSanitizer + UBSan) include the same header, and the plane arithmetic the kernels do lives here as host and device
// code, so that the CPU program checks the very functions the kernels call against character loops.
//
// A window of W = L + b codes is four planes of W bits (what the strand reads, cut by the derived pattern P'); a query is
// four planes of L bits (query_planes: a compared position in its base's plane alone, an N position in all four).  A
// position is ONE bit of a 32-bit word here.  Left of the break point x = g0 + i query position j meets site position j,
// right of it site position j + b.  The two mismatch words are taken in the coordinates in which every position has a
// partner at either shift -- the query's for a DNA bulge (b = d >= 0), the site's for an RNA bulge (b = -r < 0):
//   DNA  A bit j: q[j] does not match t[j];  B bit j: q[j] does not match t[j + d]        (the text shifted down by d)
//   RNA  A bit s: q[s] does not match t[s];  B bit s: q[s + r] does not match t[s]        (the query shifted down by r)
// both cut to the low min(L, W) bits, so that for every break point
//   dist(b, i) = popc(A & low(x)) + popc(B & ~low(x))  >=  popc(A & B)
// -- a position counts on one side or the other, and A & B holds those that count on both.  The positions are independent
// (a set per position), so this is k_bulge's argument unchanged, and its RNA form in site coordinates.  What A holds at
// and above W for an RNA bulge is cut away: no mask low(x) reaches there, x <= g0 + G - 1 - r < W.
#pragma once
#include <cstdint>
#include <string>

#include "issl_search_text.hpp"
#include "issl_variants_text.hpp"

namespace issl {
namespace bulge_variants_text {

using search_text::BulgeArgs;
using variants_text::Planes;
using variants_text::VariantArgs;

// One b of a call: the pattern P' and the window as k_variants takes them, the break points as k_bulge takes them.
struct BulgeVariantArgs {
    VariantArgs a;      // of P': length W = L + b, win_mask the low W bits, max_variants counted over all W codes
    BulgeArgs g;
    uint32_t query_mask; // the low L bits
    uint32_t both_mask;  // the low min(L, W) bits: where A and B live
    uint32_t both_bits;  // their number
};

// The low n bits, n in 0..32.
ISSL_ST_HD uint32_t low32(uint32_t n) { return n >= 32 ? ~0u : (1u << n) - 1; }

ISSL_ST_HD Planes shifted_down(const Planes &p, uint32_t n) { return {{p.p[0] >> n, p.p[1] >> n, p.p[2] >> n, p.p[3] >> n}}; }

// The second pair of planes of the two shifts: the text shifted for a DNA bulge, the (wave-uniform) query for an RNA bulge.
ISSL_ST_HD Planes shifted_text(const Planes &t, int32_t b) { return b > 0 ? shifted_down(t, static_cast<uint32_t>(b)) : t; }
ISSL_ST_HD Planes shifted_query(const Planes &q, uint32_t r) { return shifted_down(q, r); }

// The two mismatch words.  t: the window's planes cut by P'; tb = shifted_text(t, b); q: the query's planes; qb =
// shifted_query(q, r).
ISSL_ST_HD uint32_t mismatch_a(const Planes &t, const Planes &q, uint32_t both_mask) { return ~variants_text::matches(t, q) & both_mask; }
ISSL_ST_HD uint32_t mismatch_b(const Planes &tb, const Planes &qb, uint32_t both_mask) { return ~variants_text::matches(tb, qb) & both_mask; }

// The positions that match at one shift or the other.  Every bit lies inside both_mask: t has W bits, q has L, and the
// shifted planes have fewer.  The hot loop of k_bulge_variants keeps the greatest count of a group of queries.
ISSL_ST_HD uint32_t match_either(const Planes &t, const Planes &tb, const Planes &q, const Planes &qb)
{
    return variants_text::matches(t, q) | variants_text::matches(tb, qb);
}

// The same word with the two shifts folded into one operand, as the hot loop forms it: (t & q) | (tb & q) = (t | tb) & q
// for a DNA bulge, where the lane's planes are united once per survivor, and (t & q) | (t & qb) = t & (q | qb) for an RNA
// bulge, where the query's planes are united on the scalar side.  Five vector instructions per query either way.
ISSL_ST_HD Planes united(const Planes &a, const Planes &b) { return {{a.p[0] | b.p[0], a.p[1] | b.p[1], a.p[2] | b.p[2], a.p[3] | b.p[3]}}; }

// popc(A & B), never above any dist(b, i) and equal to the distance for b = 0, from match_either()'s word.
ISSL_ST_HD uint32_t bound(uint32_t either, uint32_t both_bits) { return both_bits - static_cast<uint32_t>(__builtin_popcount(either)); }

// min over i of dist(b, i) and the smallest i that reaches it.  The walk is incremental: moving the break point from i to
// i + 1 hands position g0 + i from B's side to A's.
ISSL_ST_HD uint32_t walk_min(uint32_t A, uint32_t B, const BulgeArgs &g, uint32_t &at)
{
    const uint32_t x = g.g0 + g.i_lo;
    uint32_t cur = static_cast<uint32_t>(__builtin_popcount(A & low32(x)) + __builtin_popcount(B & ~low32(x)));
    uint32_t best = cur;
    at = g.i_lo;
    for (uint32_t i = g.i_lo; i < g.i_hi; ++i) {
        cur += (A >> (g.g0 + i)) & 1u;
        cur -= (B >> (g.g0 + i)) & 1u;
        if (cur < best) {
            best = cur;
            at = i + 1;
        }
    }
    return best;
}

// The positions of alignment (b, at) that do not match, in QUERY coordinates: B's side moves up by r for an RNA bulge.
ISSL_ST_HD uint32_t walk_mism(uint32_t A, uint32_t B, const BulgeArgs &g, uint32_t at)
{
    const uint32_t left = low32(g.g0 + at);
    return (A & left) | ((B & ~left) << g.r);
}

// The derived-pattern planes of bulge b and everything else the kernels take for it.
inline BulgeVariantArgs make_args(const issl_search_pattern &pat, const issl_search_bulges &bg, int32_t b, int max_dist, int max_variants)
{
    BulgeVariantArgs out{};
    out.a = variants_text::make_args(search_text::bulge_pattern(pat, bg, b), max_dist, max_variants);
    out.g = search_text::make_bulge_args(bg, b);
    out.query_mask = search_text::low_bits32(pat.length);
    out.both_bits = b < 0 ? out.a.length : pat.length;
    out.both_mask = search_text::low_bits32(out.both_bits);
    return out;
}

// One row from the window's characters w[0..W) (upper case): what the finish pass does per row and a CPU checker per
// window.  false: the window holds a byte that is none of the 14 codes.  The caller compares n_var and dist with its
// limits.  site: the sets the strand reads, not cut by the pattern, W positions.
struct RowFields { Planes site; uint32_t mism, dist, at, n_var; bool admitted; };
ISSL_ST_HD bool window_row(const uint8_t *w, const BulgeVariantArgs &v, uint32_t strand, uint64_t sig, uint64_t care, RowFields &out)
{
    Planes f{{0, 0, 0, 0}};
    for (uint32_t i = 0; i < v.a.length; ++i) {
        const uint32_t set = variants_text::text_set(w[i]);
        if (!set) return false;
        for (uint32_t b = 0; b < 4; ++b) f.p[b] |= (set >> b & 1u) << i;
    }
    out.n_var = static_cast<uint32_t>(__builtin_popcount(variants_text::ambiguous(f)));
    out.site = strand ? variants_text::strand1(f, v.a.rev_shift) : f;
    out.admitted = variants_text::admits(out.site, v.a.allow, v.a.win_mask);
    const Planes t = variants_text::intersect(out.site, v.a.allow), q = variants_text::query_planes(sig, care, v.query_mask);
    const uint32_t A = mismatch_a(t, q, v.both_mask), B = mismatch_b(shifted_text(t, v.g.b), shifted_query(q, v.g.r), v.both_mask);
    out.dist = walk_min(A, B, v.g, out.at);
    out.mism = walk_mism(A, B, v.g, out.at);
    return true;
}

// ---- the lines of bin/isslSearchGenome --guide .. --guide-variants ------------------------------------------------------

// append_bulge_line's line with the site in IUPAC letters: lower case where a paired position does not match, upper case
// elsewhere (the unpaired bases of a DNA bulge among them), '-' x r at an RNA bulge.
inline void append_bulge_variant_line(std::string &out, const char *query, uint32_t length, uint32_t guide_start, const char *name,
                                      size_t name_len, const issl_bulge_variant_hit &h)
{
    const uint32_t brk = guide_start + h.at, d = h.bulge > 0 ? static_cast<uint32_t>(h.bulge) : 0u,
                   r = h.bulge < 0 ? static_cast<uint32_t>(-h.bulge) : 0u;
    out.append(query, brk);
    out.append(d, '-');
    out.append(query + brk, length - brk);
    out += '\t';
    out.append(name, name_len);
    char buf[64];
    std::snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t", static_cast<unsigned long long>(h.pos), h.strand ? '-' : '+',
                  static_cast<unsigned>(h.dist));
    out += buf;
    if (h.bulge == 0) out += '0';
    else {
        out += h.bulge > 0 ? 'D' : 'R';
        out += static_cast<char>('0' + d + r);
    }
    out += '\t';
    const Planes t{{h.site[0], h.site[1], h.site[2], h.site[3]}};
    const uint32_t site_len = length + d - r;
    for (uint32_t s = 0; s < site_len; ++s) {
        if (s == brk) out.append(r, '-');
        const char c = variants_text::set_letter(variants_text::set_at(t, s));
        const bool paired = s < brk || s >= brk + d;
        const uint32_t j = s < brk ? s : s - d + r; // the query position it meets
        out += (paired && (h.mism >> j & 1u) && c != '?') ? static_cast<char>(c - 'A' + 'a') : c;
    }
    out += '\n';
}

} // namespace bulge_variants_text
} // namespace issl
