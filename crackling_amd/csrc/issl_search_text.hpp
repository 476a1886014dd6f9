// The text side of the genome search (issl_search_* / issl_genome_search*, include/issl_hip.h): the IUPAC table, pattern
// and query text -> the structs the kernels take, the checks of those structs, and the lines bin/isslSearchGenome prints.
// Host code that g++ alone compiles, no HIP and no library call: the library (issl_search.hip), the executable
// (cli_search.cpp) and tools/search_sanitize.cpp (a CPU program under AddressSanitizer + UBSan) include the same header.
// The arithmetic on packed words that the kernels do (window_word, reverse_complement, admits, ...) lives here too, as
// host and device code, so that the CPU program checks the very functions the kernels call against plain character loops.
// The same holds for the bulge search (issl_genome_search_bulges*, issl_bulge.hip): its two mismatch words, the bound, the
// minimum over the break points, check_bulges and the derived patterns are here, under tools/bulge_sanitize.cpp.
// L = 32 uses all 64 bits of a packed word: nothing here shifts by 64.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/issl_hip.h"

#if defined(__HIPCC__)
#define ISSL_ST_HD __host__ __device__ __forceinline__
#else
#define ISSL_ST_HD inline
#endif

namespace issl {
namespace search_text {

constexpr uint32_t kMaxLength = 32;
constexpr uint64_t kEven = 0x5555555555555555ull;

// ---- packed words: base i in bits 2i and 2i + 1, A C G T = 0..3 ---------------------------------------------------

// The pattern as the kernels use it: by value in the kernel arguments.
struct SearchArgs {
    uint64_t allow[4];  // bit 2i: base b allowed at position i
    uint64_t full;      // bit 2i for every i < length
    uint32_t length;
    uint32_t rev_shift; // 64 - 2 * length (0 for 32 bases: no shift by 64 anywhere)
    uint32_t win_mask;  // the low `length` bits
    uint32_t max_dist;
};

// Bit i of v -> bit 2i.
ISSL_ST_HD uint64_t spread_bits(uint32_t v)
{
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & kEven;
    return x;
}

// Bit 2i of x -> bit i.
ISSL_ST_HD uint32_t gather_even_bits(uint64_t x)
{
    x &= kEven;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return static_cast<uint32_t>(x);
}

ISSL_ST_HD uint64_t reverse_bits64(uint64_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}

// The window that starts k (0..15) bases into w0, out of three words of 16 bases each, cut to the pattern's length
// (in_mask: its low 2 * length bits).
ISSL_ST_HD uint64_t window_word(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t k, uint64_t in_mask)
{
    const uint64_t lo = w0 | (static_cast<uint64_t>(w1) << 32);
    return ((lo >> (2 * k)) | ((static_cast<uint64_t>(w2) << 1) << (63 - 2 * k))) & in_mask; // (k == 0: w2 is shifted out)
}

// f holds `length` bases and zeros above them.
ISSL_ST_HD uint64_t reverse_complement(uint64_t f, uint32_t rev_shift)
{
    uint64_t y = reverse_bits64(~f);                  // base i at the top, its two bits swapped
    y = ((y >> 1) & kEven) | ((y & kEven) << 1);
    return y >> rev_shift;
}

// Every base of t is allowed where it stands.
ISSL_ST_HD bool admits(const SearchArgs &a, uint64_t t)
{
    const uint64_t lo = t & kEven, hi = (t >> 1) & kEven;
    const uint64_t ok = (~lo & ~hi & a.allow[0]) | (lo & ~hi & a.allow[1]) | (~lo & hi & a.allow[2]) | (lo & hi & a.allow[3]);
    return ok == a.full;
}

// Bit 2i: position i is compared (care_even = care & kEven) and differs.
ISSL_ST_HD uint64_t mismatches(uint64_t t, uint64_t sig, uint64_t care_even)
{
    const uint64_t x = t ^ sig;
    return (x | (x >> 1)) & care_even;
}

// The number of compared positions that differ (care_odd = care & ~kEven), in 32-bit halves: a position never lies across
// the two, and the hot loop of k_search needs no 64-bit shift this way.
ISSL_ST_HD uint32_t distance(uint64_t t, uint64_t sig, uint64_t care_odd)
{
    const uint32_t xl = static_cast<uint32_t>(t) ^ static_cast<uint32_t>(sig);
    const uint32_t xh = static_cast<uint32_t>(t >> 32) ^ static_cast<uint32_t>(sig >> 32);
    const uint32_t ml = ((xl << 1) | xl) & static_cast<uint32_t>(care_odd);
    const uint32_t mh = ((xh << 1) | xh) & static_cast<uint32_t>(care_odd >> 32);
    return static_cast<uint32_t>(__builtin_popcount(ml) + __builtin_popcount(mh));
}

// ---- bulges (issl_genome_search_bulges*): a window of L + b bases aligned to the query at two shifts --------------------
// b = d > 0: d bases of the site pair with nothing (DNA bulge); b = -r < 0: r bases of the query pair with nothing (RNA
// bulge).  Left of the break point g0 + i query position j meets t[j], right of it t[j + b].  A and B are the mismatch
// words of the two shifts over the WHOLE query, one bit per position (bit 2j), so that
//   dist(d, i)  = popc(A & low(g0 + i)) + popc(B & ~low(g0 + i))
//   dist(-r, i) = popc(A & low(g0 + i)) + popc(B & ~low(g0 + i + r))
// and popc(A & B) - r is a lower bound of every one of them: the r skipped positions are all that A & B can count and the
// sum does not.  What B holds below position r of an RNA bulge is never inside a mask.

// One b of a call: the break points i_lo..i_hi and what the kernels need to place a row.
struct BulgeArgs {
    int32_t b;       // -R..D
    uint32_t r;      // query positions without a partner: -b for an RNA bulge, else 0
    uint32_t g0;     // guide_start
    uint32_t i_lo, i_hi; // 0, 0 for b = 0; 1..G-1 for a DNA bulge; 1..G-1-r for an RNA bulge
    uint32_t slot;   // b + R: its place in the hit word and in the profile
    uint32_t slots;  // R + D + 1
};

// The low 2n bits, n in 0..32.
ISSL_ST_HD uint64_t low_pairs(uint32_t n) { return n >= 32 ? ~0ull : (1ull << (2 * n)) - 1; }

// t as query position j meets it right of the break point: base j of the result is t[j + b].
ISSL_ST_HD uint64_t bulge_shift(uint64_t t, int32_t b) { return b >= 0 ? t >> (2 * b) : t << (2 * -b); }

// The bound of the hot loop of k_bulge, in 32-bit halves as distance() counts.  popc(A & B) - r holds for every b, but
// for an RNA bulge the r it gives away lets one comparison in a hundred through on random text.  The tight form counts in
// SITE coordinates, where every position has exactly one partner at either shift: site position s meets query position s
// left of the break point and s + r right of it, so with B' = B >> 2r (the query shifted down instead of the text up)
//   dist(-r, i) = popc(A & low(g0 + i)) + popc(B' & ~low(g0 + i)) >= popc(A & B')
// -- the DNA form, nothing subtracted.  One function for both:
//   DNA  tb = t >> 2d, sig_b = sig,       care_both = care
//   RNA  tb = t,       sig_b = sig >> 2r, care_both = care & (care >> 2r)
// (bulge_bound_text, bulge_bound_query; sig_b and care_both are wave-uniform).  Returns popc(A & B) resp. popc(A & B'),
// care_both_odd = care_both & ~kEven; never above any dist(b, i), equal to the distance for b = 0.
ISSL_ST_HD uint64_t bulge_bound_text(uint64_t t, int32_t b) { return b > 0 ? t >> (2 * b) : t; }
ISSL_ST_HD uint64_t bulge_bound_query(uint64_t x, uint32_t r) { return x >> (2 * r); }
ISSL_ST_HD uint32_t bulge_both(uint64_t t, uint64_t tb, uint64_t sig, uint64_t sig_b, uint64_t care_both_odd)
{
    const uint32_t al = static_cast<uint32_t>(t) ^ static_cast<uint32_t>(sig), ah = static_cast<uint32_t>(t >> 32) ^ static_cast<uint32_t>(sig >> 32);
    const uint32_t bl = static_cast<uint32_t>(tb) ^ static_cast<uint32_t>(sig_b), bh = static_cast<uint32_t>(tb >> 32) ^ static_cast<uint32_t>(sig_b >> 32);
    const uint32_t ml = ((al << 1) | al) & ((bl << 1) | bl) & static_cast<uint32_t>(care_both_odd);
    const uint32_t mh = ((ah << 1) | ah) & ((bh << 1) | bh) & static_cast<uint32_t>(care_both_odd >> 32);
    return static_cast<uint32_t>(__builtin_popcount(ml) + __builtin_popcount(mh));
}

// min over i of dist(b, i) and the smallest i that reaches it, from A and B (bit 2j, as mismatches() gives them).  The
// walk is incremental: moving the break point from i to i + 1 hands position g0 + i from B's side to A's.
ISSL_ST_HD uint32_t bulge_min(uint64_t A, uint64_t B, const BulgeArgs &g, uint32_t &at)
{
    const uint32_t x = g.g0 + g.i_lo;
    uint32_t cur = static_cast<uint32_t>(__builtin_popcountll(A & low_pairs(x)) + __builtin_popcountll(B & ~low_pairs(x + g.r)));
    uint32_t best = cur;
    at = g.i_lo;
    for (uint32_t i = g.i_lo; i < g.i_hi; ++i) {
        cur += static_cast<uint32_t>(A >> (2 * (g.g0 + i))) & 1u;
        cur -= static_cast<uint32_t>(B >> (2 * (g.g0 + i + g.r))) & 1u;
        if (cur < best) {
            best = cur;
            at = i + 1;
        }
    }
    return best;
}

// The positions of alignment (b, at) that are paired and differ, bit 2j.
ISSL_ST_HD uint64_t bulge_mism(uint64_t A, uint64_t B, const BulgeArgs &g, uint32_t at)
{
    return (A & low_pairs(g.g0 + at)) | (B & ~low_pairs(g.g0 + at + g.r));
}

// ---- text ----------------------------------------------------------------------------------------------------------

// Bases an IUPAC code stands for, bit b = base b of A C G T; 0: not a code.  Either letter case.
inline uint32_t iupac_bases(char ch)
{
    switch (ch >= 'a' && ch <= 'z' ? ch - 'a' + 'A' : ch) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return 8;
    case 'R': return 1 | 4;
    case 'Y': return 2 | 8;
    case 'S': return 2 | 4;
    case 'W': return 1 | 8;
    case 'K': return 4 | 8;
    case 'M': return 1 | 2;
    case 'B': return 2 | 4 | 8;
    case 'D': return 1 | 4 | 8;
    case 'H': return 1 | 2 | 8;
    case 'V': return 1 | 2 | 4;
    case 'N': return 15;
    default: return 0;
    }
}

// 0..3 for A C G T, 4 for N, 5 for anything else.  Either letter case.
inline uint32_t query_code(char ch)
{
    switch (ch >= 'a' && ch <= 'z' ? ch - 'a' + 'A' : ch) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    case 'N': return 4;
    default: return 5;
    }
}

// The low `bits` bits set, bits in 0..64.
inline uint64_t low_bits64(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }
inline uint32_t low_bits32(uint32_t bits) { return bits >= 32 ? ~0u : (1u << bits) - 1; }

inline std::string shown(char ch)
{
    char buf[16];
    if (ch >= 0x20 && ch < 0x7f) std::snprintf(buf, sizeof buf, "'%c'", ch);
    else std::snprintf(buf, sizeof buf, "byte 0x%02x", static_cast<unsigned>(static_cast<unsigned char>(ch)));
    return buf;
}

// pattern (NUL-terminated) -> *pat.  false + message.
inline bool parse_pattern(const char *pattern, issl_search_pattern *pat, std::string &err)
{
    const size_t len = std::strlen(pattern);
    if (len < 1 || len > kMaxLength) {
        err = "pattern of " + std::to_string(len) + " characters: the length is 1 to 32";
        return false;
    }
    std::memset(pat, 0, sizeof *pat);
    pat->length = static_cast<uint32_t>(len);
    for (size_t i = 0; i < len; ++i) {
        const uint32_t bases = iupac_bases(pattern[i]);
        if (!bases) {
            err = "pattern position " + std::to_string(i) + ": " + shown(pattern[i]) + " is no IUPAC code (ACGTRYSWKMBDHVN)";
            return false;
        }
        for (uint32_t b = 0; b < 4; ++b)
            if (bases >> b & 1u) pat->allow[b] |= 1u << i;
    }
    return true;
}

// One query text of `length` characters -> *q.  false + message (`k`: the query's index, for the message).
inline bool parse_query(const char *text, uint32_t length, size_t k, issl_search_query *q, std::string &err)
{
    q->sig = q->care = 0;
    for (uint32_t i = 0; i < length; ++i) {
        const uint32_t c = query_code(text[i]);
        if (c > 4) {
            err = "query " + std::to_string(k) + " position " + std::to_string(i) + ": " + shown(text[i]) + " is not one of ACGTN";
            return false;
        }
        if (c < 4) {
            q->sig |= static_cast<uint64_t>(c) << (2 * i);
            q->care |= 3ull << (2 * i);
        }
    }
    return true;
}

// issl_search_prepare without the library around it.
inline bool prepare(const char *pattern, const char *queries, size_t n, size_t stride, issl_search_pattern *pat,
                    issl_search_query *out, std::string &err)
{
    if (!pattern || !pat || (n && (!queries || !out))) {
        err = "null argument";
        return false;
    }
    if (!parse_pattern(pattern, pat, err)) return false;
    if (n > 1 && stride < pat->length) {
        err = "stride " + std::to_string(stride) + " below the pattern's length " + std::to_string(pat->length);
        return false;
    }
    for (size_t k = 0; k < n; ++k)
        if (!parse_query(queries + k * stride, pat->length, k, out + k, err)) return false;
    return true;
}

// What a search call checks of its pattern and max_dist before any device work.
inline bool check_pattern(const issl_search_pattern *pat, int max_dist, std::string &err)
{
    if (pat->length < 1 || pat->length > kMaxLength) {
        err = "pattern length " + std::to_string(pat->length) + ": 1 to 32";
        return false;
    }
    if (max_dist < 0 || static_cast<uint32_t>(max_dist) > pat->length) {
        err = "max_dist " + std::to_string(max_dist) + ": 0 to the pattern's length " + std::to_string(pat->length);
        return false;
    }
    const uint32_t in = low_bits32(pat->length);
    uint32_t any = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        if (pat->allow[b] & ~in) {
            err = "pattern: allow[" + std::to_string(b) + "] has bits at or above its length " + std::to_string(pat->length);
            return false;
        }
        any |= pat->allow[b];
    }
    for (uint32_t i = 0; i < pat->length; ++i)
        if (!(any >> i & 1u)) {
            err = "pattern position " + std::to_string(i) + " allows no base";
            return false;
        }
    return true;
}

inline SearchArgs make_args(const issl_search_pattern &pat, int max_dist)
{
    SearchArgs a{};
    for (int b = 0; b < 4; ++b) a.allow[b] = spread_bits(pat.allow[b]);
    a.win_mask = low_bits32(pat.length);
    a.full = spread_bits(a.win_mask);
    a.length = pat.length;
    a.rev_shift = 64 - 2 * pat.length;
    a.max_dist = static_cast<uint32_t>(max_dist);
    return a;
}

// Host queries: no bit at or above 2L, care in whole pairs, sig inside care.
inline bool check_queries(const issl_search_query *q, size_t n, uint32_t length, std::string &err)
{
    const uint64_t in = low_bits64(2 * length), even = kEven;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t c = q[k].care;
        if ((c | q[k].sig) & ~in) {
            err = "query " + std::to_string(k) + ": bits at or above position " + std::to_string(length);
            return false;
        }
        if (((c >> 1) & even) != (c & even) || (q[k].sig & ~c)) {
            err = "query " + std::to_string(k) + ": care marks whole positions and sig is 0 where nothing is compared";
            return false;
        }
    }
    return true;
}

// What a bulge search checks of its span and limits, after check_pattern() has passed.
inline bool check_bulges(const issl_search_pattern *pat, const issl_search_bulges *bg, std::string &err)
{
    const uint32_t L = pat->length, g0 = bg->guide_start, G = bg->guide_length, D = bg->max_dna, R = bg->max_rna;
    if (G < 2 || g0 > L || G > L - g0) {
        err = "span (" + std::to_string(g0) + ", " + std::to_string(G) + ") out of range: guide_length is at least 2 and the span lies inside the pattern's " +
              std::to_string(L) + " positions";
        return false;
    }
    if (D > 3 || R > 3) {
        err = std::string(D > 3 ? "max_dna " : "max_rna ") + std::to_string(D > 3 ? D : R) + ": 0 to 3";
        return false;
    }
    if (L + D > kMaxLength) {
        err = "max_dna " + std::to_string(D) + " with a pattern of " + std::to_string(L) + ": the window of a DNA bulge has at most 32 bases";
        return false;
    }
    if (R > G - 2) {
        err = "max_rna " + std::to_string(R) + " with guide_length " + std::to_string(G) + ": at most guide_length - 2";
        return false;
    }
    if (D + R > 0)
        for (uint32_t i = g0 + 1; i + 1 < g0 + G; ++i)
            for (uint32_t b = 0; b < 4; ++b)
                if (!(pat->allow[b] >> i & 1u)) {
                    err = "pattern position " + std::to_string(i) + " is not N: a break point may lie there (only the span's first and last position and what is outside it carry other codes)";
                    return false;
                }
    return true;
}

// P' of bulge b: P[:g0 + 1] + N * (G - 2 + b) + P[g0 + G - 1:], the same for every break point; P itself for b = 0.
inline issl_search_pattern bulge_pattern(const issl_search_pattern &pat, const issl_search_bulges &bg, int32_t b)
{
    if (b == 0) return pat;
    issl_search_pattern out{};
    out.length = static_cast<uint32_t>(static_cast<int32_t>(pat.length) + b);
    const uint32_t head = bg.guide_start + 1, tail_from = bg.guide_start + bg.guide_length - 1;
    const uint32_t tail_to = static_cast<uint32_t>(static_cast<int32_t>(tail_from) + b);
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t tail = static_cast<uint64_t>(pat.allow[k] >> tail_from) << tail_to;
        out.allow[k] = (pat.allow[k] & low_bits32(head)) | (low_bits32(tail_to) & ~low_bits32(head)) | static_cast<uint32_t>(tail);
    }
    return out;
}

ISSL_ST_HD BulgeArgs make_bulge_args(const issl_search_bulges &bg, int32_t b)
{
    BulgeArgs g{};
    g.b = b;
    g.r = b < 0 ? static_cast<uint32_t>(-b) : 0u;
    g.g0 = bg.guide_start;
    g.i_lo = b ? 1u : 0u;
    g.i_hi = b ? bg.guide_length - 1 - g.r : 0u;
    g.slot = static_cast<uint32_t>(b + static_cast<int32_t>(bg.max_rna));
    g.slots = bg.max_rna + bg.max_dna + 1;
    return g;
}

// One row from the window's characters: what the finish pass does per row and a CPU checker per window.  t: the L + b
// bases the strand reads, packed.  false: no alignment of this b is within max_dist.
ISSL_ST_HD bool bulge_row(uint64_t t, const issl_search_query &q, const BulgeArgs &g, uint32_t max_dist, uint32_t &dist, uint32_t &at,
                          uint32_t &mism)
{
    const uint64_t A = mismatches(t, q.sig, q.care & kEven), B = mismatches(bulge_shift(t, g.b), q.sig, q.care & kEven);
    dist = bulge_min(A, B, g, at);
    mism = gather_even_bits(bulge_mism(A, B, g, at));
    return dist <= max_dist;
}

// ---- the lines of bin/isslSearchGenome --------------------------------------------------------------------------

// The query file: one query per line, "\n" or "\r\n" line ends, a trailing blank line is ignored; every line has the
// pattern's length.  The texts end up one after the other in `packed`.  false + message.
inline bool split_query_lines(const std::string &text, uint32_t length, std::string &packed, size_t &n, std::string &err)
{
    std::vector<std::pair<size_t, size_t>> lines;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        const size_t next = e == std::string::npos ? text.size() : e + 1;
        if (e == std::string::npos) e = text.size();
        if (e > p && text[e - 1] == '\r') --e;
        lines.emplace_back(p, e - p);
        p = next;
    }
    if (!lines.empty() && lines.back().second == 0) lines.pop_back();
    packed.clear();
    n = 0;
    for (const auto &l : lines) {
        if (l.second != length) {
            err = "line " + std::to_string(n + 1) + ": " + std::to_string(l.second) + " characters, the pattern has " + std::to_string(length);
            return false;
        }
        packed.append(text, l.first, l.second);
        ++n;
    }
    return true;
}

// "<query text>\t<record name>\t<pos>\t<+|->\t<dist>\t<site>\n": the site's mismatching positions in lower case.
inline void append_hit_line(std::string &out, const char *query, uint32_t length, const char *name, size_t name_len,
                            const issl_search_hit &h)
{
    out.append(query, length);
    out += '\t';
    out.append(name, name_len);
    char buf[64];
    std::snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t", static_cast<unsigned long long>(h.pos), h.strand ? '-' : '+',
                  static_cast<unsigned>(h.dist));
    out += buf;
    for (uint32_t i = 0; i < length; ++i) {
        const char c = "ACGT"[(h.site >> (2 * i)) & 3u];
        out += (h.mism >> i & 1u) ? static_cast<char>(c - 'A' + 'a') : c;
    }
    out += '\n';
}

// "<query text>\t<hits at 0>\t...\t<hits at max_dist>\n"
inline void append_profile_line(std::string &out, const char *query, uint32_t length, const uint64_t *counts, uint32_t max_dist)
{
    out.append(query, length);
    char buf[32];
    for (uint32_t d = 0; d <= max_dist; ++d) {
        std::snprintf(buf, sizeof buf, "\t%llu", static_cast<unsigned long long>(counts[d]));
        out += buf;
    }
    out += '\n';
}

// "<query aligned>\t<record name>\t<pos>\t<+|->\t<dist>\t<0|D1..D3|R1..R3>\t<site aligned>\n": '-' x d in the query at
// g0 + at for a DNA bulge, '-' x r in the site at g0 + at for an RNA bulge; the site's mismatching bases in lower case,
// its unpaired bases in upper case.
inline void append_bulge_line(std::string &out, const char *query, uint32_t length, uint32_t guide_start, const char *name,
                              size_t name_len, const issl_bulge_hit &h)
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
    const uint32_t site_len = length + d - r;
    for (uint32_t s = 0; s < site_len; ++s) {
        if (s == brk) out.append(r, '-');
        const char c = "ACGT"[(h.site >> (2 * s)) & 3u];
        const bool paired = s < brk || s >= brk + d;
        const uint32_t j = s < brk ? s : s - d + r; // the query position it meets
        out += (paired && (h.mism >> j & 1u)) ? static_cast<char>(c - 'A' + 'a') : c;
    }
    out += '\n';
}

} // namespace search_text
} // namespace issl
