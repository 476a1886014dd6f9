// The text side of the genome search (issl_search_* / issl_genome_search*, include/issl_hip.h): the IUPAC table, pattern
// and query text -> the structs the kernels take, the checks of those structs, and the lines bin/isslSearchGenome prints.
// Host code that g++ alone compiles, no HIP and no library call: the library (issl_search.hip), the executable
// (cli_search.cpp) and tools/search_sanitize.cpp (a CPU program under AddressSanitizer + UBSan) include the same header.
// The arithmetic on packed words that the kernels do (window_word, reverse_complement, admits, ...) lives here too, as
// host and device code, so that the CPU program checks the very functions the kernels call against plain character loops.
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

} // namespace search_text
} // namespace issl
