// The rules by which RNAfold's output is read (issl_folds_*, include/issl_hip.h): Crackling.py:439-497 over bytes -- the
// lines of a text-mode file, rstrip(), the key guide[1:20], the three text columns, the two regular expressions of :396-397
// and the number behind them.  Host and device run the same code (issl_folds.hip: one thread per row of the fold list;
// tools/folds_sanitize.cpp: a CPU program under AddressSanitizer + UBSan); no device call, no table, no array indexed at
// run time.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ISSL_FT_HD __host__ __device__ __forceinline__
#else
#define ISSL_FT_HD inline
#endif

namespace issl {
namespace folds_text {

enum Kind : uint32_t { kFine = 0, kFormat = 1, kUnsupported = 2 }; // what a looked-up pair can be refused for
constexpr uint32_t kNoText = 0xFFFFFFFFu;                           // issl_text_span.length of a column that keeps '?'

// Python's str.isspace() / \s below 128, which rstrip() removes: TAB LF VT FF CR, FS GS RS US, blank.
ISSL_FT_HD bool is_space(uint8_t c) { return (c >= 0x09u && c <= 0x0du) || (c >= 0x1cu && c <= 0x20u); }
ISSL_FT_HD bool is_eol(uint8_t c) { return c == '\n' || c == '\r'; }
// Does byte c end a line when `next` follows it (0 behind the text)?  CR LF ends once, at its LF.
ISSL_FT_HD bool ends_line(uint8_t c, uint8_t next) { return c == '\n' || (c == '\r' && next != '\n'); }

// Line ends 64 bytes at a time, as k_folds_mark and k_folds_pairs find them.  The four bytes of the little-endian word w
// are bytes at .. at + 3 of a group: their LF and CR bits into the group's two masks.
ISSL_FT_HD void byte_masks(uint32_t w, uint32_t at, uint64_t &lf, uint64_t &cr)
{
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = (w >> (8 * k)) & 0xFFu;
        lf |= static_cast<uint64_t>(c == '\n') << (at + k);
        cr |= static_cast<uint64_t>(c == '\r') << (at + k);
    }
}
// Bit b: byte b of the group ends a line.  here: bytes of the text in this group and behind it (> 0); next_is_lf: the byte
// behind the group is LF.  What lies behind the text is nobody's line end, and no LF behind a CR.
ISSL_FT_HD uint64_t group_line_ends(uint64_t lf, uint64_t cr, uint64_t here, bool next_is_lf)
{
    if (here < 64) {
        lf &= (1ull << here) - 1;
        cr &= (1ull << here) - 1;
    }
    return lf | (cr & ~((lf >> 1) | (static_cast<uint64_t>(next_is_lf) << 63)));
}

// The line that starts at s stops at the first CR or LF, or at the text's end.
ISSL_FT_HD uint64_t line_stop(const uint8_t *t, uint64_t s, uint64_t len)
{
    while (s < len && !is_eol(t[s])) ++s;
    return s;
}
// Where the next line starts behind a line that stopped at e < len.
ISSL_FT_HD uint64_t next_line(const uint8_t *t, uint64_t e, uint64_t len)
{
    return (t[e] == '\r' && e + 1 < len && t[e + 1] == '\n') ? e + 2 : e + 1;
}
// rstrip(): the end of [s, e) without its trailing blanks.
ISSL_FT_HD uint64_t strip_end(const uint8_t *t, uint64_t s, uint64_t e)
{
    while (e > s && is_space(t[e - 1])) --e;
    return e;
}

// Where the text's last line starts (len for an empty text): the one line that can be without a partner.
ISSL_FT_HD uint64_t last_line_start(const uint8_t *t, uint64_t len)
{
    if (len == 0) return 0;
    uint64_t e = len - 1; // the last byte: a terminator (LF, a lone CR, the LF of CR LF) or the last byte of an open line
    if (t[e] == '\n' && e > 0 && t[e - 1] == '\r') --e;
    if (is_eol(t[e])) { // the line this terminator ends
        while (e > 0 && !is_eol(t[e - 1])) --e;
        return e;
    }
    while (e > 0 && !is_eol(t[e - 1])) --e;
    return e;
}

// The key of the pair whose first line starts at s: bytes [1, 20) of the line, U read as T, two bits per base (A 0, C 1,
// G 2, T 3; byte 1 in bits 0-1, as bases 1 .. 19 of issl_guide.guide23 >> 2).  False for a line with fewer than 20 bytes
// ahead of its blanks or a byte other than A C G T U among the nineteen: no guide looks such a pair up.
ISSL_FT_HD bool pair_key(const uint8_t *t, uint64_t s, uint64_t len, uint64_t &key)
{
    if (len - s < 20 || is_eol(t[s])) return false; // (s <= len)
    uint64_t k = 0;
    for (uint32_t p = 1; p < 20; ++p) {
        const uint8_t c = t[s + p];
        const uint32_t code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : (c == 'T' || c == 'U') ? 3u : 4u;
        if (code > 3u) return false;
        k |= static_cast<uint64_t>(code) << (2 * (p - 1));
    }
    key = k;
    return true;
}

ISSL_FT_HD bool same_bytes(const uint8_t *t, const char *lit, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (t[i] != static_cast<uint8_t>(lit[i])) return false;
    return true;
}

// The number text [a, b): blanks and TABs around it, an optional sign, digits[.digits] or .digits.  The value is the digit
// string as an integer divided by 10^(fraction digits), one IEEE division: correctly rounded up to 15 digits (leading zeros
// of the integer part do not count), kUnsupported beyond.
ISSL_FT_HD uint32_t read_number(const uint8_t *t, uint64_t a, uint64_t b, double &value)
{
    while (a < b && (t[a] == ' ' || t[a] == '\t')) ++a;
    while (b > a && (t[b - 1] == ' ' || t[b - 1] == '\t')) --b;
    bool negative = false;
    if (a < b && (t[a] == '+' || t[a] == '-')) negative = t[a++] == '-';
    uint64_t v = 0, digits = 0, counted = 0, fraction = 0;
    for (; a < b && t[a] >= '0' && t[a] <= '9'; ++a) {
        ++digits;
        if (counted || t[a] != '0') ++counted;
        if (counted <= 15) v = v * 10 + (t[a] - '0');
    }
    if (a < b && t[a] == '.') {
        for (++a; a < b && t[a] >= '0' && t[a] <= '9'; ++a) {
            ++digits;
            ++counted;
            ++fraction;
            if (counted <= 15) v = v * 10 + (t[a] - '0');
        }
    }
    if (a != b || digits == 0) return kFormat;
    if (counted > 15) return kUnsupported;
    double scale = 1.0;
    for (uint64_t i = 0; i < fraction; ++i) scale *= 10.0; // exact: at most 10^15
#if defined(__HIP_DEVICE_COMPILE__)
    const double q = __ddiv_rn(static_cast<double>(v), scale);
#else
    const double q = static_cast<double>(v) / scale;
#endif
    value = negative ? -q : q;
    return kFine;
}

// The bytes a CSV field is quoted for (csv.QUOTE_MINIMAL under one of the table's five delimiters), as bits: ',' 1, TAB 2,
// ';' 4, '|' 8, ' ' 16; '"', CR or LF 32.  quote_bits: those that stand in [a, a + n).  A span of the folds carries them in
// its `reserved` word, so that the table knows without reading the text whether a field needs quotes.
ISSL_FT_HD uint32_t quote_bit(uint8_t c)
{
    return c == ',' ? 1u : c == '\t' ? 2u : c == ';' ? 4u : c == '|' ? 8u : c == ' ' ? 16u : (c == '"' || c == '\r' || c == '\n') ? 32u : 0u;
}
ISSL_FT_HD uint32_t quote_bits(const uint8_t *t, uint64_t a, uint32_t n)
{
    uint32_t bits = 0;
    for (uint32_t i = 0; i < n; ++i) bits |= quote_bit(t[a + i]);
    return bits;
}

// What one pair gives its row of the fold list.
struct Pair {
    double energy;
    uint32_t scaffold, present;
    uint64_t offset[3]; // ssL1, ssStructure, ssEnergy: bytes of the text
    uint32_t length[3];
};

// The pair whose first line starts at s (its second line exists) -> kFine and `out`, or why the reference's steps fail.
ISSL_FT_HD uint32_t read_pair(const uint8_t *t, uint64_t len, uint64_t s, Pair &out)
{
    const uint64_t e1 = line_stop(t, s, len), r1 = strip_end(t, s, e1);
    const uint64_t s2 = e1 < len ? next_line(t, e1, len) : len;
    const uint64_t e2 = line_stop(t, s2, len), r2 = strip_end(t, s2, e2);
    out.energy = 0.0;
    out.scaffold = out.present = 0;
    if (r1 - s >= kNoText || r2 - s2 >= kNoText) return kUnsupported; // a span's length has 32 bits
    // :469-474: L1, L2.split(' ')[0], L2.split(' ')[1][1:-1]
    uint64_t b1 = s2;
    while (b1 < r2 && t[b1] != ' ') ++b1;
    if (b1 == r2) return kFormat; // (IndexError in the reference)
    uint64_t b2 = b1 + 1;
    while (b2 < r2 && t[b2] != ' ') ++b2;
    const uint64_t word = b2 - (b1 + 1);
    out.offset[0] = s;
    out.length[0] = static_cast<uint32_t>(r1 - s);
    out.offset[1] = s2;
    out.length[1] = static_cast<uint32_t>(b1 - s2);
    out.offset[2] = word >= 3 ? b1 + 2 : b1 + 1;
    out.length[2] = word >= 3 ? static_cast<uint32_t>(word - 2) : 0u;
    // :481-497: the greedy (.+) of both patterns ends at the line's last ')'
    uint64_t z = r2;
    while (z > s2 && t[z - 1] != ')') --z;
    if (z == s2) return kFine; // no ')': neither pattern matches, the row stays untested
    --z;
    uint64_t number = 0;
    bool matched = false;
    for (uint64_t m = s2; m + 103 <= z; ++m) { // :396, re.search: the leftmost start
        if (t[m + 101] != '(' || !is_space(t[m + 100])) continue;
        if (!same_bytes(t + m + 28, "((((....))))...))))", 19)) continue;
        if (!same_bytes(t + m + 68, "((((....))))(((((((...)))))))...", 32)) continue;
        matched = true;
        number = m + 102;
        out.scaffold = 1;
        break;
    }
    if (!matched) {
        for (uint64_t p = s2; p + 3 <= z; ++p) { // :397
            if (!is_space(t[p]) || t[p + 1] != '(') continue;
            matched = true;
            number = p + 2;
            break;
        }
    }
    if (!matched) return kFine;
    double value = 0.0;
    const uint32_t kind = read_number(t, number, z, value);
    if (kind != kFine) {
        out.scaffold = 0;
        return kind;
    }
    out.energy = value;
    out.present = 1;
    return kFine;
}

} // namespace folds_text
} // namespace issl
