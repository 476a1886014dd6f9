// Python's repr(float) for host and device code: the shortest decimal that reads back as the same double, the one closest
// to it among those, in the notation float_repr_style 'short' prints.  The digits come from Schubfach (R. Giulietti, "The
// Schubfach way to render doubles", 2020), written from the paper's definition: with v = c * 2^q and k = floor(log10(2^q))
// the three values 4c - 2 (or 4c - 1 below a power of two), 4c and 4c + 2 are scaled by 10^-k -- one 64 x 128 bit
// product each against a 128-bit power of ten rounded up (repr_tables.inc, tools/gen_repr_tables.py), the product's lost
// bits folded into its last one ("round to odd") -- and the candidates s, s + 1 (and the shorter s' , s' + 1 of a tenth
// the precision) are tested against the scaled interval.  No big integers, no loop over digits.
// A sink takes the characters in order (put) -- one that only counts gives the length without a buffer.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ISSL_HD __host__ __device__ __forceinline__
#else
#define ISSL_HD inline
#endif

namespace issl {

constexpr int kReprPow10Min = -292, kReprPow10Max = 324; // the table's range (checked against repr_tables.inc where it is included)
constexpr uint32_t kReprMax = 24;                          // "-2.2250738585072014e-308"
typedef const unsigned long long (*ReprTable)[2];

struct U128 {
    uint64_t hi, lo;
};

ISSL_HD U128 mul_64x64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return U128{__umul64hi(a, b), a * b};
#else
    const unsigned __int128 p = static_cast<unsigned __int128>(a) * b;
    return U128{static_cast<uint64_t>(p >> 64), static_cast<uint64_t>(p)};
#endif
}

// floor(log2(10^e)), |e| <= 1233; floor(log10(2^e)) and floor(log10(3/4 * 2^e)), |e| <= 1500 (arithmetic shifts: floors)
ISSL_HD int32_t floor_log2_pow10(int32_t e) { return (e * 1741647) >> 19; }
ISSL_HD int32_t floor_log10_pow2(int32_t e) { return (e * 1262611) >> 22; }
ISSL_HD int32_t floor_log10_three_quarters_pow2(int32_t e) { return (e * 1262611 - 524031) >> 22; }

// The upper 64 bits of g * cp (g: 128 bits, cp < 2^62 here), with bit 0 set when anything below them is.
ISSL_HD uint64_t round_to_odd(uint64_t g_hi, uint64_t g_lo, uint64_t cp)
{
    const U128 x = mul_64x64(g_lo, cp);
    const U128 y = mul_64x64(g_hi, cp);
    const uint64_t y0 = y.lo + x.hi;
    const uint64_t y1 = y.hi + (y0 < x.hi ? 1u : 0u);
    return y1 | (y0 > 1u ? 1u : 0u);
}

struct Shortest {
    uint64_t digits; // 1 .. 17 significant digits, may end in zeros
    int32_t exp10;   // value = digits * 10^exp10
};

// frac: the 52 stored bits, bexp: the 11 exponent bits (0 .. 2046), not both zero.
ISSL_HD Shortest shortest_digits(uint64_t frac, uint32_t bexp, ReprTable tab)
{
    uint64_t c;
    int32_t q;
    if (bexp != 0) {
        c = frac | (1ull << 52);
        q = static_cast<int32_t>(bexp) - 1075;
    } else {
        c = frac;
        q = -1074;
    }
    const bool even = (c & 1u) == 0;
    const bool lower_closer = frac == 0 && bexp > 1; // the lower neighbour is half as far away
    const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1u : 0u), cb = 4 * c, cbr = 4 * c + 2;
    const int32_t k = lower_closer ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
    const int32_t h = q + floor_log2_pow10(-k) + 1; // 1 .. 4
    const uint64_t g_hi = tab[-k - kReprPow10Min][0], g_lo = tab[-k - kReprPow10Min][1];
    const uint64_t vbl = round_to_odd(g_hi, g_lo, cbl << h);
    const uint64_t vb = round_to_odd(g_hi, g_lo, cb << h);
    const uint64_t vbr = round_to_odd(g_hi, g_lo, cbr << h);
    const uint64_t lower = vbl + (even ? 0u : 1u), upper = vbr - (even ? 0u : 1u); // an even c's interval is closed
    const uint64_t s = vb / 4;
    if (s >= 10) { // one digit less?
        const uint64_t sp = s / 10;
        const bool up_inside = lower <= 40 * sp, wp_inside = 40 * sp + 40 <= upper;
        if (up_inside != wp_inside) return Shortest{sp + (wp_inside ? 1u : 0u), k + 1};
    }
    const bool u_inside = lower <= 4 * s, w_inside = 4 * s + 4 <= upper;
    if (u_inside != w_inside) return Shortest{s + (w_inside ? 1u : 0u), k};
    const uint64_t mid = 4 * s + 2; // both or neither inside: the closer one, ties to even
    const bool up = vb > mid || (vb == mid && (s & 1u) != 0);
    return Shortest{s + (up ? 1u : 0u), k};
}

// The decimal digits of a number below 10^20, four bits each, least significant first (a: digits 0 .. 15, b: 16 .. 19).
struct Digits {
    uint64_t a = 0;
    uint32_t b = 0, n = 0;
    ISSL_HD uint32_t from_top(uint32_t i) const // digit i counted from the most significant one
    {
        const uint32_t at = n - 1 - i;
        return at < 16 ? static_cast<uint32_t>(a >> (4 * at)) & 15u : (b >> (4 * (at - 16))) & 15u;
    }
};

ISSL_HD uint64_t nibbles8(uint32_t v) // eight decimal digits of v < 10^8
{
    uint64_t out = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        out |= static_cast<uint64_t>(v % 10u) << (4 * i);
        v /= 10u;
    }
    return out;
}

ISSL_HD Digits make_digits(uint64_t v)
{
    Digits d;
    const uint64_t top = v / 100000000ull;
    const uint32_t p0 = static_cast<uint32_t>(v - top * 100000000ull);
    const uint32_t p2 = static_cast<uint32_t>(top / 100000000ull);                       // < 1845
    const uint32_t p1 = static_cast<uint32_t>(top - static_cast<uint64_t>(p2) * 100000000ull);
    d.a = nibbles8(p0) | nibbles8(p1) << 32;
    d.b = static_cast<uint32_t>(nibbles8(p2));
    // the number of digits: the highest nibble set, one digit for zero
    if (d.b) d.n = 16 + (35 - __builtin_clz(d.b)) / 4;
    else if (d.a) d.n = (67 - __builtin_clzll(d.a)) / 4;
    else d.n = 1;
    return d;
}

template <class Sink> ISSL_HD void put_u64(Sink &s, uint64_t v)
{
    const Digits d = make_digits(v);
    for (uint32_t i = 0; i < d.n; ++i) s.put(static_cast<char>('0' + d.from_top(i)));
}

// repr(v).
template <class Sink> ISSL_HD void put_repr(Sink &s, double v, ReprTable tab)
{
    uint64_t bits;
    memcpy(&bits, &v, 8);
    const uint32_t bexp = static_cast<uint32_t>(bits >> 52) & 0x7FFu;
    const uint64_t frac = bits & ((1ull << 52) - 1ull);
    if (bexp == 0x7FFu && frac != 0) { // every NaN prints without a sign
        s.put('n'); s.put('a'); s.put('n');
        return;
    }
    if (bits >> 63) s.put('-');
    if (bexp == 0x7FFu) {
        s.put('i'); s.put('n'); s.put('f');
        return;
    }
    if (bexp == 0 && frac == 0) {
        s.put('0'); s.put('.'); s.put('0');
        return;
    }
    Shortest sd = shortest_digits(frac, bexp, tab);
    while (sd.digits % 10u == 0) { // (at most 16 times: 17 digits, not zero)
        sd.digits /= 10u;
        ++sd.exp10;
    }
    const Digits d = make_digits(sd.digits);
    const int32_t n = static_cast<int32_t>(d.n), decpt = n + sd.exp10; // the point stands behind digit decpt
    if (decpt > -4 && decpt <= 16) { // 1e-4 <= |v| < 1e16: fixed notation
        if (decpt <= 0) {
            s.put('0'); s.put('.');
            for (int32_t i = decpt; i < 0; ++i) s.put('0');
            for (int32_t i = 0; i < n; ++i) s.put(static_cast<char>('0' + d.from_top(i)));
        } else {
            for (int32_t i = 0; i < decpt; ++i) s.put(i < n ? static_cast<char>('0' + d.from_top(i)) : '0');
            s.put('.');
            if (decpt >= n) s.put('0');
            for (int32_t i = decpt; i < n; ++i) s.put(static_cast<char>('0' + d.from_top(i)));
        }
        return;
    }
    s.put(static_cast<char>('0' + d.from_top(0)));
    if (n > 1) {
        s.put('.');
        for (int32_t i = 1; i < n; ++i) s.put(static_cast<char>('0' + d.from_top(i)));
    }
    s.put('e');
    int32_t e = decpt - 1;
    s.put(e < 0 ? '-' : '+');
    if (e < 0) e = -e;
    if (e >= 100) s.put(static_cast<char>('0' + e / 100));
    s.put(static_cast<char>('0' + (e / 10) % 10));
    s.put(static_cast<char>('0' + e % 10));
}

// Sinks: into memory, and the length alone.
struct WriteSink {
    char *p;
    ISSL_HD void put(char c) { *p++ = c; }
};
struct CountSink {
    uint64_t n = 0;
    ISSL_HD void put(char) { ++n; }
};

// round(x * 10^6), ties to even, on the exact binary value: what printf("%f") prints of a finite x with 0 <= x < 2^32,
// without the point (issl_text.cpp, format_f6).  x = m * 2^-s, so x * 10^6 = m * 10^6 / 2^s: one 128-bit product.
ISSL_HD uint64_t round_micro(double x)
{
    uint64_t bits;
    memcpy(&bits, &x, 8);
    const uint32_t e = static_cast<uint32_t>(bits >> 52) & 0x7FFu;
    const uint64_t frac = bits & ((1ull << 52) - 1ull);
    if (e == 0 && frac == 0) return 0;
    const uint64_t m = e ? (frac | (1ull << 52)) : frac;
    const uint32_t sh = e ? 1075u - e : 1074u; // >= 21 below 2^32
    if (sh >= 75) return 0;                    // m * 10^6 < 2^73 <= 2^(sh - 2): below half of the last place
    const U128 p = mul_64x64(m, 1000000u);
    uint64_t q, rem_hi, rem_lo, half_hi, half_lo;
    if (sh >= 64) {
        q = p.hi >> (sh - 64);
        rem_hi = p.hi & ((1ull << (sh - 64)) - 1ull);
        rem_lo = p.lo;
        half_hi = sh > 64 ? 1ull << (sh - 65) : 0;
        half_lo = sh > 64 ? 0 : 1ull << 63;
    } else {
        q = p.hi << (64 - sh) | p.lo >> sh;
        rem_hi = 0;
        rem_lo = p.lo & ((1ull << sh) - 1ull);
        half_hi = 0;
        half_lo = 1ull << (sh - 1);
    }
    const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
    const bool tie = rem_hi == half_hi && rem_lo == half_lo;
    if (above || (tie && (q & 1u))) ++q;
    return q;
}

// What Crackling holds after reading a score back from the scorer's "%f" text (Crackling.py:785-786): float() of the six
// decimals.  Exact for 0 <= x < 2^32 (the scorer's range is 0 .. 100): round_micro(x) / 10^6 in one IEEE division.  A
// value outside that range, a negative one and a NaN are passed through as they are.
ISSL_HD double through_text(double x)
{
    if (!(x >= 0.0 && x < 4294967296.0)) return x;
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(static_cast<double>(round_micro(x)), 1000000.0);
#else
    return static_cast<double>(round_micro(x)) / 1000000.0;
#endif
}

} // namespace issl
