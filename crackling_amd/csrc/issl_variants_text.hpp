// The text side of the variant-aware genome search (issl_genome_search_variants*, issl_vcf_snps, issl_genome_apply_snps;
// include/issl_hip.h), beside issl_search_text.hpp and in its style: host code that g++ alone compiles, no HIP and no
// library call.  The library (issl_variants.hip), the executable (cli_search.cpp) and tools/variants_sanitize.cpp (a CPU
// program under AddressSanitizer + UBSan) include the same header, and the plane arithmetic that the kernels do lives here
// as host and device code, so that the CPU program checks the very functions the kernels call against character loops.
//
// Bit planes: a stretch of up to 32 text positions is four 32-bit words, one per base of A C G T; plane b bit i is set
// when base b is in the set S(text[i]) its IUPAC code stands for.  This is issl_search_pattern.allow's convention, so the
// pattern is four planes as it comes.  L = 32 uses all 32 bits of a plane: nothing here shifts by 32.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "issl_search_text.hpp"

namespace issl {
namespace variants_text {

using search_text::low_bits32;

struct Planes { uint32_t p[4]; };

// The pattern and the limits as the kernels use them: by value in the kernel arguments.
struct VariantArgs {
    uint32_t allow[4];    // issl_search_pattern.allow
    uint32_t allow_rc[4]; // the pattern as strand 1 meets the FORWARD window: allow_rc[b] bit j = allow[3 - b] bit L-1-j
    uint32_t win_mask;    // the low L bits
    uint32_t length;
    uint32_t rev_shift;   // 32 - L (0 for 32 bases)
    uint32_t max_dist;
    uint32_t need;        // L - max_dist: a hit has at least this many matching positions
    uint32_t max_variants;
};

// ---- text byte <-> set ---------------------------------------------------------------------------------------------

// Upper-case text byte -> the set of one of the 14 codes A C G T R Y S W K M B D H V (bit b = base b of A C G T); 0 for
// N, for the record separator and for any other byte: such a position disqualifies its windows.  A nibble per letter,
// 'A'..'P' in one word and 'Q'..'Z' in the other.
ISSL_ST_HD uint32_t text_set(uint8_t c)
{
    const uint32_t i = static_cast<uint32_t>(c) - 'A';
    if (i > 25u) return 0;
    const uint64_t tab = i < 16u ? 0x00030C00B400D2E1ull : 0x0000000A09708650ull;
    return static_cast<uint32_t>(tab >> (4 * (i & 15u))) & 15u;
}

// Set 1..15 -> its IUPAC letter (15 is N, which no text position of a window holds); 0 -> '?'.
// ("?ACMGRSV" and "TWYHKDBN" as the bytes of two words.)
ISSL_ST_HD char set_letter(uint32_t set)
{
    const uint64_t tab = (set & 8u) ? 0x4E42444B48595754ull : 0x565352474D43413Full;
    return static_cast<char>(tab >> (8 * (set & 7u)));
}

// The set of position i.
ISSL_ST_HD uint32_t set_at(const Planes &t, uint32_t i)
{
    return (t.p[0] >> i & 1u) | (t.p[1] >> i & 1u) << 1 | (t.p[2] >> i & 1u) << 2 | (t.p[3] >> i & 1u) << 3;
}

// ---- planes ---------------------------------------------------------------------------------------------------------

// 32 bits that start s (0..31) bits into lo, out of two neighbouring words (v_alignbit_b32 on the device).
ISSL_ST_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (s & 31u));
#endif
}

ISSL_ST_HD uint32_t reverse_bits32(uint32_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
#endif
}

// What strand 1 reads of a window of L positions (zeros above them): T[i] = comp(S(w[L-1-i])), so plane b is the
// bit-reversed plane 3 - b, shifted down by 32 - L.
ISSL_ST_HD Planes strand1(const Planes &w, uint32_t rev_shift)
{
    return {{reverse_bits32(w.p[3]) >> rev_shift, reverse_bits32(w.p[2]) >> rev_shift, reverse_bits32(w.p[1]) >> rev_shift,
             reverse_bits32(w.p[0]) >> rev_shift}};
}

// The positions whose set holds more than one base.
ISSL_ST_HD uint32_t ambiguous(const Planes &w)
{
    const uint32_t ac = w.p[0] | w.p[1];
    return (w.p[0] & w.p[1]) | (ac & w.p[2]) | ((ac | w.p[2]) & w.p[3]);
}

// A[i] = T[i] & allowed(pattern[i]), plane by plane.
ISSL_ST_HD Planes intersect(const Planes &t, const uint32_t *allow)
{
    return {{t.p[0] & allow[0], t.p[1] & allow[1], t.p[2] & allow[2], t.p[3] & allow[3]}};
}

// Every A[i] is non-empty.  With allow_rc on the forward window this is strand 1's test without reversing the window.
ISSL_ST_HD bool admits(const Planes &t, const uint32_t *allow, uint32_t win_mask)
{
    return ((t.p[0] & allow[0]) | (t.p[1] & allow[1]) | (t.p[2] & allow[2]) | (t.p[3] & allow[3])) == win_mask;
}

// The positions that match: q[i] is N or in A[i] (q: the query's planes, a compared position in its base's plane alone,
// an N position in all four).  The hot comparison of k_variants: four ANDs ORed together, five instructions as the
// compiler folds them (v_and_or_b32, v_or3_b32), for all 32 positions.
ISSL_ST_HD uint32_t matches(const Planes &a, const Planes &q)
{
    return (a.p[0] & q.p[0]) | (a.p[1] & q.p[1]) | (a.p[2] & q.p[2]) | (a.p[3] & q.p[3]);
}

// The positions that do not match; the distance is their number.
ISSL_ST_HD uint32_t mismatches(const Planes &a, const Planes &q, uint32_t win_mask) { return ~matches(a, q) & win_mask; }

// A query of the public type (2-bit sig + care) as planes.
ISSL_ST_HD Planes query_planes(uint64_t sig, uint64_t care, uint32_t win_mask)
{
    const uint32_t lo = search_text::gather_even_bits(sig), hi = search_text::gather_even_bits(sig >> 1);
    const uint32_t free_ = ~search_text::gather_even_bits(care) & win_mask;
    return {{(~lo & ~hi & win_mask) | free_, (lo & ~hi & win_mask) | free_, (~lo & hi & win_mask) | free_, (lo & hi & win_mask) | free_}};
}

inline VariantArgs make_args(const issl_search_pattern &pat, int max_dist, int max_variants)
{
    VariantArgs a{};
    a.length = pat.length;
    a.win_mask = low_bits32(pat.length);
    a.rev_shift = 32 - pat.length;
    for (uint32_t b = 0; b < 4; ++b) {
        a.allow[b] = pat.allow[b];
        a.allow_rc[b] = reverse_bits32(pat.allow[3 - b]) >> a.rev_shift;
    }
    a.max_dist = static_cast<uint32_t>(max_dist);
    a.need = pat.length - a.max_dist;
    a.max_variants = static_cast<uint32_t>(max_variants);
    return a;
}

inline bool check_max_variants(const issl_search_pattern *pat, int max_variants, std::string &err)
{
    if (max_variants >= 0 && static_cast<uint32_t>(max_variants) <= pat->length) return true;
    err = "max_variants " + std::to_string(max_variants) + ": 0 to the pattern's length " + std::to_string(pat->length);
    return false;
}

// One row from the window's characters w[0..L) (upper case): what the finish pass does per row and a CPU checker per
// window.  false: the window holds a byte that is none of the 14 codes.  The caller compares n_var and dist with its limits.
struct RowFields { Planes site; uint32_t mism, dist, n_var; bool admitted; };
ISSL_ST_HD bool window_row(const uint8_t *w, const VariantArgs &a, uint32_t strand, uint64_t sig, uint64_t care, RowFields &out)
{
    Planes f{{0, 0, 0, 0}};
    for (uint32_t i = 0; i < a.length; ++i) {
        const uint32_t set = text_set(w[i]);
        if (!set) return false;
        for (uint32_t b = 0; b < 4; ++b) f.p[b] |= (set >> b & 1u) << i;
    }
    out.n_var = static_cast<uint32_t>(__builtin_popcount(ambiguous(f)));
    out.site = strand ? strand1(f, a.rev_shift) : f;
    out.admitted = admits(out.site, a.allow, a.win_mask);
    out.mism = mismatches(intersect(out.site, a.allow), query_planes(sig, care, a.win_mask), a.win_mask);
    out.dist = static_cast<uint32_t>(__builtin_popcount(out.mism));
    return true;
}

// ---- SNPs -----------------------------------------------------------------------------------------------------------

// One place of the text after the host's merge: what the check and the apply kernel take.
struct SnpPlace {
    uint64_t at;    // position in the handle's text
    uint32_t index; // the smallest input index of the place's entries
    uint8_t ref, alt, pad[2];
};

// A blank as a record's name ends at one: what Python's bytes.split() splits at.
inline bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// Ranges, sort by (record, pos), merge.  starts[r], lengths[r]: where record r lies in the text.  false + message.
inline bool merge_snps(const issl_snp *snps, size_t n, const uint64_t *starts, const uint64_t *lengths, size_t n_records,
                       std::vector<SnpPlace> &places, std::string &err)
{
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) {
        const issl_snp &s = snps[k];
        const char *bad = s.record >= n_records ? "its record is out of range"
                          : s.pos >= lengths[s.record] ? "its position lies beyond the record"
                          : (s.ref != 1 && s.ref != 2 && s.ref != 4 && s.ref != 8) ? "ref is not one base (1, 2, 4 or 8)"
                          : (s.alt == 0 || s.alt > 15) ? "alt is not a non-empty set of A C G T" : nullptr;
        if (bad) {
            err = "snp " + std::to_string(k) + ": " + bad;
            return false;
        }
        order[k] = k;
    }
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        if (snps[x].record != snps[y].record) return snps[x].record < snps[y].record;
        if (snps[x].pos != snps[y].pos) return snps[x].pos < snps[y].pos;
        return x < y;
    });
    places.clear();
    for (size_t j = 0; j < n; ++j) {
        const issl_snp &s = snps[order[j]];
        const uint64_t at = starts[s.record] + s.pos;
        if (!places.empty() && places.back().at == at) {
            if (places.back().ref != s.ref) {
                err = "snp " + std::to_string(order[j]) + ": its ref differs from that of snp " + std::to_string(places.back().index) +
                      " at the same place";
                return false;
            }
            places.back().alt |= s.alt;
            continue;
        }
        places.push_back({at, static_cast<uint32_t>(order[j]), s.ref, s.alt, {0, 0}});
    }
    return true;
}

// One base of ACGT, either case -> its bit; 0 for anything else.
inline uint8_t allele_bit(const char *p, size_t len)
{
    if (len != 1) return 0;
    const uint32_t c = search_text::query_code(p[0]);
    return c < 4 ? static_cast<uint8_t>(1u << c) : 0;
}

// A record's name up to its first blank -> its number (the first record of a name keeps it): what CHROM is looked up in.
using RecordNames = std::unordered_map<std::string, uint32_t>;
inline RecordNames record_names(const char *const *names, const size_t *name_lens, size_t n_records)
{
    RecordNames by_name;
    for (size_t r = 0; r < n_records; ++r) {
        size_t e = 0;
        while (e < name_lens[r] && !is_blank(names[r][e])) ++e;
        by_name.emplace(std::string(names[r], e), static_cast<uint32_t>(r));
    }
    return by_name;
}

// One data line of a VCF: where its first five fields lie in the text, and POS (huge: it does not fit 64 bits).
struct VcfLine {
    size_t f_at[5], f_len[5];
    uint64_t pos;
    bool huge;
};

// The line splitter of the VCF readers (read_vcf here, read_vcf_indels of issl_haplotypes_text.hpp): the next data line from
// p on, empty lines and '#' lines skipped, p and line_no moved behind it.  1: a line; 0: the text's end; -1 + message: a
// malformed line, named.
inline int next_vcf_line(const char *vcf, size_t len, size_t &p, size_t &line_no, VcfLine &out, std::string &err)
{
    while (p < len) {
        const char *nl = static_cast<const char *>(std::memchr(vcf + p, '\n', len - p));
        size_t e = nl ? static_cast<size_t>(nl - vcf) : len;
        const size_t next = nl ? e + 1 : len;
        if (e > p && vcf[e - 1] == '\r') --e;
        const size_t from = p;
        p = next;
        ++line_no;
        if (e == from || vcf[from] == '#') continue;
        size_t fields = 0;
        for (size_t q = from; fields < 5;) {
            const char *tab = static_cast<const char *>(std::memchr(vcf + q, '\t', e - q));
            const size_t fe = tab ? static_cast<size_t>(tab - vcf) : e;
            out.f_at[fields] = q;
            out.f_len[fields++] = fe - q;
            if (!tab) break;
            q = fe + 1;
        }
        if (fields < 5) {
            err = "VCF line " + std::to_string(line_no) + ": fewer than five tab-separated fields";
            return -1;
        }
        out.pos = 0;
        out.huge = false;
        bool numeric = out.f_len[1] > 0;
        for (size_t i = 0; i < out.f_len[1] && numeric; ++i) {
            const char d = vcf[out.f_at[1] + i];
            if (d < '0' || d > '9') numeric = false;
            else if (out.pos > (0xFFFFFFFFFFFFFFFFull - 9) / 10) out.huge = true;
            else out.pos = out.pos * 10 + static_cast<uint64_t>(d - '0');
        }
        if (!numeric) {
            err = "VCF line " + std::to_string(line_no) + ": POS is not a number";
            return -1;
        }
        return 1;
    }
    return 0;
}

// The record a data line names, counted in c (lines, unknown_chrom, beyond_record: the fields both readers' counts have).
// false: the line is skipped.
template <class Counts>
inline bool vcf_line_record(const char *vcf, const VcfLine &l, const RecordNames &by_name, const uint64_t *lengths, Counts &c, uint32_t &record)
{
    ++c.lines;
    const auto rec = by_name.find(std::string(vcf + l.f_at[0], l.f_len[0]));
    if (rec == by_name.end()) {
        ++c.unknown_chrom;
        return false;
    }
    if (l.huge || l.pos == 0 || l.pos > lengths[rec->second]) {
        ++c.beyond_record;
        return false;
    }
    record = rec->second;
    return true;
}

// The entries and counts of a VCF's text; the rules are in include/issl_hip.h.  false + message (a malformed line, named).
inline bool read_vcf(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                     size_t n_records, std::vector<issl_snp> &found, issl_vcf_counts &c, std::string &err)
{
    const RecordNames by_name = record_names(names, name_lens, n_records);
    c = issl_vcf_counts{};
    found.clear();
    size_t line_no = 0, p = 0;
    VcfLine l;
    for (int got; (got = next_vcf_line(vcf, len, p, line_no, l, err)) != 0;) {
        if (got < 0) return false;
        uint32_t record = 0;
        if (!vcf_line_record(vcf, l, by_name, lengths, c, record)) continue;
        const size_t *f_at = l.f_at, *f_len = l.f_len;
        const uint8_t ref = allele_bit(vcf + f_at[3], f_len[3]);
        uint8_t alt = 0;
        for (size_t q = f_at[4], end = f_at[4] + f_len[4];;) {
            const char *comma = static_cast<const char *>(std::memchr(vcf + q, ',', end - q));
            const size_t ae = comma ? static_cast<size_t>(comma - vcf) : end;
            const uint8_t bit = ref ? allele_bit(vcf + q, ae - q) : 0;
            if (bit) alt |= bit;
            else ++c.alleles_skipped;
            if (!comma) break;
            q = ae + 1;
        }
        if (!alt) {
            ++c.no_allele;
            continue;
        }
        issl_snp s{};
        s.pos = l.pos - 1;
        s.record = record;
        s.ref = ref;
        s.alt = alt;
        found.push_back(s);
    }
    c.snps = found.size();
    return true;
}

// issl_vcf_snps without the library around it.  out may be NULL with cap == 0; *n is always complete, nothing is written
// when *n > cap.
inline bool vcf_snps(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                     size_t n_records, issl_snp *out, size_t cap, size_t *n, issl_vcf_counts *counts, std::string &err)
{
    std::vector<issl_snp> found;
    issl_vcf_counts c{};
    if (!read_vcf(vcf, len, names, name_lens, lengths, n_records, found, c, err)) return false;
    *n = found.size();
    if (counts) *counts = c;
    if (out && found.size() <= cap && !found.empty()) std::memcpy(out, found.data(), sizeof(issl_snp) * found.size());
    return true;
}

// ---- the lines of bin/isslSearchGenome --variants --------------------------------------------------------------------

// "<query text>\t<record name>\t<pos>\t<+|->\t<dist>\t<site>\n": the site in IUPAC letters, lower case where mism is set.
inline void append_variant_line(std::string &out, const char *query, uint32_t length, const char *name, size_t name_len,
                                const issl_variant_hit &h)
{
    out.append(query, length);
    out += '\t';
    out.append(name, name_len);
    char buf[64];
    std::snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t", static_cast<unsigned long long>(h.pos), h.strand ? '-' : '+',
                  static_cast<unsigned>(h.dist));
    out += buf;
    const Planes t{{h.site[0], h.site[1], h.site[2], h.site[3]}};
    for (uint32_t i = 0; i < length; ++i) {
        const char c = set_letter(set_at(t, i));
        out += (h.mism >> i & 1u) && c != '?' ? static_cast<char>(c - 'A' + 'a') : c;
    }
    out += '\n';
}

} // namespace variants_text
} // namespace issl
