// The text side of the search on the ALT haplotypes of indels (issl_vcf_indels, issl_haplotypes_*; include/issl_hip.h),
// beside issl_variants_text.hpp and in its style: host code that g++ alone compiles, no HIP and no library call.  The
// library (issl_haplotypes.hip), the executable (cli_search.cpp) and tools/haplotypes_sanitize.cpp (a CPU program under
// AddressSanitizer + UBSan) include the same header, and what the kernels do per byte and per row -- is a REF base in the
// set of its text byte, which byte is byte i of a strip, which reference position has a window of a strip -- lives here as
// host and device code, so that the CPU program checks the very functions the kernels call against character loops.
//
// A strip: for a window length W, the min(W - 1, p) text bytes ahead of the trimmed edit (p, REF', ALT'), then ALT', then
// the min(W - 1, length - p - |REF'|) text bytes behind REF', then '\n'.  Its windows of W bytes are exactly the windows of
// the record's ALT haplotype that overlap the edit.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "issl_variants_text.hpp"

namespace issl {
namespace haplotypes_text {

namespace vt = variants_text;

// ---- the trim --------------------------------------------------------------------------------------------------------

// Two bytes over ACGT in either case are the same base.
ISSL_ST_HD bool same_base(uint8_t a, uint8_t b) { return ((a ^ b) & 0xDFu) == 0; }

// A byte of ACGT in either case -> 0..3; 4 for any other byte.
ISSL_ST_HD uint32_t base_code(uint8_t c)
{
    const uint8_t u = c & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}
ISSL_ST_HD bool is_base(uint8_t c) { return base_code(c) < 4; }

// (p, REF', ALT') of include/issl_hip.h: REF' = ref[prefix .. prefix + ref_len), ALT' = alt[prefix .. prefix + alt_len).
struct Trimmed { uint32_t prefix, ref_len, alt_len; };
ISSL_ST_HD Trimmed trim(const uint8_t *ref, uint32_t ref_len, const uint8_t *alt, uint32_t alt_len)
{
    while (ref_len && alt_len && same_base(ref[ref_len - 1], alt[alt_len - 1])) --ref_len, --alt_len; // the common suffix first
    uint32_t prefix = 0;
    while (prefix < ref_len && prefix < alt_len && same_base(ref[prefix], alt[prefix])) ++prefix;
    return {prefix, ref_len - prefix, alt_len - prefix};
}

// ---- the layout ------------------------------------------------------------------------------------------------------

// The table entry beside the strip text: what maps a row of the strip search back to the reference.
struct Strip {
    uint64_t p;       // 0-based inside the record, of the trimmed edit
    uint32_t record;  // the reference record
    uint32_t left;    // bytes of the strip ahead of ALT'
    uint32_t alt_len; // |ALT'|
    uint32_t ref_len; // |REF'|
    uint32_t reserved[2];
};

// Where the bytes of strip k come from and go to: what the build kernel takes beside Strip.
struct StripSource {
    uint64_t from_left;  // position in the handle's text of the strip's first byte (left > 0)
    uint64_t from_right; // position in the handle's text of the first byte behind REF' (right > 0)
    uint64_t to;         // position of the strip in the strip text
    uint32_t alt_at;     // where ALT' starts in the allele text
    uint32_t right;      // bytes of the strip behind ALT'
};

// The untrimmed REF of entry k against the text: what the check kernel takes.
struct RefPlace {
    uint64_t at;     // position in the handle's text of the first REF base
    uint32_t ref_at; // where REF starts in the allele text
    uint32_t ref_len;
};

static_assert(sizeof(issl_indel) == 32 && sizeof(issl_vcf_indel_counts) == 56 && sizeof(issl_haplotype_hit) == 48 &&
                  sizeof(Strip) == 32 && sizeof(StripSource) == 32 && sizeof(RefPlace) == 16,
              "the layouts of include/issl_hip.h");

ISSL_ST_HD uint32_t strip_length(const Strip &t, const StripSource &f) { return t.left + t.alt_len + f.right; } // without the separator

// Byte i of a strip, the separator at i == strip_length: what a lane of the build kernel writes.  alleles is upper case.
ISSL_ST_HD uint8_t strip_byte(const uint8_t *text, const uint8_t *alleles, const Strip &t, const StripSource &f, uint32_t i)
{
    if (i < t.left) return text[f.from_left + i];
    i -= t.left;
    if (i < t.alt_len) return alleles[f.alt_at + i];
    i -= t.alt_len;
    return i < f.right ? text[f.from_right + i] : static_cast<uint8_t>('\n');
}

// REF base `base` (upper case ACGT) lies in the set of text byte c: the REF check, per byte.
ISSL_ST_HD bool ref_in_text(uint8_t c, uint8_t base)
{
    const uint32_t code = base_code(base);
    return code < 4 && (vt::text_set(c) >> code & 1u);
}

// The window that starts s bytes into its strip: the reference position of its first base and edit_at (include/issl_hip.h).
ISSL_ST_HD void strip_row(const Strip &t, uint64_t s, uint64_t &pos, int32_t &edit_at)
{
    edit_at = static_cast<int32_t>(static_cast<int64_t>(t.left) - static_cast<int64_t>(s));
    if (s < t.left) pos = t.p - t.left + s;
    else if (s < static_cast<uint64_t>(t.left) + t.alt_len) pos = t.p;
    else pos = t.p + t.ref_len + (s - t.left - t.alt_len);
}

// The host's checks and the layout of issl_haplotypes_open.  rec_starts[r], lengths[r]: where record r lies in the handle's
// text.  upper: the allele text in upper case (what goes to the device); starts[k]: where strip k lies in the strip text of
// text_len bytes.  false + message naming the entry.
inline bool plan_strips(const issl_indel *indels, size_t n, const char *alleles, size_t alleles_len, const uint64_t *rec_starts,
                        const uint64_t *lengths, size_t n_records, uint32_t window, std::vector<Strip> &strips,
                        std::vector<StripSource> &sources, std::vector<RefPlace> &places, std::vector<uint64_t> &starts,
                        uint64_t &text_len, std::string &upper, std::string &err)
{
    upper.assign(alleles_len ? alleles : "", alleles_len);
    for (char &c : upper)
        if (c >= 'a' && c <= 'z') c = static_cast<char>(c - 'a' + 'A');
    strips.assign(n, Strip{});
    sources.assign(n, StripSource{});
    places.assign(n, RefPlace{});
    starts.assign(n, 0);
    text_len = 0;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(upper.data());
    for (size_t k = 0; k < n; ++k) {
        const issl_indel &d = indels[k];
        auto outside = [&](uint32_t at, uint32_t len) { return at > alleles_len || len > alleles_len - at; };
        auto bases = [&](uint32_t at, uint32_t len) {
            for (uint32_t i = 0; i < len; ++i)
                if (!is_base(bytes[at + i])) return false;
            return true;
        };
        const char *bad = d.record >= n_records ? "its record is out of range"
                          : (d.ref_len == 0 || d.alt_len == 0) ? "ref_len and alt_len are at least 1"
                          : (d.ref_len > ISSL_INDEL_MAX_ALLELE || d.alt_len > ISSL_INDEL_MAX_ALLELE) ? "an allele is longer than ISSL_INDEL_MAX_ALLELE"
                          : (d.pos > lengths[d.record] || d.ref_len > lengths[d.record] - d.pos) ? "pos + ref_len lies beyond the record"
                          : (outside(d.ref_at, d.ref_len) || outside(d.alt_at, d.alt_len)) ? "its bases lie outside the allele text"
                          : (!bases(d.ref_at, d.ref_len) || !bases(d.alt_at, d.alt_len)) ? "its bases are not all of ACGT" : nullptr;
        if (bad) {
            err = "indel " + std::to_string(k) + ": " + bad;
            return false;
        }
        const Trimmed t = trim(bytes + d.ref_at, d.ref_len, bytes + d.alt_at, d.alt_len);
        if (t.ref_len == 0 && t.alt_len == 0) {
            err = "indel " + std::to_string(k) + ": REF and ALT are the same, it changes nothing";
            return false;
        }
        Strip &s = strips[k];
        StripSource &f = sources[k];
        s.p = d.pos + t.prefix;
        s.record = d.record;
        s.left = static_cast<uint32_t>(std::min<uint64_t>(window - 1, s.p));
        s.alt_len = t.alt_len;
        s.ref_len = t.ref_len;
        f.right = static_cast<uint32_t>(std::min<uint64_t>(window - 1, lengths[d.record] - s.p - t.ref_len));
        f.from_left = rec_starts[d.record] + s.p - s.left;
        f.from_right = rec_starts[d.record] + s.p + t.ref_len;
        f.alt_at = d.alt_at + t.prefix;
        f.to = starts[k] = text_len;
        text_len += strip_length(s, f) + 1ull;
        places[k] = {rec_starts[d.record] + d.pos, d.ref_at, d.ref_len};
    }
    return true;
}

// ---- the VCF reader --------------------------------------------------------------------------------------------------

// The indels and counts of a VCF's text; the rules are in include/issl_hip.h.  alleles: REF then ALT of every entry, as the
// bytes stand in the file.  false + message (a malformed line, named; more allele text than 32-bit offsets reach).
inline bool read_vcf_indels(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                            size_t n_records, std::vector<issl_indel> &found, std::string &alleles, issl_vcf_indel_counts &c,
                            std::string &err)
{
    const vt::RecordNames by_name = vt::record_names(names, name_lens, n_records);
    c = issl_vcf_indel_counts{};
    found.clear();
    alleles.clear();
    size_t line_no = 0, p = 0;
    vt::VcfLine l;
    auto all_bases = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!is_base(static_cast<uint8_t>(vcf[at + i]))) return false;
        return n > 0;
    };
    for (int got; (got = vt::next_vcf_line(vcf, len, p, line_no, l, err)) != 0;) {
        if (got < 0) return false;
        uint32_t record = 0;
        if (!vt::vcf_line_record(vcf, l, by_name, lengths, c, record)) continue;
        const size_t ref_at = l.f_at[3], ref_len = l.f_len[3];
        const bool ref_ok = all_bases(ref_at, ref_len);
        if (ref_ok && ref_len > lengths[record] - (l.pos - 1)) {
            ++c.beyond_record;
            continue;
        }
        bool gave = false;
        for (size_t q = l.f_at[4], end = l.f_at[4] + l.f_len[4];;) {
            const char *comma = static_cast<const char *>(std::memchr(vcf + q, ',', end - q));
            const size_t ae = comma ? static_cast<size_t>(comma - vcf) : end, alt_len = ae - q;
            bool take = ref_ok && all_bases(q, alt_len) && !(ref_len == 1 && alt_len == 1);
            if (take && alt_len == ref_len) {
                size_t i = 0;
                while (i < ref_len && same_base(static_cast<uint8_t>(vcf[ref_at + i]), static_cast<uint8_t>(vcf[q + i]))) ++i;
                take = i < ref_len;
            }
            if (!take) ++c.alleles_skipped;
            else if (ref_len > ISSL_INDEL_MAX_ALLELE || alt_len > ISSL_INDEL_MAX_ALLELE) ++c.too_long;
            else {
                if (alleles.size() + ref_len + alt_len > 0xFFFFFFFFull) {
                    err = "VCF line " + std::to_string(line_no) + ": more than 2^32 - 1 bytes of allele text";
                    return false;
                }
                issl_indel d{};
                d.pos = l.pos - 1;
                d.record = record;
                d.ref_len = static_cast<uint32_t>(ref_len);
                d.alt_len = static_cast<uint32_t>(alt_len);
                d.ref_at = static_cast<uint32_t>(alleles.size());
                d.alt_at = d.ref_at + d.ref_len;
                alleles.append(vcf + ref_at, ref_len);
                alleles.append(vcf + q, alt_len);
                found.push_back(d);
                gave = true;
            }
            if (!comma) break;
            q = ae + 1;
        }
        if (!gave) ++c.no_allele;
    }
    c.indels = found.size();
    return true;
}

// issl_vcf_indels without the library around it.  out and alleles may be NULL with capacity 0; *n and *alleles_len are
// always complete, nothing is written when either exceeds its capacity.
inline bool vcf_indels(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                       size_t n_records, issl_indel *out, size_t cap, size_t *n, char *alleles, size_t alleles_cap, size_t *alleles_len,
                       issl_vcf_indel_counts *counts, std::string &err)
{
    std::vector<issl_indel> found;
    std::string text;
    issl_vcf_indel_counts c{};
    if (!read_vcf_indels(vcf, len, names, name_lens, lengths, n_records, found, text, c, err)) return false;
    *n = found.size();
    *alleles_len = text.size();
    if (counts) *counts = c;
    if (found.size() > cap || text.size() > alleles_cap) return true;
    if (out && !found.empty()) std::memcpy(out, found.data(), sizeof(issl_indel) * found.size());
    if (alleles && !text.empty()) std::memcpy(alleles, text.data(), text.size());
    return true;
}

// ---- the lines of bin/isslSearchGenome --indel-vcf -------------------------------------------------------------------

// --variants' line followed by "\t<POS 1-based of the trimmed edit>:<REF' or ->><ALT' or ->\t<edit_at>".
inline void append_haplotype_line(std::string &out, const char *query, uint32_t length, const char *name, size_t name_len,
                                  const issl_haplotype_hit &h, const issl_indel &d, const char *alleles)
{
    issl_variant_hit v{};
    v.pos = h.pos;
    std::memcpy(v.site, h.site, sizeof v.site);
    v.mism = h.mism;
    v.strand = h.strand;
    v.dist = h.dist;
    vt::append_variant_line(out, query, length, name, name_len, v);
    out.pop_back(); // (its line end)
    const uint8_t *ref = reinterpret_cast<const uint8_t *>(alleles) + d.ref_at, *alt = reinterpret_cast<const uint8_t *>(alleles) + d.alt_at;
    const Trimmed t = trim(ref, d.ref_len, alt, d.alt_len);
    char buf[32];
    std::snprintf(buf, sizeof buf, "\t%llu:", static_cast<unsigned long long>(d.pos + t.prefix + 1));
    out += buf;
    auto bases = [&](const uint8_t *b, uint32_t n) {
        if (!n) out += '-';
        for (uint32_t i = 0; i < n; ++i) out += static_cast<char>(b[i] >= 'a' ? b[i] - 'a' + 'A' : b[i]);
    };
    bases(ref + t.prefix, t.ref_len);
    out += '>';
    bases(alt + t.prefix, t.alt_len);
    std::snprintf(buf, sizeof buf, "\t%d\n", static_cast<int>(h.edit_at));
    out += buf;
}

} // namespace haplotypes_text
} // namespace issl
