// The text side of the search on the ALT haplotypes of indels (crackling_amd/csrc/issl_haplotypes_text.hpp, the header
// issl_haplotypes.hip and bin/isslSearchGenome include) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
// CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/haplotypes_sanitize.cpp \
//       -o <tmp>/haplotypes_sanitize && <tmp>/haplotypes_sanitize file.vcf <name> <length> [<name> <length> ...]
// First the functions the kernels call against character loops, on random records, edits of every kind (deletions,
// insertions, substitutions, complex alleles, with and without shared bases at either end, at the record's ends) and every
// window length 1..32: trim against strings; plan_strips' layout and strip_byte, byte by byte into an allocation of exactly
// the strip text's size, against the whole-record ALT haplotype -- the windows of a strip are the windows of the haplotype
// that overlap the edit, in order; strip_row against the position of such a window in the reference; ref_in_text against
// the IUPAC table; plan_strips' refusals: "layout ok <windows checked>".  Then the VCF: the file's entries and counts are
// printed ("indel <record> <pos> <REF> <ALT>", "counts ..." or "refused <message>"), and the reader is run on every
// truncation of the file and on 3000 copies with bytes changed, each in an allocation of exactly its size, with both
// capacity rules; what it returns goes through plan_strips: "vcf ok <inputs read>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_haplotypes_text.hpp"

namespace st = issl::search_text;
namespace ht = issl::haplotypes_text;

static void die(const char *what)
{
    std::fprintf(stderr, "haplotypes_sanitize: %s\n", what);
    std::exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

static std::string random_bases(size_t n, const char *codes, uint32_t n_codes)
{
    std::string s(n, 'A');
    for (char &c : s) c = codes[rng() % n_codes];
    return s;
}

static std::string upper(std::string s)
{
    for (char &c : s)
        if (c >= 'a' && c <= 'z') c = static_cast<char>(c - 'a' + 'A');
    return s;
}

// the trim with strings
static void trim_strings(std::string ref, std::string alt, size_t &prefix, std::string &r, std::string &a)
{
    ref = upper(ref), alt = upper(alt);
    while (!ref.empty() && !alt.empty() && ref.back() == alt.back()) ref.pop_back(), alt.pop_back();
    prefix = 0;
    while (prefix < ref.size() && prefix < alt.size() && ref[prefix] == alt[prefix]) ++prefix;
    r = ref.substr(prefix), a = alt.substr(prefix);
}

static void check_tables()
{
    for (uint32_t c = 0; c < 256; ++c) {
        const char ch = static_cast<char>(c);
        const bool base = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'a' || ch == 'c' || ch == 'g' || ch == 't';
        if (ht::is_base(static_cast<uint8_t>(c)) != base) die("is_base");
        for (uint32_t b = 0; b < 4; ++b) {
            uint32_t set = (ch >= 'A' && ch <= 'Z') ? st::iupac_bases(ch) : 0;
            if (set == 15) set = 0; // N is no code of a window
            if (ht::ref_in_text(static_cast<uint8_t>(c), static_cast<uint8_t>("ACGT"[b])) != ((set >> b & 1u) != 0)) die("ref_in_text");
        }
        if (ht::ref_in_text('N', static_cast<uint8_t>(c)) || (ht::ref_in_text('A', static_cast<uint8_t>(c)) != (ch == 'A' || ch == 'a')))
            die("ref_in_text's base");
    }
}

// One random case: a record among three, an edit in it, a window length.  -> windows checked.
static size_t check_layout_case(uint32_t W, int kind)
{
    static const char codes[] = "ACGTRYSWKMBDHV";
    std::vector<std::string> recs = {random_bases(rng() % 5, codes, 14), random_bases(1 + rng() % 70, codes, kind & 1 ? 14 : 2),
                                     random_bases(rng() % 9, codes, 4)};
    std::vector<uint64_t> starts, lengths;
    std::string text;
    for (const std::string &r : recs) {
        starts.push_back(text.size());
        lengths.push_back(r.size());
        text += r;
        text += '\n';
    }
    const std::string &rec = recs[1];
    // REF: 1..6 bases of the record (an ambiguity code there reads as one of its bases: 'A' stands in), ALT: 1..40 bases
    uint64_t pos = rng() % rec.size();
    if (kind == 2) pos = 0;
    uint32_t ref_len = 1 + rng() % std::min<uint32_t>(6, static_cast<uint32_t>(rec.size() - pos));
    if (kind == 3) ref_len = static_cast<uint32_t>(rec.size() - pos); // to the record's end
    if (kind == 4) pos = 0, ref_len = static_cast<uint32_t>(rec.size()); // the whole record
    std::string ref = rec.substr(pos, ref_len);
    for (char &c : ref)
        if (!ht::is_base(static_cast<uint8_t>(c))) c = 'A';
    std::string alt;
    switch (rng() % 5) {
    case 0: alt = ref.substr(0, 1 + rng() % ref.size()); break;                        // a deletion behind an anchor
    case 1: alt = ref + random_bases(1 + rng() % 40, "AC", 2); break;                  // an insertion behind REF
    case 2: alt = random_bases(1 + rng() % 3, "AC", 2) + ref.substr(ref.size() / 2); break; // shares a suffix
    case 3: alt = random_bases(ref.size(), "ACGT", 4); break;                          // a substitution
    default: alt = random_bases(1 + rng() % 40, "ACGT", 4); break;
    }
    if (upper(alt) == upper(ref)) alt += 'G';
    if (rng() & 1) { // either case
        char &c = alt[rng() % alt.size()];
        c = static_cast<char>(c - 'A' + 'a');
    }

    // the allele text in an allocation of exactly its size, with a stranger ahead of the entry
    const std::string lead = "ca";
    const size_t alleles_len = lead.size() + ref.size() + alt.size();
    char *alleles = static_cast<char *>(std::malloc(alleles_len));
    if (!alleles) die("no memory");
    std::memcpy(alleles, lead.data(), lead.size());
    std::memcpy(alleles + lead.size(), ref.data(), ref.size());
    std::memcpy(alleles + lead.size() + ref.size(), alt.data(), alt.size());
    issl_indel d[2] = {};
    d[0].pos = 0, d[0].record = 1, d[0].ref_len = 1, d[0].alt_len = 2, d[0].ref_at = 0, d[0].alt_at = 0; // "c" > "ca": an insertion at 0
    d[1].pos = pos, d[1].record = 1, d[1].ref_len = ref_len, d[1].alt_len = static_cast<uint32_t>(alt.size());
    d[1].ref_at = static_cast<uint32_t>(lead.size()), d[1].alt_at = static_cast<uint32_t>(lead.size() + ref.size());

    std::vector<ht::Strip> strips;
    std::vector<ht::StripSource> sources;
    std::vector<ht::RefPlace> places;
    std::vector<uint64_t> strip_starts;
    uint64_t text_len = 0;
    std::string up, err;
    if (!ht::plan_strips(d, 2, alleles, alleles_len, starts.data(), lengths.data(), 3, W, strips, sources, places, strip_starts, text_len, up, err))
        die(err.c_str());
    if (up != upper(std::string(alleles, alleles_len))) die("the upper-cased allele text");

    size_t prefix;
    std::string r, a;
    trim_strings(ref, alt, prefix, r, a);
    const ht::Trimmed t = ht::trim(reinterpret_cast<const uint8_t *>(ref.data()), ref_len, reinterpret_cast<const uint8_t *>(alt.data()),
                                   static_cast<uint32_t>(alt.size()));
    if (t.prefix != prefix || t.ref_len != r.size() || t.alt_len != a.size()) die("trim");
    const uint64_t p = pos + prefix;
    const ht::Strip &s = strips[1];
    const ht::StripSource &f = sources[1];
    if (s.p != p || s.record != 1 || s.alt_len != a.size() || s.ref_len != r.size() || s.left != std::min<uint64_t>(W - 1, p) ||
        f.right != std::min<uint64_t>(W - 1, rec.size() - p - r.size()) || s.reserved[0] || s.reserved[1])
        die("the layout");
    if (places[1].at != starts[1] + pos || places[1].ref_at != lead.size() || places[1].ref_len != ref_len) die("the REF place");
    if (strip_starts[0] != 0 || strip_starts[1] != ht::strip_length(strips[0], sources[0]) + 1ull || f.to != strip_starts[1] ||
        text_len != strip_starts[1] + ht::strip_length(s, f) + 1ull)
        die("the strip starts");

    // the strips, byte by byte, into exactly their room; the resident text in exactly its room
    uint8_t *resident = static_cast<uint8_t *>(std::malloc(text.size()));
    uint8_t *out = static_cast<uint8_t *>(std::malloc(text_len));
    if (!resident || !out) die("no memory");
    std::memcpy(resident, text.data(), text.size());
    for (size_t k = 0; k < 2; ++k)
        for (uint32_t i = 0; i <= ht::strip_length(strips[k], sources[k]); ++i)
            out[sources[k].to + i] = ht::strip_byte(resident, reinterpret_cast<const uint8_t *>(up.data()), strips[k], sources[k], i);
    const std::string strip(reinterpret_cast<const char *>(out) + f.to, ht::strip_length(s, f));
    if (out[f.to + strip.size()] != '\n' || out[f.to - 1] != '\n') die("the separators");

    // the whole-record ALT haplotype: its windows that overlap the edit are the strip's windows, in order
    const std::string hap = rec.substr(0, p) + upper(a) + rec.substr(p + r.size());
    size_t checked = 0, at = 0;
    for (size_t h = 0; h + W <= hap.size(); ++h) {
        const bool overlaps = a.empty() ? (h < p && h + W > p) : (h < p + a.size() && h + W > p);
        if (!overlaps) continue;
        if (at + W > strip.size() || hap.compare(h, W, strip, at, W) != 0) die("a window of the strip differs from the haplotype's");
        const uint64_t want = h < p ? h : h < p + a.size() ? p : p + r.size() + (h - p - a.size());
        uint64_t got;
        int32_t edit_at;
        ht::strip_row(s, at, got, edit_at);
        if (got != want || edit_at != static_cast<int64_t>(p) - static_cast<int64_t>(h)) die("strip_row");
        ++at, ++checked;
    }
    if (at != (strip.size() >= W ? strip.size() - W + 1 : 0)) die("the strip holds a window the haplotype does not");

    // refusals: each names entry 1
    auto refused = [&](issl_indel bad, size_t len) {
        issl_indel two[2] = {d[0], bad};
        std::string e;
        if (ht::plan_strips(two, 2, alleles, len, starts.data(), lengths.data(), 3, W, strips, sources, places, strip_starts, text_len, up, e))
            die("plan_strips takes a bad entry");
        if (e.compare(0, 9, "indel 1: ") != 0) die("the refusal does not name the entry");
    };
    issl_indel bad = d[1];
    bad.record = 3, refused(bad, alleles_len);
    bad = d[1], bad.pos = rec.size() - ref_len + 1, refused(bad, alleles_len);
    bad = d[1], bad.pos = ~0ull, refused(bad, alleles_len);
    bad = d[1], bad.ref_len = 0, refused(bad, alleles_len);
    bad = d[1], bad.alt_len = ISSL_INDEL_MAX_ALLELE + 1, refused(bad, alleles_len);
    bad = d[1], refused(bad, alleles_len - 1);                    // ALT ends outside the allele text
    bad = d[1], bad.alt_at = 0xFFFFFFFFu, refused(bad, alleles_len);
    bad = d[1], bad.alt_at = bad.ref_at, bad.alt_len = bad.ref_len, refused(bad, alleles_len); // a no-op
    std::free(out);
    std::free(resident);
    std::free(alleles);
    return checked;
}

struct Records {
    std::vector<std::string> names;
    std::vector<const char *> ptrs;
    std::vector<size_t> lens;
    std::vector<uint64_t> lengths, starts;
};

// One run of the reader on bytes copied into an allocation of exactly their size.  -> what it found.
static bool read_exact(const std::string &text, const Records &r, std::vector<issl_indel> &out, std::string &alleles, issl_vcf_indel_counts &counts,
                       std::string &err)
{
    char *exact = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));
    if (!exact) die("no memory");
    std::memcpy(exact, text.data(), text.size());
    size_t n = 0, bytes = 0, n2 = 0, bytes2 = 0;
    auto call = [&](issl_indel *o, size_t cap, char *al, size_t al_cap, size_t *pn, size_t *pb, issl_vcf_indel_counts *c) {
        return ht::vcf_indels(exact, text.size(), r.ptrs.data(), r.lens.data(), r.lengths.data(), r.names.size(), o, cap, pn, al, al_cap, pb, c, err);
    };
    bool ok = call(nullptr, 0, nullptr, 0, &n, &bytes, &counts);
    out.assign(n, issl_indel{});
    alleles.assign(bytes, '\0');
    if (ok) {
        if (n > 0) { // one entry short, then one allele byte short: nothing may be written to either buffer
            std::vector<issl_indel> small(n);
            std::string few(bytes, '\0');
            if (!call(small.data(), n - 1, &few[0], bytes, &n2, &bytes2, nullptr) || n2 != n || bytes2 != bytes) die("the counting rule");
            if (!call(small.data(), n, &few[0], bytes - 1, &n2, &bytes2, nullptr) || n2 != n || bytes2 != bytes) die("the counting rule");
            for (const issl_indel &d : small)
                if (d.pos || d.record || d.ref_len || d.alt_len) die("a short buffer was written");
            for (char c : few)
                if (c) die("a short allele buffer was written");
        }
        ok = call(out.data(), n, bytes ? &alleles[0] : nullptr, bytes, &n2, &bytes2, &counts);
        if (!ok || n2 != n || bytes2 != bytes || counts.indels != n) die("the second call differs");
        size_t at = 0;
        for (const issl_indel &d : out) {
            if (d.record >= r.names.size() || d.ref_len == 0 || d.alt_len == 0 || d.ref_len > ISSL_INDEL_MAX_ALLELE ||
                d.alt_len > ISSL_INDEL_MAX_ALLELE || d.pos + d.ref_len > r.lengths[d.record] || d.ref_at != at || d.alt_at != at + d.ref_len ||
                d.reserved)
                die("an entry out of range");
            at += d.ref_len + d.alt_len;
        }
        if (at != bytes) die("the allele text's length");
        if (counts.lines < counts.no_allele + counts.unknown_chrom + counts.beyond_record) die("the counts do not add up");
        // what the reader gives, the open's host side takes
        std::vector<ht::Strip> strips;
        std::vector<ht::StripSource> sources;
        std::vector<ht::RefPlace> places;
        std::vector<uint64_t> strip_starts;
        uint64_t text_len = 0;
        std::string up, plan_err;
        if (!ht::plan_strips(out.data(), n, alleles.data(), bytes, r.starts.data(), r.lengths.data(), r.names.size(), 23, strips, sources, places,
                             strip_starts, text_len, up, plan_err))
            die(plan_err.c_str());
    }
    std::free(exact);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (argc - 2) % 2) die("usage: haplotypes_sanitize file.vcf <name> <length> ...");
    check_tables();
    size_t windows = 0;
    for (uint32_t W = 1; W <= 32; ++W)
        for (int round = 0; round < 60; ++round) windows += check_layout_case(W, round % 6);
    std::printf("layout ok %zu\n", windows);

    Records r;
    for (int i = 2; i + 1 < argc; i += 2) {
        r.names.push_back(argv[i]);
        r.lengths.push_back(std::strtoull(argv[i + 1], nullptr, 10));
    }
    uint64_t at = 0;
    for (size_t k = 0; k < r.names.size(); ++k) {
        r.ptrs.push_back(r.names[k].data());
        r.lens.push_back(r.names[k].size());
        r.starts.push_back(at);
        at += r.lengths[k] + 1;
    }
    std::string text;
    {
        FILE *fp = std::fopen(argv[1], "rb");
        if (!fp) die("cannot open the VCF");
        char buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
        std::fclose(fp);
    }
    std::vector<issl_indel> indels;
    std::string alleles, err;
    issl_vcf_indel_counts c{};
    if (read_exact(text, r, indels, alleles, c, err)) {
        for (const issl_indel &d : indels)
            std::printf("indel %u %llu %.*s %.*s\n", d.record, static_cast<unsigned long long>(d.pos), static_cast<int>(d.ref_len),
                        alleles.data() + d.ref_at, static_cast<int>(d.alt_len), alleles.data() + d.alt_at);
        std::printf("counts %llu %llu %llu %llu %llu %llu %llu\n", static_cast<unsigned long long>(c.lines), static_cast<unsigned long long>(c.indels),
                    static_cast<unsigned long long>(c.alleles_skipped), static_cast<unsigned long long>(c.no_allele),
                    static_cast<unsigned long long>(c.unknown_chrom), static_cast<unsigned long long>(c.beyond_record),
                    static_cast<unsigned long long>(c.too_long));
    } else {
        std::printf("refused %s\n", err.c_str());
    }
    size_t inputs = 0;
    for (size_t cut = 0; cut <= text.size(); ++cut, ++inputs) read_exact(text.substr(0, cut), r, indels, alleles, c, err);
    for (int k = 0; k < 3000 && !text.empty(); ++k, ++inputs) {
        std::string m = text;
        static const char bytes[] = "\t\n\r,#0195ACGTNacgt<>.*- \0\xff";
        for (uint32_t changes = 1 + rng() % 3; changes; --changes) m[rng() % m.size()] = bytes[rng() % (sizeof bytes - 1)];
        read_exact(m, r, indels, alleles, c, err);
    }
    std::printf("vcf ok %zu\n", inputs);
    return 0;
}
