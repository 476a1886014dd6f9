// The plane arithmetic and the VCF reader of the variant-aware genome search (crackling_amd/csrc/issl_variants_text.hpp,
// the header issl_variants.hip and bin/isslSearchGenome include) under AddressSanitizer + UndefinedBehaviorSanitizer: a
// stand-alone CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/variants_sanitize.cpp \
//       -o <tmp>/variants_sanitize && <tmp>/variants_sanitize cases.txt file.vcf <name> <length> [<name> <length> ...]
// cases.txt: one case per line, "<pattern> <window> <query> <strand>", all of one length; printed per case, through
// window_row(): "none" for a window that holds a byte outside the 14 codes, else
// "<admitted> <dist> <mism hex> <n_var> <site[0..3] hex>".  Then the functions the kernels call -- text_set, set_letter,
// funnel, strand1, ambiguous, admits (with allow on the reversed window and with allow_rc on the forward one), intersect,
// matches, query_planes -- against character loops, for every length 1..32, random sets, both strands and window offsets
// 0..63 over three plane words: "arithmetic ok <window-strands checked>".  Then the VCF: the file's entries and counts are
// printed ("snp <record> <pos> <ref> <alt>", "counts ..." or "refused <message>"), and the reader is run on every
// truncation of the file and on 3000 copies with a byte changed, each in an allocation of exactly its size; what it
// returns goes through merge_snps: "vcf ok <inputs read>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_variants_text.hpp"

namespace st = issl::search_text;
namespace vt = issl::variants_text;

static void die(const char *what)
{
    std::fprintf(stderr, "variants_sanitize: %s\n", what);
    std::exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

// a set with its bases complemented: A<->T, C<->G
static uint32_t comp(uint32_t set) { return (set & 1u) << 3 | (set & 2u) << 1 | (set & 4u) >> 1 | (set & 8u) >> 3; }

static void check_tables()
{
    for (uint32_t c = 0; c < 256; ++c) {
        const char ch = static_cast<char>(c);
        uint32_t want = (ch >= 'A' && ch <= 'Z') ? st::iupac_bases(ch) : 0;
        if (want == 15) want = 0; // N is no code of a window
        if (vt::text_set(static_cast<uint8_t>(c)) != want) die("text_set");
    }
    for (uint32_t set = 1; set < 16; ++set)
        if (st::iupac_bases(vt::set_letter(set)) != set) die("set_letter");
    if (vt::set_letter(0) != '?') die("set_letter(0)");
}

static size_t check_arithmetic()
{
    static const char text_codes[] = "ACGTRYSWKMBDHV", pattern_codes[] = "ACGTRYSWKMBDHVN";
    size_t checked = 0;
    for (uint32_t L = 1; L <= 32; ++L) {
        for (int round = 0; round < 6; ++round) {
            // three plane words (96 positions); windows start in the first two
            std::string text(96, 'A');
            for (char &c : text) c = round < 2 ? "ACGT"[rng() & 3u] : (rng() % 29 == 0 ? 'N' : text_codes[rng() % 14]);
            uint32_t plane[4][3] = {}, bad[3] = {};
            for (size_t i = 0; i < text.size(); ++i) {
                const uint32_t set = vt::text_set(static_cast<uint8_t>(text[i]));
                for (uint32_t b = 0; b < 4; ++b) plane[b][i / 32] |= (set >> b & 1u) << (i % 32);
                bad[i / 32] |= (set ? 0u : 1u) << (i % 32);
            }
            std::string pattern(L, 'N'), query(L, 'N');
            for (char &c : pattern) c = round == 0 ? 'N' : pattern_codes[rng() % 15];
            for (char &c : query) c = "ACGTN"[rng() % 5];
            issl_search_pattern pat;
            issl_search_query q;
            std::string err;
            if (!st::prepare(pattern.c_str(), query.data(), 1, L, &pat, &q, err)) die(err.c_str());
            for (int v = -1; v <= static_cast<int>(L) + 1; ++v)
                if (vt::check_max_variants(&pat, v, err) != (v >= 0 && v <= static_cast<int>(L))) die("check_max_variants");
            const vt::VariantArgs a = vt::make_args(pat, 0, static_cast<int>(L));
            if (a.win_mask != st::low_bits32(L) || a.rev_shift != 32 - L || a.need != L) die("the masks of a length");
            const vt::Planes qp = vt::query_planes(q.sig, q.care, a.win_mask);
            for (uint32_t i = 0; i < L; ++i)
                if (vt::set_at(qp, i) != st::iupac_bases(query[i])) die("query_planes");
            for (uint32_t b = 0; b < 4; ++b)
                if (qp.p[b] & ~a.win_mask) die("query_planes above the length");
            for (uint32_t p = 0; p < 64; ++p) {
                const uint32_t wi = p / 32, sh = p % 32;
                const bool is_bad = (vt::funnel(bad[wi], bad[wi + 1], sh) & a.win_mask) != 0;
                bool want_bad = false;
                for (uint32_t i = 0; i < L; ++i) want_bad = want_bad || text[p + i] == 'N';
                if (is_bad != want_bad) die("the validity bits");
                if (is_bad) continue;
                const vt::Planes f{{vt::funnel(plane[0][wi], plane[0][wi + 1], sh) & a.win_mask, vt::funnel(plane[1][wi], plane[1][wi + 1], sh) & a.win_mask,
                                    vt::funnel(plane[2][wi], plane[2][wi + 1], sh) & a.win_mask, vt::funnel(plane[3][wi], plane[3][wi + 1], sh) & a.win_mask}};
                uint32_t n_var = 0;
                for (uint32_t i = 0; i < L; ++i) {
                    const uint32_t set = st::iupac_bases(text[p + i]);
                    if (vt::set_at(f, i) != set) die("the window cut");
                    n_var += (set & (set - 1)) != 0;
                }
                if (static_cast<uint32_t>(__builtin_popcount(vt::ambiguous(f))) != n_var) die("ambiguous");
                const vt::Planes r = vt::strand1(f, a.rev_shift);
                for (int strand = 0; strand < 2; ++strand) {
                    const vt::Planes &t = strand ? r : f;
                    bool admitted = true;
                    uint32_t mism = 0;
                    for (uint32_t i = 0; i < L; ++i) {
                        const uint32_t set = strand ? comp(st::iupac_bases(text[p + L - 1 - i])) : st::iupac_bases(text[p + i]);
                        if (vt::set_at(t, i) != set) die("strand1");
                        const uint32_t cut = set & st::iupac_bases(pattern[i]);
                        admitted = admitted && cut != 0;
                        if (query[i] != 'N' && !(cut & st::iupac_bases(query[i]))) mism |= 1u << i;
                    }
                    for (uint32_t b = 0; b < 4; ++b)
                        if (t.p[b] & ~a.win_mask) die("bits above the length");
                    if (vt::admits(t, a.allow, a.win_mask) != admitted) die("admits");
                    if (vt::admits(f, strand ? a.allow_rc : a.allow, a.win_mask) != admitted) die("admits on the forward window");
                    vt::RowFields row{};
                    if (!vt::window_row(reinterpret_cast<const uint8_t *>(text.data()) + p, a, static_cast<uint32_t>(strand), q.sig, q.care, row))
                        die("window_row refuses a window of codes");
                    if (row.admitted != admitted || row.n_var != n_var || std::memcmp(&row.site, &t, sizeof t)) die("window_row");
                    ++checked;
                    if (!admitted) continue; // (only an admitted window-strand is compared: an N of the query meets no empty set)
                    const vt::Planes cut = vt::intersect(t, a.allow);
                    if (vt::mismatches(cut, qp, a.win_mask) != mism || row.mism != mism) die("mismatches");
                    if (static_cast<uint32_t>(__builtin_popcount(vt::matches(cut, qp))) != L - static_cast<uint32_t>(__builtin_popcount(mism)))
                        die("matches");
                    if (row.dist != static_cast<uint32_t>(__builtin_popcount(mism))) die("window_row's distance");
                }
            }
        }
    }
    return checked;
}

static void run_cases(const char *path)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) die("cannot open the cases");
    char pattern[64], window[64], query[64];
    unsigned strand;
    while (std::fscanf(fp, "%63s %63s %63s %u", pattern, window, query, &strand) == 4) {
        const size_t L = std::strlen(pattern);
        if (std::strlen(window) != L || std::strlen(query) != L) die("a case of two lengths");
        issl_search_pattern pat;
        issl_search_query q;
        std::string err;
        if (!st::prepare(pattern, query, 1, L, &pat, &q, err)) die(err.c_str());
        const vt::VariantArgs a = vt::make_args(pat, 0, static_cast<int>(L));
        uint8_t *exact = static_cast<uint8_t *>(std::malloc(L)); // a read past the window is a report
        if (!exact) die("no memory");
        std::memcpy(exact, window, L);
        vt::RowFields row{};
        if (!vt::window_row(exact, a, strand, q.sig, q.care, row)) std::printf("none\n");
        else
            std::printf("%d %u %x %u %x %x %x %x\n", row.admitted ? 1 : 0, row.dist, row.mism, row.n_var, row.site.p[0], row.site.p[1],
                        row.site.p[2], row.site.p[3]);
        std::free(exact);
    }
    std::fclose(fp);
}

struct Records {
    std::vector<std::string> names;
    std::vector<const char *> ptrs;
    std::vector<size_t> lens;
    std::vector<uint64_t> lengths, starts;
};

// One run of the reader on bytes copied into an allocation of exactly their size.  -> what it found.
static bool read_exact(const std::string &text, const Records &r, std::vector<issl_snp> &out, issl_vcf_counts &counts, std::string &err)
{
    char *exact = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));
    if (!exact) die("no memory");
    std::memcpy(exact, text.data(), text.size());
    size_t n = 0, again = 0;
    bool ok = vt::vcf_snps(exact, text.size(), r.ptrs.data(), r.lens.data(), r.lengths.data(), r.names.size(), nullptr, 0, &n, &counts, err);
    out.assign(n, issl_snp{});
    if (ok) {
        if (n > 1) { // one below: nothing may be written
            std::vector<issl_snp> small(n - 1);
            if (!vt::vcf_snps(exact, text.size(), r.ptrs.data(), r.lens.data(), r.lengths.data(), r.names.size(), small.data(), n - 1, &again, nullptr, err) ||
                again != n)
                die("the counting rule");
            for (const issl_snp &s : small)
                if (s.pos || s.record || s.ref || s.alt) die("a short buffer was written");
        }
        ok = vt::vcf_snps(exact, text.size(), r.ptrs.data(), r.lens.data(), r.lengths.data(), r.names.size(), out.data(), n, &again, &counts, err);
        if (!ok || again != n || counts.snps != n) die("the second call differs");
        for (const issl_snp &s : out)
            if (s.record >= r.names.size() || s.pos >= r.lengths[s.record] || (s.ref != 1 && s.ref != 2 && s.ref != 4 && s.ref != 8) || !s.alt ||
                s.alt > 15)
                die("an entry out of range");
        if (counts.lines != counts.snps + counts.no_allele + counts.unknown_chrom + counts.beyond_record) die("the counts do not add up");
        std::vector<vt::SnpPlace> places;
        std::string merge_err;
        if (vt::merge_snps(out.data(), out.size(), r.starts.data(), r.lengths.data(), r.names.size(), places, merge_err)) {
            for (size_t k = 1; k < places.size(); ++k)
                if (places[k - 1].at >= places[k].at) die("merge_snps: the places are not ascending");
        } else if (merge_err.find("ref differs") == std::string::npos) die("merge_snps refuses entries in range");
    }
    std::free(exact);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 3) % 2) die("usage: variants_sanitize cases.txt file.vcf <name> <length> ...");
    check_tables();
    run_cases(argv[1]);
    std::printf("arithmetic ok %zu\n", check_arithmetic());

    Records r;
    for (int i = 3; i + 1 < argc; i += 2) {
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
        FILE *fp = std::fopen(argv[2], "rb");
        if (!fp) die("cannot open the VCF");
        char buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
        std::fclose(fp);
    }
    std::vector<issl_snp> snps;
    issl_vcf_counts c{};
    std::string err;
    if (read_exact(text, r, snps, c, err)) {
        for (const issl_snp &s : snps)
            std::printf("snp %u %llu %u %u\n", s.record, static_cast<unsigned long long>(s.pos), static_cast<unsigned>(s.ref), static_cast<unsigned>(s.alt));
        std::printf("counts %llu %llu %llu %llu %llu %llu\n", static_cast<unsigned long long>(c.lines), static_cast<unsigned long long>(c.snps),
                    static_cast<unsigned long long>(c.alleles_skipped), static_cast<unsigned long long>(c.no_allele),
                    static_cast<unsigned long long>(c.unknown_chrom), static_cast<unsigned long long>(c.beyond_record));
    } else {
        std::printf("refused %s\n", err.c_str());
    }
    size_t inputs = 0;
    for (size_t cut = 0; cut <= text.size(); ++cut, ++inputs) read_exact(text.substr(0, cut), r, snps, c, err);
    for (int k = 0; k < 3000 && !text.empty(); ++k, ++inputs) {
        std::string m = text;
        static const char bytes[] = "\t\n\r,#0195ACGTN<>.*- \0\xff";
        for (uint32_t changes = 1 + rng() % 3; changes; --changes) m[rng() % m.size()] = bytes[rng() % (sizeof bytes - 1)];
        read_exact(m, r, snps, c, err);
    }
    std::printf("vcf ok %zu\n", inputs);
    return 0;
}
