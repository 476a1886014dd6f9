// The text side and the packed-word arithmetic of the genome search (crackling_amd/csrc/issl_search_text.hpp, the header
// issl_search.hip and bin/isslSearchGenome include) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone CPU
// program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/search_sanitize.cpp \
//       -o <tmp>/search_sanitize && <tmp>/search_sanitize cases.bin
// cases.bin, little endian, per case: u32 pattern length, the pattern's bytes, u32 n, u32 stride, then (n - 1) * stride +
// pattern length bytes of query text (nothing when n == 0).  Pattern and queries are copied into allocations of exactly
// their size (the pattern with its NUL), so a read past either is a report.  Printed per case: "case <k>", then
// "refused <message>" or "pattern <allow[0..3] as hex> <length>" and one "<sig as hex> <care as hex>" per query.
// Then the arithmetic the kernels do on packed words -- window_word, reverse_complement, admits, mismatches,
// distance, gather_even_bits, spread_bits -- against plain character loops, for every length 1..32 on random text, as the kernel cuts
// its windows out of three words of 16 bases: "arithmetic ok <windows checked>".  Last the lines of the executable: query
// files with both line ends, a trailing blank line, a short line; hit and profile lines.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_search_text.hpp"

namespace st = issl::search_text;

static void die(const char *what)
{
    std::fprintf(stderr, "search_sanitize: %s\n", what);
    std::exit(1);
}

static bool take(FILE *fp, void *out, size_t n) { return n == 0 || std::fread(out, 1, n, fp) == n; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

static char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// base i of `text` at bits 2i, 2i + 1
static uint64_t pack(const std::string &text)
{
    uint64_t w = 0;
    for (size_t i = 0; i < text.size(); ++i) w |= static_cast<uint64_t>(st::query_code(text[i])) << (2 * i);
    return w;
}

static size_t check_arithmetic()
{
    static const char codes[] = "ACGTRYSWKMBDHVN";
    size_t checked = 0;
    for (uint32_t L = 1; L <= 32; ++L) {
        for (int round = 0; round < 6; ++round) {
            // a tile of 5 words (80 bases); windows start in the first three
            std::string text(80, 'A');
            for (char &c : text) c = "ACGT"[rng() & 3u];
            uint32_t words[5] = {};
            for (size_t i = 0; i < text.size(); ++i) words[i / 16] |= st::query_code(text[i]) << (2 * (i % 16));
            std::string pattern(L, 'N'), query(L, 'N');
            for (char &c : pattern) c = round == 0 ? 'N' : codes[rng() % 15];
            for (char &c : query) c = "ACGTN"[rng() % 5];
            issl_search_pattern pat;
            issl_search_query q;
            std::string err;
            if (!st::prepare(pattern.c_str(), query.data(), 1, L, &pat, &q, err)) die(err.c_str());
            if (!st::check_pattern(&pat, static_cast<int>(L), err) || !st::check_queries(&q, 1, L, err)) die(err.c_str());
            const st::SearchArgs a = st::make_args(pat, 0);
            const uint64_t in_mask = a.full | (a.full << 1);
            if (in_mask != st::low_bits64(2 * L) || a.rev_shift != 64 - 2 * L) die("the masks of a length");
            for (uint32_t p = 0; p < 48; ++p) {
                const std::string w = text.substr(p, L);
                std::string rc(L, 'A');
                for (uint32_t i = 0; i < L; ++i) rc[i] = complement(w[L - 1 - i]);
                const uint64_t f = st::window_word(words[p / 16], words[p / 16 + 1], words[p / 16 + 2], p % 16, in_mask);
                if (f != pack(w)) die("window_word");
                const uint64_t r = st::reverse_complement(f, a.rev_shift);
                if (r != pack(rc)) die("reverse_complement");
                for (int strand = 0; strand < 2; ++strand) {
                    const std::string &t = strand ? rc : w;
                    const uint64_t tw = strand ? r : f;
                    bool admitted = true;
                    uint32_t mism = 0;
                    for (uint32_t i = 0; i < L; ++i) {
                        admitted = admitted && (st::iupac_bases(pattern[i]) >> st::query_code(t[i]) & 1u);
                        if (query[i] != 'N' && query[i] != t[i]) mism |= 1u << i;
                    }
                    if (st::admits(a, tw) != admitted) die("admits");
                    const uint64_t m = st::mismatches(tw, q.sig, q.care & st::kEven);
                    if (st::gather_even_bits(m) != mism || st::spread_bits(mism) != m) die("mismatches");
                    if (st::distance(tw, q.sig, q.care & ~st::kEven) != static_cast<uint32_t>(__builtin_popcount(mism))) die("distance");
                    ++checked;
                }
            }
        }
    }
    return checked;
}

static void show_lines(const std::string &text, uint32_t length)
{
    char *exact = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));
    if (!exact) die("no memory");
    std::memcpy(exact, text.data(), text.size());
    std::string packed, err;
    size_t n = 0;
    if (st::split_query_lines(std::string(exact, text.size()), length, packed, n, err)) std::printf("lines %zu %s\n", n, packed.c_str());
    else std::printf("lines refused %s\n", err.c_str());
    std::free(exact);
}

int main(int argc, char **argv)
{
    if (argc != 2) die("usage: search_sanitize cases.bin");
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) die("cannot open the cases");
    for (unsigned k = 0;; ++k) {
        uint32_t plen, n, stride;
        if (std::fread(&plen, 1, 4, fp) != 4) break;
        char *pattern = static_cast<char *>(std::malloc(plen + 1ull));
        if (!pattern || !take(fp, pattern, plen) || !take(fp, &n, 4) || !take(fp, &stride, 4)) die("a case is cut short");
        pattern[plen] = 0;
        const size_t qbytes = n ? (n - 1ull) * stride + plen : 0;
        char *queries = static_cast<char *>(std::malloc(qbytes ? qbytes : 1));
        if (!queries || !take(fp, queries, qbytes)) die("a case is cut short");
        issl_search_pattern pat;
        std::vector<issl_search_query> out(n);
        std::string err;
        std::printf("case %u\n", k);
        if (!st::prepare(pattern, n ? queries : nullptr, n, stride, &pat, n ? out.data() : nullptr, err)) {
            std::printf("refused %s\n", err.c_str());
        } else {
            std::printf("pattern %08x %08x %08x %08x %u\n", pat.allow[0], pat.allow[1], pat.allow[2], pat.allow[3], pat.length);
            for (const auto &q : out) std::printf("%016llx %016llx\n", static_cast<unsigned long long>(q.sig), static_cast<unsigned long long>(q.care));
            // every max_dist the call accepts and the two next to them
            for (int d = -1; d <= static_cast<int>(pat.length) + 1; ++d)
                if (st::check_pattern(&pat, d, err) != (d >= 0 && d <= static_cast<int>(pat.length))) die("check_pattern");
            if (!st::check_queries(out.data(), n, pat.length, err)) die(err.c_str());
        }
        std::free(pattern);
        std::free(queries);
    }
    std::fclose(fp);
    std::printf("arithmetic ok %zu\n", check_arithmetic());

    show_lines("ACG\nNNN\n", 3);
    show_lines("ACG\r\nNNN", 3);
    show_lines("ACG\nNNN\n\n", 3);
    show_lines("ACG\nNN\n", 3);
    show_lines("", 3);
    show_lines("\n", 3);
    std::string out;
    issl_search_hit h{};
    h.site = pack("ACGTACGTACGTACGTACGTACGTACGTACGT");
    h.pos = 1234567890123ull;
    h.strand = 1;
    h.dist = 2;
    h.mism = 0x80000001u;
    st::append_hit_line(out, "ACGTACGTACGTACGTACGTACGTACGTACGN", 32, "chr", 3, h);
    const uint64_t counts[3] = {0, 7, 18446744073709551615ull};
    st::append_profile_line(out, "ACG", 3, counts, 2);
    std::fputs(out.c_str(), stdout);
    return 0;
}
