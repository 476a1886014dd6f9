// The rules RNAfold's output is read by (crackling_amd/csrc/issl_folds_text.hpp, the code the kernels of issl_folds.hip
// run per row) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/folds_sanitize.cpp \
//       -o <tmp>/folds_sanitize && <tmp>/folds_sanitize cases.bin
// cases.bin: per case  u32 n_guides, n_guides x 23 bytes (the guides of the page, in the order of the fold list), u64 len,
// len bytes (what RNAfold printed), little endian.  Every text is copied into an allocation of exactly len bytes, so a read
// past it is a report.  The pairs are found as the device finds them -- every byte asked whether it ends a line, the parity
// of the line's number, the key, the last pair of a key wins, the text's last line starts no pair -- with a std::map in
// place of the sorted keys.  Printed per case: "case <k>", then per guide "-" (no pair), or
// "<energy bits as hex> <scaffold> <present> <offset> <length> x 3"; a refused case prints "refused <code> <row>" instead
// of its rows, for the lowest refused row.  tests/test_folds_model.py compares that with the model of tests/folds_util.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_folds_text.hpp"

namespace ft = issl::folds_text;

static void die(const char *what)
{
    std::fprintf(stderr, "folds_sanitize: %s\n", what);
    std::exit(1);
}

static bool take(FILE *fp, void *out, size_t n) { return n == 0 || std::fread(out, 1, n, fp) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) die("usage: folds_sanitize cases.bin");
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) die("cannot open the cases");
    for (unsigned k = 0;; ++k) {
        uint32_t n_guides;
        if (std::fread(&n_guides, 1, 4, fp) != 4) break;
        std::vector<char> guides(23ull * n_guides);
        uint64_t len;
        if (!take(fp, guides.data(), guides.size()) || !take(fp, &len, 8)) die("a case is cut short");
        uint8_t *text = static_cast<uint8_t *>(std::malloc(len ? len : 1)); // (exactly len bytes where there are any)
        if (!text || !take(fp, text, len)) die("a case is cut short");
        if (len == 0) { std::free(text); text = nullptr; }
        std::printf("case %u\n", k);
        const uint64_t last_line = ft::last_line_start(text, len);
        std::map<uint64_t, uint64_t> first_of; // key -> offset of the pair's first line
        auto offer = [&](uint64_t start) { // a pair starts here when the line has a partner and a key
            uint64_t key;
            if (start < last_line && ft::pair_key(text, start, len, key)) first_of[key] = start;
        };
        if (len) offer(0);
        uint32_t line = 0; // the number of the line the next end closes, modulo 2^32 as the device's ranks are
        for (uint64_t g = 0; g * 64 < len; ++g) { // k_folds_mark / k_folds_pairs: 64 bytes at a time, as sixteen words
            const uint64_t here = len - g * 64;
            uint64_t lf = 0, cr = 0;
            for (uint32_t w = 0; w < 16; ++w) {
                uint32_t word = 0; // (the device reads its buffer's zero padding behind the text)
                for (uint32_t b = 0; b < 4; ++b)
                    if (4ull * w + b < here) word |= static_cast<uint32_t>(text[g * 64 + 4 * w + b]) << (8 * b);
                ft::byte_masks(word, 4 * w, lf, cr);
            }
            uint64_t ends = ft::group_line_ends(lf, cr, here, here > 64 && text[(g + 1) * 64] == '\n');
            for (uint32_t b = 0; b < 64 && g * 64 + b < len; ++b) { // the same question asked byte by byte
                const uint64_t i = g * 64 + b;
                if (ft::ends_line(text[i], i + 1 < len ? text[i + 1] : 0) != (((ends >> b) & 1u) != 0)) die("the group's mask and the bytes disagree");
            }
            while (ends) {
                const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(ends));
                ends &= ends - 1;
                if (line & 1u) offer(g * 64 + b + 1);
                ++line;
            }
        }
        std::string rows;
        uint64_t refused_row = 0;
        uint32_t refused = ft::kFine;
        for (uint32_t g = 0; g < n_guides && refused == ft::kFine; ++g) {
            uint64_t key = 0;
            for (uint32_t p = 1; p < 20; ++p) {
                const char c = guides[23ull * g + p];
                key |= static_cast<uint64_t>(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3) << (2 * (p - 1));
            }
            const auto at = first_of.find(key);
            if (at == first_of.end()) {
                rows += "-\n";
                continue;
            }
            ft::Pair pair;
            const uint32_t kind = ft::read_pair(text, len, at->second, pair);
            if (kind != ft::kFine) {
                refused = kind;
                refused_row = g;
                break;
            }
            for (int c = 0; c < 3; ++c) { // the quoting bits of a span against the question asked byte by byte
                const uint32_t bits = ft::quote_bits(text, pair.offset[c], pair.length[c]);
                for (const char d : {',', '\t', ';', '|', ' '}) {
                    bool needs = false;
                    for (uint32_t i = 0; i < pair.length[c]; ++i) {
                        const char x = static_cast<char>(text[pair.offset[c] + i]);
                        needs = needs || x == d || x == '"' || x == '\n' || x == '\r';
                    }
                    if (needs != ((bits & (ft::quote_bit(static_cast<uint8_t>(d)) | ft::quote_bit('"'))) != 0)) die("quote bits");
                }
            }
            uint64_t energy;
            std::memcpy(&energy, &pair.energy, 8);
            char buf[256];
            std::snprintf(buf, sizeof buf, "%016llx %u %u %llu %u %llu %u %llu %u\n", static_cast<unsigned long long>(energy), pair.scaffold,
                          pair.present, static_cast<unsigned long long>(pair.offset[0]), pair.length[0],
                          static_cast<unsigned long long>(pair.offset[1]), pair.length[1], static_cast<unsigned long long>(pair.offset[2]),
                          pair.length[2]);
            rows += buf;
        }
        if (refused != ft::kFine) std::printf("refused %d %llu\n", refused == ft::kFormat ? -3 : -4, static_cast<unsigned long long>(refused_row));
        else std::fputs(rows.c_str(), stdout);
        std::free(text);
    }
    std::fclose(fp);
    return 0;
}
