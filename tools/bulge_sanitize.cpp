// The bulge arithmetic of the genome search (crackling_amd/csrc/issl_search_text.hpp: bulge_shift, bulge_both, bulge_min,
// bulge_mism, bulge_row, bulge_pattern, check_bulges, append_bulge_line -- the functions k_bulge, k_bulge_finish and
// bin/isslSearchGenome call) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone CPU program, no device code
// and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/bulge_sanitize.cpp \
//       -o <tmp>/bulge_sanitize && <tmp>/bulge_sanitize
// For every L in 2..32, every legal span start g0, span lengths 2, 3, the middle one and the longest, every b in -3..3 that
// the limits allow (L + b <= 32, r <= G - 2) and a query with and without N, on random windows over two alphabets (four
// letters; two letters, which makes ties and small distances): every break point's distance from the two mismatch words
// against a character loop over the derived pair of the contract, the minimum and the smallest break point that reaches it,
// mism in query coordinates, the bound never above the minimum, and the derived pattern against the one built as text.
// Prints "bulges ok <alignments checked>", then the refusals of check_bulges and sample lines of the executable.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_search_text.hpp"

namespace st = issl::search_text;

static void die(const char *what, uint32_t L = 0, uint32_t g0 = 0, uint32_t G = 0, int b = 0)
{
    std::fprintf(stderr, "bulge_sanitize: %s (L %u span %u:%u b %d)\n", what, L, g0, G, b);
    std::exit(1);
}

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rng()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

static uint64_t pack(const std::string &text)
{
    uint64_t w = 0;
    for (size_t i = 0; i < text.size(); ++i) w |= static_cast<uint64_t>(st::query_code(text[i]) & 3u) << (2 * i);
    return w;
}

// P' or q' of alignment (b, i), as the contract spells it.
static std::string derived(const std::string &text, uint32_t g0, int b, uint32_t i)
{
    const size_t at = g0 + i;
    if (b >= 0) return text.substr(0, at) + std::string(static_cast<size_t>(b), 'N') + text.substr(at);
    return text.substr(0, at) + text.substr(at + static_cast<size_t>(-b));
}

static size_t check_alignments()
{
    size_t checked = 0;
    for (uint32_t L = 2; L <= 32; ++L)
        for (uint32_t g0 = 0; g0 + 2 <= L; ++g0) {
            const uint32_t longest = L - g0;
            const uint32_t spans[4] = {2, 3, longest / 2 + 1, longest};
            for (uint32_t G : spans) {
                if (G < 2 || G > longest) continue;
                // a pattern with codes at the span's ends and outside it, N inside
                std::string pattern(L, 'N');
                for (uint32_t p = 0; p < L; ++p)
                    if (p <= g0 || p + 1 >= g0 + G) pattern[p] = "NRYVN"[rng() % 5];
                issl_search_pattern pat;
                std::string err;
                if (!st::parse_pattern(pattern.c_str(), &pat, err)) die(err.c_str());
                for (int b = -3; b <= 3; ++b) {
                    const uint32_t r = b < 0 ? static_cast<uint32_t>(-b) : 0u;
                    if (static_cast<int>(L) + b > 32 || r + 2 > G) continue;
                    const issl_search_bulges bg{g0, G, b > 0 ? static_cast<uint32_t>(b) : 0u, r};
                    if (!st::check_bulges(&pat, &bg, err)) die(err.c_str(), L, g0, G, b);
                    const st::BulgeArgs ba = st::make_bulge_args(bg, b);
                    if (b && (ba.i_lo != 1 || ba.i_hi != G - 1 - r)) die("the break points of a bulge", L, g0, G, b);
                    // P' is the same for every break point and is what bulge_pattern gives
                    const issl_search_pattern dp = st::bulge_pattern(pat, bg, b);
                    for (uint32_t i = ba.i_lo; i <= ba.i_hi; ++i) {
                        issl_search_pattern want;
                        if (!st::parse_pattern(derived(pattern, g0, b, i).c_str(), &want, err)) die(err.c_str(), L, g0, G, b);
                        if (std::memcmp(&want, &dp, sizeof want)) die("bulge_pattern", L, g0, G, b);
                    }
                    for (int trial = 0; trial < 4; ++trial) {
                        const bool with_n = trial & 1, two_letters = trial & 2;
                        const uint32_t W = static_cast<uint32_t>(static_cast<int>(L) + b);
                        std::string t(W, 'A'), query(L, 'A');
                        for (char &c : t) c = two_letters ? "AC"[rng() & 1u] : "ACGT"[rng() & 3u];
                        for (char &c : query) c = with_n && rng() % 4 == 0 ? 'N' : two_letters ? "AC"[rng() & 1u] : "ACGT"[rng() & 3u];
                        issl_search_query q;
                        if (!st::parse_query(query.data(), L, 0, &q, err)) die(err.c_str());
                        const uint64_t tw = pack(t), tb = st::bulge_shift(tw, b);
                        const uint64_t A = st::mismatches(tw, q.sig, q.care & st::kEven), B = st::mismatches(tb, q.sig, q.care & st::kEven);
                        uint32_t best = ~0u, best_i = 0, best_mism = 0;
                        for (uint32_t i = ba.i_lo; i <= ba.i_hi; ++i) {
                            // the character loop over the derived query, its mismatches mapped back to query positions
                            const std::string dq = derived(query, g0, b, i);
                            if (dq.size() != W) die("the derived query's length", L, g0, G, b);
                            uint32_t dist = 0, mism = 0;
                            for (uint32_t p = 0; p < W; ++p)
                                if (dq[p] != 'N' && dq[p] != t[p]) {
                                    ++dist;
                                    mism |= 1u << (p < g0 + i ? p : static_cast<uint32_t>(static_cast<int>(p) - b));
                                }
                            const uint32_t x = g0 + i;
                            const uint32_t got = static_cast<uint32_t>(__builtin_popcountll(A & st::low_pairs(x)) +
                                                                       __builtin_popcountll(B & ~st::low_pairs(x + r)));
                            if (got != dist) die("the distance of a break point", L, g0, G, b);
                            if (st::gather_even_bits(st::bulge_mism(A, B, ba, i)) != mism) die("bulge_mism", L, g0, G, b);
                            if (dist < best) {
                                best = dist;
                                best_i = i;
                                best_mism = mism;
                            }
                            ++checked;
                        }
                        uint32_t at = 99;
                        if (st::bulge_min(A, B, ba, at) != best || at != best_i) die("bulge_min", L, g0, G, b);
                        // the bound as k_bulge forms it: the text shifted for a DNA bulge, the query for an RNA bulge
                        const uint32_t both = st::bulge_both(tw, st::bulge_bound_text(tw, b), q.sig, st::bulge_bound_query(q.sig, r),
                                                             q.care & st::bulge_bound_query(q.care, r) & ~st::kEven);
                        if (both != static_cast<uint32_t>(__builtin_popcountll(A & (B >> (2 * r))))) die("bulge_both", L, g0, G, b);
                        if (static_cast<uint32_t>(__builtin_popcountll(A & B)) > best + r) die("popc(A & B) - r is above the minimum", L, g0, G, b);
                        if (both > best) die("the bound is above the minimum", L, g0, G, b);
                        if (b == 0 && both != best) die("without a bulge the bound is the distance", L, g0, G, b);
                        uint32_t dist, mism;
                        if (st::bulge_row(tw, q, ba, best, dist, at, mism) != true || dist != best || at != best_i || mism != best_mism)
                            die("bulge_row", L, g0, G, b);
                        if (best > 0 && st::bulge_row(tw, q, ba, best - 1, dist, at, mism)) die("bulge_row above max_dist", L, g0, G, b);
                    }
                }
            }
        }
    return checked;
}

static void refusal(const char *pattern, issl_search_bulges bg)
{
    issl_search_pattern pat;
    std::string err;
    if (!st::parse_pattern(pattern, &pat, err)) die(err.c_str());
    if (st::check_bulges(&pat, &bg, err)) std::printf("accepted\n");
    else std::printf("refused %s\n", err.c_str());
}

int main()
{
    std::printf("bulges ok %zu\n", check_alignments());
    const char *ngg = "NNNNNNNNNNNNNNNNNNNNNGG";
    refusal(ngg, {0, 20, 2, 2});
    refusal(ngg, {0, 23, 0, 0}); // any code inside the span when nothing bulges
    refusal("VNNNNNNNNNNNNNNNNNNNNRG", {0, 20, 3, 3});
    refusal(ngg, {4, 20, 1, 1});
    refusal(ngg, {0, 1, 1, 0});
    refusal(ngg, {24, 2, 1, 0});
    refusal(ngg, {0xFFFFFFFFu, 2, 1, 0});
    refusal(ngg, {2, 0xFFFFFFFFu, 1, 0});
    refusal(ngg, {0, 20, 4, 0});
    refusal(ngg, {0, 20, 0, 4});
    refusal("NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNGG", {0, 20, 1, 0});
    refusal(ngg, {0, 3, 0, 2});
    refusal(ngg, {0, 23, 1, 0});
    refusal("NNNNNRNNNNNNNNNNNNNNNGG", {0, 20, 0, 1});
    std::string out;
    issl_bulge_hit h{};
    h.site = pack("ACGTACGTACTTGCAACGTACGGG");
    h.pos = 1234567890123ull;
    h.strand = 1;
    h.dist = 2;
    h.bulge = 1;
    h.at = 10;
    h.mism = (1u << 0) | (1u << 10);
    st::append_bulge_line(out, "CCGTACGTACTGCAACGTACNGG", 23, 0, "chr", 3, h);
    h.bulge = -2;
    h.at = 3;
    h.site = pack("ACGTACGTACTTGCAACGTAC");
    h.mism = (1u << 2) | (1u << 5) | (1u << 22);
    st::append_bulge_line(out, "TTTACGTACGTACTTGCAACGTA", 23, 4, "chr", 3, h);
    h.bulge = 0;
    h.at = 0;
    h.site = pack("ACG");
    h.mism = 2;
    st::append_bulge_line(out, "ATG", 3, 0, "", 0, h);
    std::fputs(out.c_str(), stdout);
    return 0;
}
