// The plane arithmetic of the bulge search on a variant-aware text (crackling_amd/csrc/issl_bulge_variants_text.hpp:
// make_args, shifted_text, shifted_query, united, mismatch_a, mismatch_b, match_either, bound, walk_min, walk_mism, window_row,
// append_bulge_variant_line -- the functions k_bulge_variants, k_bulge_variants_finish and bin/isslSearchGenome call) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/bulge_variants_sanitize.cpp \
//       -o <tmp>/bulge_variants_sanitize && <tmp>/bulge_variants_sanitize
// For every L in 2..32, every legal span start g0, span lengths 2, 3, the middle one and the longest, every b in -3..3 that
// the limits allow (L + b <= 32, r <= G - 2), both strands, a query with and without N, on random windows of L + b codes
// with 0, 1 and 2 ambiguity codes over two alphabets (four letters; two letters, which makes ties and small distances):
// every break point's distance from the two mismatch words against a character loop over the derived pair of the contract
// -- sets of bases per position, cut by the derived pattern --, the minimum and the smallest break point that reaches it,
// mism in query coordinates, the bound never above the minimum and equal to it without a bulge, and window_row's site,
// n_var and admission.  Prints "bulge variants ok <alignments checked>", then sample lines of the executable.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_bulge_variants_text.hpp"

namespace st = issl::search_text;
namespace vt = issl::variants_text;
namespace bvt = issl::bulge_variants_text;

static void die(const char *what, uint32_t L = 0, uint32_t g0 = 0, uint32_t G = 0, int b = 0)
{
    std::fprintf(stderr, "bulge_variants_sanitize: %s (L %u span %u:%u b %d)\n", what, L, g0, G, b);
    std::exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

// P' or q' of alignment (b, i), as the contract spells it.
static std::string derived(const std::string &text, uint32_t g0, int b, uint32_t i)
{
    const size_t at = g0 + i;
    if (b >= 0) return text.substr(0, at) + std::string(static_cast<size_t>(b), 'N') + text.substr(at);
    return text.substr(0, at) + text.substr(at + static_cast<size_t>(-b));
}

static uint32_t complement(uint32_t set)
{
    return (set & 1u) << 3 | (set & 2u) << 1 | (set & 4u) >> 1 | (set & 8u) >> 3;
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
                    const bvt::BulgeVariantArgs v = bvt::make_args(pat, bg, b, static_cast<int>(L), static_cast<int>(L));
                    const uint32_t W = static_cast<uint32_t>(static_cast<int>(L) + b);
                    if (v.a.length != W || v.both_bits != (b < 0 ? W : L) || v.query_mask != st::low_bits32(L)) die("make_args", L, g0, G, b);
                    const std::string dp = derived(pattern, g0, b, v.g.i_lo); // the same for every break point (bulge_sanitize.cpp)
                    for (int trial = 0; trial < 24; ++trial) {
                        const bool with_n = trial & 1, two_letters = trial & 2;
                        const uint32_t n_codes = static_cast<uint32_t>(trial % 12 / 4), strand = static_cast<uint32_t>(trial / 12);
                        std::string w(W, 'A'), query(L, 'A');
                        for (char &c : w) c = two_letters ? "AC"[rng() & 1u] : "ACGT"[rng() & 3u];
                        uint32_t n_var = 0;
                        for (uint32_t k = 0; k < n_codes; ++k) {
                            const uint32_t p = rng() % W;
                            if (vt::text_set(static_cast<uint8_t>(w[p])) & (vt::text_set(static_cast<uint8_t>(w[p])) - 1)) continue;
                            w[p] = "RYSWKMBDHV"[rng() % 10];
                            ++n_var;
                        }
                        for (char &c : query) c = with_n && rng() % 4 == 0 ? 'N' : two_letters ? "AC"[rng() & 1u] : "ACGT"[rng() & 3u];
                        issl_search_query q;
                        if (!st::parse_query(query.data(), L, 0, &q, err)) die(err.c_str());
                        // what the strand reads, position by position, and the same cut by P'
                        std::vector<uint32_t> T(W), cut(W);
                        bool admitted = true;
                        for (uint32_t p = 0; p < W; ++p) {
                            T[p] = strand ? complement(vt::text_set(static_cast<uint8_t>(w[W - 1 - p]))) : vt::text_set(static_cast<uint8_t>(w[p]));
                            cut[p] = T[p] & st::iupac_bases(dp[p]);
                            admitted = admitted && cut[p];
                        }
                        bvt::RowFields row{};
                        if (!bvt::window_row(reinterpret_cast<const uint8_t *>(w.data()), v, strand, q.sig, q.care, row)) die("window_row refuses codes", L, g0, G, b);
                        if (row.n_var != n_var || row.admitted != admitted) die("n_var or the admission", L, g0, G, b);
                        for (uint32_t p = 0; p < 32; ++p)
                            if (vt::set_at(row.site, p) != (p < W ? T[p] : 0u)) die("the site", L, g0, G, b);
                        if (!admitted) continue; // (no row exists: the kernels drop the window-strand in the front)
                        const vt::Planes t = vt::intersect(row.site, v.a.allow), qp = vt::query_planes(q.sig, q.care, v.query_mask);
                        const vt::Planes tb = bvt::shifted_text(t, b), qb = bvt::shifted_query(qp, r);
                        const uint32_t A = bvt::mismatch_a(t, qp, v.both_mask), B = bvt::mismatch_b(tb, qb, v.both_mask);
                        uint32_t best = ~0u, best_i = 0, best_mism = 0;
                        for (uint32_t i = v.g.i_lo; i <= v.g.i_hi; ++i) {
                            // the character loop over the derived query, its mismatches mapped back to query positions
                            const std::string dq = derived(query, g0, b, i);
                            if (dq.size() != W) die("the derived query's length", L, g0, G, b);
                            uint32_t dist = 0, mism = 0;
                            for (uint32_t p = 0; p < W; ++p)
                                if (dq[p] != 'N' && !(cut[p] >> st::query_code(dq[p]) & 1u)) {
                                    ++dist;
                                    mism |= 1u << (p < g0 + i ? p : static_cast<uint32_t>(static_cast<int>(p) - b));
                                }
                            const uint32_t x = g0 + i;
                            const uint32_t got = static_cast<uint32_t>(__builtin_popcount(A & bvt::low32(x)) + __builtin_popcount(B & ~bvt::low32(x)));
                            if (got != dist) die("the distance of a break point", L, g0, G, b);
                            if (bvt::walk_mism(A, B, v.g, i) != mism) die("walk_mism", L, g0, G, b);
                            if (dist < best) {
                                best = dist;
                                best_i = i;
                                best_mism = mism;
                            }
                            ++checked;
                        }
                        uint32_t at = 99;
                        if (bvt::walk_min(A, B, v.g, at) != best || at != best_i) die("walk_min", L, g0, G, b);
                        const uint32_t either = bvt::match_either(t, tb, qp, qb);
                        if (either & ~v.both_mask) die("match_either leaves the mask", L, g0, G, b);
                        // the folded forms of the hot loop: the text united for a DNA bulge, the query for an RNA bulge
                        if (b >= 0 && vt::matches(bvt::united(t, tb), qp) != either) die("the united text", L, g0, G, b);
                        if (b < 0 && vt::matches(t, bvt::united(qp, qb)) != either) die("the united query", L, g0, G, b);
                        const uint32_t low = bvt::bound(either, v.both_bits);
                        if (low != static_cast<uint32_t>(__builtin_popcount(A & B))) die("the bound is popc(A & B)", L, g0, G, b);
                        if (low > best) die("the bound is above the minimum", L, g0, G, b);
                        if (b == 0 && low != best) die("without a bulge the bound is the distance", L, g0, G, b);
                        if (row.dist != best || row.at != best_i || row.mism != best_mism) die("window_row", L, g0, G, b);
                    }
                    // a byte that is none of the 14 codes, at every offset
                    for (uint32_t p = 0; p < W; ++p) {
                        std::string w(W, 'C');
                        w[p] = "Nn-\n"[rng() & 3u];
                        issl_search_query q{0, 0};
                        bvt::RowFields row{};
                        if (bvt::window_row(reinterpret_cast<const uint8_t *>(w.data()), v, p & 1u, q.sig, q.care, row)) die("window_row takes a bad byte", L, g0, G, b);
                    }
                }
            }
        }
    return checked;
}

static void set_site(issl_bulge_variant_hit &h, const char *codes)
{
    std::memset(h.site, 0, sizeof h.site);
    for (uint32_t i = 0; codes[i]; ++i)
        for (uint32_t b = 0; b < 4; ++b) h.site[b] |= (vt::text_set(static_cast<uint8_t>(codes[i])) >> b & 1u) << i;
}

int main()
{
    std::printf("bulge variants ok %zu\n", check_alignments());
    std::string out;
    issl_bulge_variant_hit h{};
    set_site(h, "ACGTACGTACRTGCAACGTACGGG");
    h.pos = 1234567890123ull;
    h.strand = 1;
    h.dist = 2;
    h.n_var = 1;
    h.bulge = 1;
    h.at = 10;
    h.mism = (1u << 0) | (1u << 10);
    bvt::append_bulge_variant_line(out, "CCGTACGTACTGCAACGTACNGG", 23, 0, "chr", 3, h);
    h.bulge = -2;
    h.at = 3;
    set_site(h, "ACGTACGYACTTGCAACGTAC");
    h.mism = (1u << 2) | (1u << 5) | (1u << 22) | (1u << 9);
    bvt::append_bulge_variant_line(out, "TTTACGTACGTACTTGCAACGTA", 23, 4, "chr", 3, h);
    h.bulge = 0;
    h.at = 0;
    set_site(h, "AKG");
    h.mism = 2;
    bvt::append_bulge_variant_line(out, "ATG", 3, 0, "", 0, h);
    std::fputs(out.c_str(), stdout);
    return 0;
}
