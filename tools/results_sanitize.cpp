// The host-side text handling of the result table (crackling_amd/csrc/issl_results_text.hpp: CSV quoting, the name up to
// the first blank, the check and rewrite of the caller's text spans, the header row) and the number formatting its kernels
// share with the host (crackling_amd/csrc/issl_repr.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
// CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/results_sanitize.cpp \
//       -o <tmp>/results_sanitize && <tmp>/results_sanitize
// Random texts over the characters that mean something to the writer are quoted and read back by a CSV reader written here;
// random spans, a third of them leaving the text, go through results_ss_spans; a hundred thousand random doubles, every
// power of two and the neighbours of every power of ten are printed and must read back (strtod) as the same double with
// no more digits than the shortest "%.*e" that does; scores go through
// through_text against snprintf("%f") + strtod.  Exit status 0 and "ok" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_repr.hpp"
#include "../crackling_amd/csrc/issl_results_text.hpp"

#define ISSL_REPR_QUAL static const
#include "../crackling_amd/csrc/repr_tables.inc"

static void die(const char *what, const std::string &detail = std::string())
{
    std::fprintf(stderr, "results_sanitize: %s %s\n", what, detail.c_str());
    std::exit(1);
}

// One CSV field from `in` at `at` (QUOTE_MINIMAL, doubled quotes) -> the text, `at` behind the field.
static std::string read_field(const std::string &in, size_t &at, char delimiter)
{
    std::string out;
    if (at < in.size() && in[at] == '"') {
        for (++at; at < in.size(); ++at) {
            if (in[at] == '"') {
                if (at + 1 < in.size() && in[at + 1] == '"') { out.push_back('"'); ++at; }
                else { ++at; break; }
            } else out.push_back(in[at]);
        }
    } else {
        while (at < in.size() && in[at] != delimiter && in[at] != '\n') out.push_back(in[at++]);
    }
    return out;
}

static void check_quoting(std::mt19937_64 &rng)
{
    const char alphabet[] = {',', '\t', ';', '|', ' ', '"', '\n', '\r', 'a', 'Z', '0', '\0', char(0xFF), '\''};
    const char delimiters[] = {',', '\t', ';', '|', ' '};
    for (int round = 0; round < 60000; ++round) {
        const char d = delimiters[rng() % 5];
        std::string line;
        std::vector<std::string> fields(1 + rng() % 4);
        for (size_t f = 0; f < fields.size(); ++f) {
            const size_t len = rng() % 12;
            for (size_t i = 0; i < len; ++i) fields[f].push_back(alphabet[rng() % sizeof alphabet]);
            if (f) line.push_back(d);
            const size_t before = line.size();
            issl::csv_append(fields[f].data(), fields[f].size(), d, line);
            const bool quoted = line.size() > before && line[before] == '"' && issl::csv_needs_quotes(fields[f].data(), fields[f].size(), d);
            if (quoted != issl::csv_needs_quotes(fields[f].data(), fields[f].size(), d)) die("quotes");
            if (!quoted && line.size() - before != fields[f].size()) die("a field that needs no quotes changed");
        }
        line.push_back('\n');
        size_t at = 0;
        for (size_t f = 0; f < fields.size(); ++f) {
            if (read_field(line, at, d) != fields[f]) die("a field does not read back");
            if (at >= line.size() || line[at] != (f + 1 < fields.size() ? d : '\n')) die("no separator behind a field");
            ++at;
        }
        if (at != line.size()) die("text behind the last field");
    }
    for (const char d : delimiters) {
        if (!issl::results_delimiter_ok(d)) die("a supported delimiter is refused");
        const std::string row = issl::results_header_row(d);
        size_t n = 0;
        for (const char c : row) n += c == d;
        if (n != 25 || row.back() != '\n' || row.compare(0, 4, std::string("seq") + d) != 0) die("header row");
    }
    for (int c = 0; c < 256; ++c)
        if (issl::results_delimiter_ok(static_cast<char>(c)) != (c == ',' || c == '\t' || c == ';' || c == '|' || c == ' ')) die("delimiter set");
}

static void check_first_word(std::mt19937_64 &rng)
{
    const char alphabet[] = {' ', '\t', '\n', '\v', '\f', '\r', 'a', 'b', ',', '"', '\0'};
    for (int round = 0; round < 100000; ++round) {
        std::string name;
        const size_t len = rng() % 10;
        for (size_t i = 0; i < len; ++i) name.push_back(alphabet[rng() % sizeof alphabet]);
        size_t begin = 99, n = 99;
        issl::first_word(name.data(), name.size(), begin, n);
        if (begin + n > name.size()) die("word outside the name");
        auto blank = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
        for (size_t i = 0; i < begin; ++i) if (!blank(name[i])) die("a character ahead of the word");
        for (size_t i = begin; i < begin + n; ++i) if (blank(name[i])) die("a blank inside the word");
        if (begin + n < name.size() && !blank(name[begin + n])) die("the word ends early");
        if (n == 0 && begin != name.size()) die("an empty word ahead of text");
    }
    size_t begin, n;
    issl::first_word(nullptr, 0, begin, n);
    if (begin != 0 || n != 0) die("empty name");
}

static void check_spans(std::mt19937_64 &rng)
{
    for (int round = 0; round < 20000; ++round) {
        const size_t len = rng() % 64;
        std::vector<char> text(len); // (exactly len bytes: a read past them is a report)
        for (char &c : text) c = ",;\"a b\t|\n"[rng() % 9];
        std::vector<issl_text_span> in(rng() % 9);
        bool all_inside = true;
        size_t first_bad = 0;
        for (size_t i = 0; i < in.size(); ++i) {
            issl_text_span s{0, 0, 0};
            switch (rng() % 6) {
            case 0: s.length = 0xFFFFFFFFu; s.offset = rng(); break;                 // '?': the offset is not looked at
            case 1: s.offset = rng() % (len + 3); s.length = static_cast<uint32_t>(rng() % (len + 3)); break;
            case 2: s.offset = ~0ull - rng() % 4; s.length = static_cast<uint32_t>(rng() % 8); break; // offset + length wraps
            default: s.offset = len ? rng() % len : 0; s.length = static_cast<uint32_t>(len ? rng() % (len - s.offset + 1) : 0); break;
            }
            const bool inside = s.length == 0xFFFFFFFFu || (s.offset <= len && s.length <= len - s.offset);
            if (!inside && all_inside) { all_inside = false; first_bad = i; }
            in[i] = s;
        }
        const char d = ",\t;| "[rng() % 5];
        issl::ResultPool pool;
        pool.fixed_len = len;
        std::vector<issl_text_span> out;
        size_t bad = ~size_t(0);
        const bool ok = issl::results_ss_spans(text.data(), len, in.data(), in.size(), d, pool, out, &bad);
        if (ok != all_inside) die("a span outside the text passes, or one inside is refused");
        if (!ok) {
            if (bad != first_bad) die("the wrong span is reported");
            continue;
        }
        for (size_t i = 0; i < in.size(); ++i) {
            if (in[i].length == 0xFFFFFFFFu) { if (out[i].length != 0xFFFFFFFFu) die("'?' lost"); continue; }
            std::string want;
            issl::csv_append(text.data() + in[i].offset, in[i].length, d, want);
            if (out[i].length != want.size() || out[i].offset + out[i].length > len + pool.extra.size()) die("span outside the pool");
            const char *src = out[i].offset >= len ? pool.extra.data() + (out[i].offset - len) : text.data() + out[i].offset;
            if (out[i].offset < len && out[i].offset + out[i].length > len) die("span across the pool's two parts");
            if (std::memcmp(src, want.data(), want.size()) != 0) die("span text");
        }
        issl_text_span own;
        if (!pool.add("x,\"y\"", 6, d, own) || own.offset + own.length != len + pool.extra.size()) die("pool.add");
    }
}

static std::string repr_of(double v)
{
    char buf[40];
    issl::WriteSink s{buf};
    issl::put_repr(s, v, issl_repr_pow10);
    const size_t n = static_cast<size_t>(s.p - buf);
    if (n == 0 || n > issl::kReprMax) die("repr length");
    issl::CountSink c;
    issl::put_repr(c, v, issl_repr_pow10);
    if (c.n != n) die("the counting sink disagrees with the writing one");
    return std::string(buf, n);
}

static void check_repr_value(double v)
{
    const std::string r = repr_of(v);
    if (std::isnan(v)) { if (r != "nan") die("nan", r); return; }
    if (std::isinf(v)) { if (r != (v > 0 ? "inf" : "-inf")) die("inf", r); return; }
    const double back = std::strtod(r.c_str(), nullptr);
    if (std::memcmp(&back, &v, 8) != 0) die("does not read back:", r);
    if (v == 0) { if (r != (std::signbit(v) ? "-0.0" : "0.0")) die("zero", r); return; }
    // digits: no more than the shortest "%.*e" that reads back, and the same ones
    size_t digits = 0;
    std::string mine;
    for (const char c : r) {
        if (c == 'e') break;
        if (c >= '0' && c <= '9') mine.push_back(c);
    }
    while (mine.size() > 1 && mine[0] == '0') mine.erase(0, 1);
    while (mine.size() > 1 && mine.back() == '0') mine.pop_back();
    digits = mine.size();
    for (int p = 0; p < 17; ++p) {
        char buf[48];
        std::snprintf(buf, sizeof buf, "%.*e", p, v);
        const double b = std::strtod(buf, nullptr);
        if (std::memcmp(&b, &v, 8) != 0) continue;
        std::string theirs;
        for (const char *c = buf; *c && *c != 'e'; ++c)
            if (*c >= '0' && *c <= '9') theirs.push_back(*c);
        while (theirs.size() > 1 && theirs.back() == '0') theirs.pop_back();
        if (digits > theirs.size()) die("more digits than needed:", r + " vs " + buf);
        if (digits == theirs.size() && mine != theirs) die("not the closest of the shortest:", r + " vs " + buf);
        break;
    }
    const double a = std::fabs(v);
    const bool fixed = a >= 1e-4 && a < 1e16;
    if (fixed != (r.find('e') == std::string::npos)) die("notation", r);
    if (fixed && r.find('.') == std::string::npos) die("no point", r);
}

static void check_numbers(std::mt19937_64 &rng)
{
    for (int e = -1074; e < 1024; ++e) check_repr_value(std::ldexp(1.0, e));
    for (int e = -323; e < 309; ++e) {
        char buf[16];
        std::snprintf(buf, sizeof buf, "1e%d", e);
        const double p = std::strtod(buf, nullptr);
        check_repr_value(p);
        check_repr_value(std::nextafter(p, INFINITY));
        check_repr_value(std::nextafter(p, 0.0));
    }
    const double special[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 5e-324, 1.7976931348623157e308, 9007199254740993.0, 1e-4, 1e16, 0.1, 100.0, 45.0, -1.0};
    for (const double v : special) check_repr_value(v);
    for (int i = 0; i < 100000; ++i) {
        const uint64_t bits = rng();
        double v;
        std::memcpy(&v, &bits, 8);
        check_repr_value(v);
    }
    if (repr_of(9007199254740993.0) != "9007199254740992.0" || repr_of(5e-324) != "5e-324" || repr_of(1e16) != "1e+16" ||
        repr_of(1e-4) != "0.0001" || repr_of(5e-6) != "5e-06" || repr_of(-1.0) != "-1.0" || repr_of(1e22) != "1e+22")
        die("a known repr");
    std::uniform_real_distribution<double> score(0.0, 100.0), tiny(0.0, 1e-5);
    for (int i = 0; i < 100000; ++i) {
        const double x = i % 3 == 2 ? tiny(rng) : i % 3 == 1 ? std::round(score(rng) * 1e6 + 0.5) / 1e6 - 0.5e-6 : score(rng);
        char buf[400];
        std::snprintf(buf, sizeof buf, "%f", x);
        const double want = std::strtod(buf, nullptr), got = issl::through_text(x);
        if (std::memcmp(&want, &got, 8) != 0) die("through_text", buf);
    }
    const double ties[] = {1.0 / 128, 3.0 / 128, 0.5e-6, 1.5e-6, 2.5e-6, 99.9999995, 4e-7, 5e-7};
    for (const double x : ties) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "%f", x);
        if (issl::through_text(x) != std::strtod(buf, nullptr)) die("through_text on a tie", buf);
    }
    if (issl::through_text(-1.0) != -1.0 || !std::isnan(issl::through_text(NAN)) || issl::through_text(1e300) != 1e300) die("values passed through");
    for (uint64_t v : {0ull, 9ull, 10ull, 99999999ull, 100000000ull, 9999999999999999ull, 10000000000000000ull, 18446744073709551615ull}) {
        char buf[32], want[32];
        issl::WriteSink s{buf};
        issl::put_u64(s, v);
        std::snprintf(want, sizeof want, "%llu", static_cast<unsigned long long>(v));
        if (std::string(buf, static_cast<size_t>(s.p - buf)) != want) die("put_u64", want);
    }
}

int main()
{
    std::mt19937_64 rng(20261019);
    check_quoting(rng);
    check_first_word(rng);
    check_spans(rng);
    check_numbers(rng);
    std::printf("ok\n");
    return 0;
}
