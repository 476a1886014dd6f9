// Host-side text handling of the result table (issl_results.cpp): the free-text fields -- header names, chromosome names,
// RNAfold's lines -- are checked and CSV-quoted here, once per distinct text, into the pool the kernels copy from.  Plain
// C++, no device code: tools/results_sanitize.cpp runs it under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"

namespace issl {

inline bool results_delimiter_ok(char d) { return d == ',' || d == '\t' || d == ';' || d == '|' || d == ' '; }

// csv.QUOTE_MINIMAL: a field with the delimiter, the quote character or a line end in it is quoted.
inline bool csv_needs_quotes(const char *p, size_t len, char delimiter)
{
    for (size_t i = 0; i < len; ++i)
        if (p[i] == delimiter || p[i] == '"' || p[i] == '\n' || p[i] == '\r') return true;
    return false;
}

// The field as the writer prints it, appended to out.
inline void csv_append(const char *p, size_t len, char delimiter, std::string &out)
{
    if (!csv_needs_quotes(p, len, delimiter)) {
        out.append(p, len);
        return;
    }
    out.push_back('"');
    for (size_t i = 0; i < len; ++i) {
        if (p[i] == '"') out.push_back('"');
        out.push_back(p[i]);
    }
    out.push_back('"');
}

// A record's name as Bowtie2 prints it: up to the first blank (bytes.split() of Python: space, TAB, LF, VT, FF, CR).
// -> the word is p[begin .. begin + n); n == 0 for a name of blanks only.
inline void first_word(const char *p, size_t len, size_t &begin, size_t &n)
{
    auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; };
    size_t b = 0;
    while (b < len && blank(p[b])) ++b; // (split() skips leading blanks: the first word, not an empty one)
    size_t e = b;
    while (e < len && !blank(p[e])) ++e;
    begin = b;
    n = e - b;
}

// The pool behind a table's text spans: `fixed` bytes that are uploaded as they stand (RNAfold's text) followed by `extra`,
// what had to be rewritten or is the library's own.  Offsets of spans count from the start of `fixed`.
struct ResultPool {
    uint64_t fixed_len = 0;
    std::string extra;
    // A text of the library's own, quoted as needed; false when its quoted form does not fit a span's 32 bits.
    bool add(const char *p, size_t len, char delimiter, issl_text_span &s)
    {
        s = issl_text_span{fixed_len + extra.size(), 0, 0};
        csv_append(p, len, delimiter, extra);
        const uint64_t n = fixed_len + extra.size() - s.offset;
        s.length = static_cast<uint32_t>(n);
        return n < 0xFFFFFFFFull;
    }
};

// The caller's spans into ss_text[0 .. ss_len) -> spans into the pool: a span that needs no quotes stays where it is, one
// that does is rewritten into pool.extra.  False (with `bad` = the span's index) for a span that leaves the text or whose
// quoted form does not fit 32 bits.
inline bool results_ss_spans(const char *ss_text, uint64_t ss_len, const issl_text_span *in, size_t n, char delimiter,
                             ResultPool &pool, std::vector<issl_text_span> &out, size_t *bad)
{
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const issl_text_span s = in[i];
        if (s.length == 0xFFFFFFFFu) {
            out[i] = issl_text_span{0, 0xFFFFFFFFu, 0};
            continue;
        }
        if (s.offset > ss_len || s.length > ss_len - s.offset) {
            *bad = i;
            return false;
        }
        if (!csv_needs_quotes(ss_text + s.offset, s.length, delimiter)) {
            out[i] = issl_text_span{s.offset, s.length, 0};
            continue;
        }
        const uint64_t at = pool.fixed_len + pool.extra.size();
        csv_append(ss_text + s.offset, s.length, delimiter, pool.extra);
        const uint64_t len = pool.fixed_len + pool.extra.size() - at;
        if (len >= 0xFFFFFFFFull) {
            *bad = i;
            return false;
        }
        out[i] = issl_text_span{at, static_cast<uint32_t>(len), 0};
    }
    return true;
}

// The header row of Crackling.py:268 for `delimiter` (no name holds one of the five delimiters or a quote).
inline std::string results_header_row(char delimiter)
{
    static const char *const names[26] = {"seq", "sgrnascorer2score", "header", "start", "end", "strand", "isUnique", "passedG20",
                                          "passedTTTT", "passedATPercent", "passedSecondaryStructure", "ssL1", "ssStructure", "ssEnergy",
                                          "acceptedByMm10db", "acceptedBySgRnaScorer", "consensusCount", "passedBowtie",
                                          "passedOffTargetScore", "AT", "bowtieChr", "bowtieStart", "bowtieEnd", "mitOfftargetscore",
                                          "cfdOfftargetscore", "passedAvoidLeadingT"};
    std::string row;
    for (int i = 0; i < 26; ++i) {
        if (i) row.push_back(delimiter);
        row += names[i];
    }
    row.push_back('\n');
    return row;
}

} // namespace issl
