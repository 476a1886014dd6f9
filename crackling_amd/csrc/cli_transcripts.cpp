// bin/countHitTranscripts -- the console script of src/crackling/utils/countHitTranscripts.py:
//
//   countHitTranscripts --annotation|-a FILE --crackling|-c FILE --output|-o FILE
//
// FILE of -a is a GFF3 annotation, FILE of -c Crackling's output file; the output is that file with a `hits` column appended,
// "<transcripts hit>/<transcripts of the gene>" for the row's bowtieChr and bowtieStart, byte for byte what the reference
// writes (include/issl_hip.h, "transcript hit counts", states the rules).  The reference's --sample is not offered: the
// sample is a test fixture.  The reference also leaves <annotation>.p beside the GFF; nothing is written there.
//
// The CSV side is host code with the semantics of Python's csv module as the reference uses it: the file is read with
// universal newlines ("\r\n" and a lone "\r" become "\n", inside quoted fields too), parsed by
// csv.reader(delimiter=',', quotechar='"') -- doubled quotes inside a quoted field, text after a closing quote joins the
// field, an unfinished quoted field ends with the file, a blank line is a row without fields -- and written with the unix
// dialect and QUOTE_MINIMAL: a field is quoted when it holds a comma, a quote or a line break, quotes are doubled, a row
// of one empty field is written as "", every row ends in "\n".  Names are looked up on the host, all rows go to the
// device in one call.
//
// Where the reference dies with a traceback -- an attribute without '=', an exon coordinate that is no integer, a header
// without seq, bowtieChr, bowtieStart or bowtieEnd, a row too short for those columns, a bowtieStart or bowtieEnd that is no
// integer on a row whose bowtieChr is not '?' (an optional sign and ASCII digits within int64 here; Python's int() takes
// more) -- the executable prints a message on stderr, exits with status 1 and writes no output file.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as cracklingBowtie does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "countHitTranscripts"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_annotation_open_file) X(issl_annotation_lookup) X(issl_annotation_hits) \
    X(issl_annotation_close)
#include "cli_api.hpp"

namespace {

// This executable's messages carry its name, the library's included.
int fail_with(const std::string &message)
{
    std::fprintf(stderr, "countHitTranscripts: %s\n", message.c_str());
    return 1;
}

// "\r\n" and a lone "\r" -> "\n": what Python's text mode hands the csv module.
std::string universal_newlines(const std::string &in)
{
    std::string out;
    out.reserve(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
        if (in[i] == '\r') {
            out += '\n';
            if (i + 1 < in.size() && in[i + 1] == '\n') ++i;
        } else {
            out += in[i];
        }
    }
    return out;
}

using Row = std::vector<std::string>;

// csv.reader(delimiter=',', quotechar='"') over the lines of `text` (doublequote, not strict, no escape character).
std::vector<Row> read_csv(const std::string &text)
{
    enum State { START_RECORD, START_FIELD, IN_FIELD, IN_QUOTED, QUOTE_IN_QUOTED, EAT_NL };
    std::vector<Row> rows;
    Row row;
    std::string field;
    State st = START_RECORD;
    bool open_record = false; // a record continues over a line end (inside a quoted field)
    auto save = [&] { row.push_back(field); field.clear(); };
    size_t i = 0;
    while (i < text.size()) {
        size_t e = text.find('\n', i);
        const size_t line_end = e == std::string::npos ? text.size() : e + 1;
        for (; i < line_end; ++i) {
            const char c = text[i];
            const bool nl = c == '\n';
            switch (st) {
            case START_RECORD:
                if (nl) { st = EAT_NL; break; }
                st = START_FIELD;
                [[fallthrough]];
            case START_FIELD:
                if (nl) { save(); st = EAT_NL; }
                else if (c == '"') st = IN_QUOTED;
                else if (c == ',') save();
                else { field += c; st = IN_FIELD; }
                break;
            case IN_FIELD:
                if (nl) { save(); st = EAT_NL; }
                else if (c == ',') { save(); st = START_FIELD; }
                else field += c;
                break;
            case IN_QUOTED:
                if (c == '"') st = QUOTE_IN_QUOTED;
                else field += c;
                break;
            case QUOTE_IN_QUOTED:
                if (c == '"') { field += c; st = IN_QUOTED; }
                else if (c == ',') { save(); st = START_FIELD; }
                else if (nl) { save(); st = EAT_NL; }
                else { field += c; st = IN_FIELD; }
                break;
            case EAT_NL:
                break; // a line holds one line end, at its end
            }
        }
        // the end of the line
        switch (st) {
        case START_FIELD:
        case IN_FIELD:
        case QUOTE_IN_QUOTED:
            save();
            st = START_RECORD;
            break;
        case EAT_NL:
            st = START_RECORD;
            break;
        default:
            break;
        }
        open_record = st != START_RECORD;
        if (!open_record) {
            rows.push_back(std::move(row));
            row.clear();
        }
    }
    if (open_record) { // the file ends inside a quoted field
        save();
        rows.push_back(std::move(row));
    }
    return rows;
}

// csv.writer(dialect='unix', quoting=QUOTE_MINIMAL).writerow
void write_row(const Row &row, std::string &out)
{
    if (row.size() == 1 && row[0].empty()) {
        out += "\"\"\n";
        return;
    }
    for (size_t k = 0; k < row.size(); ++k) {
        if (k) out += ',';
        const std::string &f = row[k];
        if (f.find_first_of(",\"\n\r") == std::string::npos) {
            out += f;
        } else {
            out += '"';
            for (const char c : f) {
                if (c == '"') out += '"';
                out += c;
            }
            out += '"';
        }
    }
    out += '\n';
}

bool to_int64(const std::string &s, long long &v)
{
    size_t i = 0;
    bool neg = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    if (i == s.size()) return false;
    unsigned long long mag = 0;
    const unsigned long long limit = neg ? (1ull << 63) : (1ull << 63) - 1;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        const unsigned long long d = static_cast<unsigned long long>(s[i] - '0');
        if (mag > (limit - d) / 10) return false;
        mag = mag * 10 + d;
    }
    v = neg ? static_cast<long long>(0 - mag) : static_cast<long long>(mag);
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    const char *annotation = nullptr, *crackling = nullptr, *output = nullptr;
    bool usage = false;
    for (int i = 1; i < argc; ++i) {
        const char **dst = nullptr;
        if (!std::strcmp(argv[i], "-a") || !std::strcmp(argv[i], "--annotation")) dst = &annotation;
        else if (!std::strcmp(argv[i], "-c") || !std::strcmp(argv[i], "--crackling")) dst = &crackling;
        else if (!std::strcmp(argv[i], "-o") || !std::strcmp(argv[i], "--output")) dst = &output;
        if (!dst || i + 1 >= argc) { usage = true; break; }
        *dst = argv[++i];
    }
    if (usage || !annotation || !crackling || !output) {
        std::fprintf(stderr, "Usage: %s --annotation|-a FILE --crackling|-c FILE --output|-o FILE\n", argv[0]);
        return 1;
    }
    if (!load_api()) return 1;
    // the annotation first, as the reference does: parsed on the host, then resolved on the device
    const char *dev = std::getenv("ISSL_DEVICE");
    issl_annotation *a = nullptr;
    if (api.issl_annotation_open_file(annotation, dev ? std::atoi(dev) : 0, &a)) return fail_with(last_error("cannot open annotation"));
    std::string raw;
    if (!read_text_file(crackling, raw)) return fail_with(std::string("cannot read '") + crackling + "'");
    std::vector<Row> rows = read_csv(universal_newlines(raw));
    std::vector<uint32_t> seq;
    std::vector<int64_t> start;
    std::vector<size_t> asked; // the rows that go to the device
    if (!rows.empty()) {
        size_t col[4];
        static const char *const names[4] = {"seq", "bowtieChr", "bowtieStart", "bowtieEnd"};
        for (int c = 0; c < 4; ++c) {
            col[c] = 0;
            while (col[c] < rows[0].size() && rows[0][col[c]] != names[c]) ++col[c];
            if (col[c] == rows[0].size()) return fail_with(std::string("the header of '") + crackling + "' has no column " + names[c]);
        }
        rows[0].push_back("hits");
        std::unordered_map<std::string, uint32_t> known;
        for (size_t r = 1; r < rows.size(); ++r) {
            const Row &row = rows[r];
            const std::string where = "row " + std::to_string(r + 1) + " of '" + crackling + "'";
            if (row.size() <= col[1]) return fail_with(where + " has no bowtieChr");
            if (row[col[1]] == "?") continue;
            long long s = 0, e = 0;
            if (row.size() <= col[0] || row.size() <= col[2] || row.size() <= col[3]) return fail_with(where + " is too short");
            if (!to_int64(row[col[2]], s)) return fail_with(where + ": bowtieStart '" + row[col[2]] + "' is not an integer");
            if (!to_int64(row[col[3]], e)) return fail_with(where + ": bowtieEnd '" + row[col[3]] + "' is not an integer");
            auto it = known.find(row[col[1]]);
            if (it == known.end()) {
                uint32_t k = 0;
                if (api.issl_annotation_lookup(a, row[col[1]].data(), row[col[1]].size(), &k)) return fail_with(last_error("lookup failed"));
                it = known.emplace(row[col[1]], k).first;
            }
            seq.push_back(it->second);
            start.push_back(s);
            asked.push_back(r);
        }
    }
    std::vector<issl_transcript_hits> hits(asked.size());
    if (api.issl_annotation_hits(a, seq.data(), start.data(), asked.size(), hits.data())) return fail_with(last_error("hits failed"));
    for (size_t r = 1; r < rows.size(); ++r) rows[r].push_back("?/?");
    for (size_t k = 0; k < asked.size(); ++k)
        if (hits[k].status == 0) rows[asked[k]].back() = std::to_string(hits[k].hit) + "/" + std::to_string(hits[k].total);
    api.issl_annotation_close(a);
    std::string out;
    for (const Row &row : rows) write_row(row, out);
    FILE *fp = std::fopen(output, "wb");
    if (!fp) return fail_with(std::string("cannot write '") + output + "'");
    const bool ok = std::fwrite(out.data(), 1, out.size(), fp) == out.size();
    if (std::fclose(fp) != 0 || !ok) return fail_with(std::string("short write on '") + output + "'");
    return 0;
}
