// GFF3 text -> AnnotationTables: loadAnnotation of src/crackling/utils/countHitTranscripts.py:45-146, quirks included
// (include/issl_hip.h lists them).  Plain C++ ahead of any device call.
#include "issl_annotation.hpp"

#include <algorithm>
#include <unordered_map>

#include "issl_host.hpp"

namespace issl {

namespace {

// what Python's str.strip() removes among ASCII characters
inline bool py_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

struct Span {
    const char *p;
    size_t n;
    std::string str() const { return std::string(p, n); }
    bool is(const char *lit) const { return std::char_traits<char>::length(lit) == n && std::equal(p, p + n, lit); }
};

Span strip(const char *b, const char *e)
{
    while (b < e && py_space(static_cast<unsigned char>(*b))) ++b;
    while (e > b && py_space(static_cast<unsigned char>(e[-1]))) --e;
    return {b, static_cast<size_t>(e - b)};
}

int bad_line(size_t line_no, const std::string &what)
{
    set_error("annotation line " + std::to_string(line_no) + ": " + what);
    return ISSL_E_FORMAT;
}

} // namespace

bool parse_int64(const char *s, size_t n, int64_t &v)
{
    size_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    if (i == n) return false;
    uint64_t mag = 0;
    const uint64_t limit = neg ? (uint64_t(1) << 63) : (uint64_t(1) << 63) - 1;
    for (; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = static_cast<uint64_t>(s[i] - '0');
        if (mag > (limit - d) / 10) return false;
        mag = mag * 10 + d;
    }
    v = neg ? static_cast<int64_t>(0 - mag) : static_cast<int64_t>(mag);
    return true;
}

int parse_annotation(const char *text, size_t len, AnnotationTables &out)
{
    out = AnnotationTables();
    std::unordered_map<std::string, uint32_t> seq_index, tr_index, gene_index, mrna_gene;
    std::vector<std::string> tr_id;
    const char *p = text, *const end = text + len;
    size_t line_no = 0;
    auto transcript = [&](uint32_t seq, const std::string &id) -> uint32_t {
        std::string key = id;
        key += '\t'; // no field holds a TAB
        key += std::to_string(seq);
        const auto it = tr_index.find(key);
        if (it != tr_index.end()) return it->second;
        const uint32_t k = static_cast<uint32_t>(tr_id.size());
        tr_index.emplace(std::move(key), k);
        tr_id.push_back(id);
        out.tr_seq.push_back(seq);
        return k;
    };
    while (p < end) {
        // universal newlines: "\n", "\r\n" or a lone "\r"
        const char *e = p;
        while (e < end && *e != '\n' && *e != '\r') ++e;
        const char *next = e;
        if (next < end) next += (*next == '\r' && next + 1 < end && next[1] == '\n') ? 2 : 1;
        ++line_no;
        Span f[9];
        size_t nf = 0;
        const char *b = p;
        for (const char *c = p;; ++c) {
            if (c == e || *c == '\t') {
                if (nf < 9) f[nf] = strip(b, c);
                ++nf;
                b = c + 1;
                if (c == e) break;
            }
        }
        p = next;
        if (nf != 9) continue;
        // attributes: key = text ahead of the first '=', value = text between the first and the second; the last key wins
        bool has_id = false, has_parent = false;
        Span id{nullptr, 0}, parent{nullptr, 0};
        const char *ab = f[8].p, *const ae = f[8].p + f[8].n;
        for (const char *c = ab;; ++c) {
            if (c == ae || *c == ';') {
                const char *eq = std::find(ab, c, '=');
                if (eq == c) return bad_line(line_no, "attribute '" + std::string(ab, c) + "' has no '='");
                const char *eq2 = std::find(eq + 1, c, '=');
                const Span key{ab, static_cast<size_t>(eq - ab)}, val{eq + 1, static_cast<size_t>(eq2 - eq - 1)};
                if (key.is("ID")) has_id = true, id = val;
                else if (key.is("Parent")) has_parent = true, parent = val;
                ab = c + 1;
                if (c == ae) break;
            }
        }
        if (!has_id || !has_parent) continue;
        const bool is_gene = f[2].is("gene"), is_mrna = f[2].is("mRNA"), is_exon = f[2].is("exon");
        if (!is_gene && !is_mrna && !is_exon) continue;
        std::string name = f[0].str();
        std::replace(name.begin(), name.end(), '.', '_');
        uint32_t seq;
        const auto it = seq_index.find(name);
        if (it != seq_index.end()) {
            seq = it->second;
        } else {
            seq = static_cast<uint32_t>(out.seqs.size());
            seq_index.emplace(name, seq);
            out.seqs.push_back(std::move(name));
        }
        if (is_mrna) {
            const std::string sid = id.str(), sparent = parent.str();
            (void)transcript(seq, sid);
            auto g = gene_index.find(sparent);
            if (g == gene_index.end()) {
                g = gene_index.emplace(sparent, static_cast<uint32_t>(out.gene_count.size())).first;
                out.gene_count.push_back(0);
            }
            ++out.gene_count[g->second];
            mrna_gene.emplace(sid, g->second); // the first mRNA line with this ID wins
        } else if (is_exon) {
            const uint32_t tr = transcript(seq, parent.str());
            int64_t s, t;
            if (!parse_int64(f[3].p, f[3].n, s)) return bad_line(line_no, "exon start '" + f[3].str() + "' is not an integer");
            if (!parse_int64(f[4].p, f[4].n, t)) return bad_line(line_no, "exon end '" + f[4].str() + "' is not an integer");
            out.exons.push_back({seq, tr, s, t});
        }
    }
    out.tr_gene.resize(tr_id.size());
    for (size_t k = 0; k < tr_id.size(); ++k) {
        const auto it = mrna_gene.find(tr_id[k]);
        out.tr_gene[k] = it == mrna_gene.end() ? kNoGene : it->second;
    }
    return ISSL_OK;
}

int annotation_intervals(const AnnotationTables &t, AnnotationIntervals &out)
{
    out = AnnotationIntervals();
    if (t.seqs.size() >= kMaxSeqs) {
        set_error("annotation with " + std::to_string(t.seqs.size()) + " sequences: a breakpoint key holds fewer than 2^24");
        return ISSL_E_UNSUPPORTED;
    }
    struct Ivl {
        uint32_t tr;
        int64_t start, end;
    };
    std::vector<Ivl> v;
    v.reserve(t.exons.size());
    for (const AnnotationExon &x : t.exons) {
        if (x.start > x.end || x.end < 0) continue; // contains nothing / nothing at or above 0
        if (x.end > kMaxCoord) {                    // start <= end: the start is in range when the end is
            set_error("exon " + std::to_string(x.start) + ".." + std::to_string(x.end) + ": coordinates above 2^40 - 2 are not supported");
            return ISSL_E_UNSUPPORTED;
        }
        v.push_back({x.transcript, std::max<int64_t>(x.start, 0), x.end});
    }
    std::sort(v.begin(), v.end(), [](const Ivl &a, const Ivl &b) { return a.tr != b.tr ? a.tr < b.tr : a.start < b.start; });
    auto flush = [&](const Ivl &c) {
        const uint64_t base = static_cast<uint64_t>(t.tr_seq[c.tr]) << kCoordBits;
        out.lo.push_back(base | static_cast<uint64_t>(c.start));
        out.hi.push_back(base | static_cast<uint64_t>(c.end + 1));
        out.tr.push_back(c.tr);
    };
    for (size_t i = 0; i < v.size();) {
        Ivl c = v[i++];
        for (; i < v.size() && v[i].tr == c.tr && v[i].start <= c.end; ++i) c.end = std::max(c.end, v[i].end);
        flush(c);
    }
    if (out.tr.size() >= (uint64_t(1) << 31)) {
        set_error("annotation with 2^31 exon intervals or more");
        return ISSL_E_UNSUPPORTED;
    }
    return ISSL_OK;
}

} // namespace issl
