// bin/isslLocateOfftargets -- where the sites of a list lie in the genome:
//
//   isslLocateOfftargets [--report] <sites file> <FASTA ...|directory>
//
// The sites file follows the scorer's query-file rules (issl_read_query_file: 20 characters and a line end per line); with
// --report it is the TSV bin/isslReportOfftargets prints and the site is its second field.  Distinct sites are located
// once and printed in the order of their first appearance, one line per location, a site's locations by record, position
// and strand:
//   <site 20-mer>\t<record name>\t<pos>\t<+|->\n
// pos is 0-based inside the record; '-' is a match of the reverse pattern, whose site is the reverse complement of the
// first 20 of the 23 matched characters (include/issl_hip.h, issl_genome_*).  A site without a location prints nothing.
// The FASTA arguments follow bin/extractOfftargets: one input or several, a lone directory stands for its non-hidden
// entries.  stdout carries data only, diagnostics go to stderr, exit status 1 on any error.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslReportOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "isslLocateOfftargets"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_read_query_file) X(issl_free) X(issl_encode_guides) X(issl_decode_guide)  \
    X(issl_genome_open_files) X(issl_genome_info) X(issl_genome_record) X(issl_genome_locate) X(issl_genome_close)
#include "cli_api.hpp"

namespace {

// The second field of every line of an isslReportOfftargets TSV, packed.  false: the file is no such TSV.
bool read_report_sites(const char *path, std::vector<uint64_t> &sites)
{
    std::string text;
    if (!read_text_file(path, text)) {
        std::fprintf(stderr, "cannot open '%s'\n", path);
        return false;
    }
    std::string packed; // the 20-mers one after the other
    size_t line = 0;
    for (size_t p = 0; p < text.size(); ++line) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        const size_t t1 = text.find('\t', p);
        const size_t t2 = t1 == std::string::npos || t1 >= e ? std::string::npos : text.find('\t', t1 + 1);
        if (t2 == std::string::npos || t2 > e || t2 - t1 - 1 != 20) {
            std::fprintf(stderr, "'%s' line %zu: not a line of isslReportOfftargets (a 20-character site as second field)\n", path, line + 1);
            return false;
        }
        packed.append(text, t1 + 1, 20);
        p = e + 1;
    }
    sites.resize(packed.size() / 20);
    return sites.empty() || api.issl_encode_guides(packed.data(), sites.size(), 20, 20, sites.data()) == 0;
}

} // namespace

int main(int argc, char **argv)
{
    bool report = false;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--report")) report = true;
        else pos.push_back(argv[i]);
    }
    if (pos.size() < 2) {
        std::fprintf(stderr, "Usage: %s [--report] <sites file> <FASTA ...|directory>\n", argv[0]);
        return 1;
    }
    if (!load_api()) return 1;
    // the sites file first, then the genome and the device
    std::vector<uint64_t> sites;
    if (report) {
        if (!read_report_sites(pos[0], sites)) return 1;
    } else {
        uint64_t *q = nullptr;
        size_t n = 0;
        if (api.issl_read_query_file(pos[0], 20, &q, &n)) return fail("cannot read sites file");
        sites.assign(q, q + n);
        api.issl_free(q);
    }
    std::vector<uint64_t> distinct;
    {
        std::unordered_set<uint64_t> seen;
        for (uint64_t s : sites)
            if (seen.insert(s).second) distinct.push_back(s);
    }
    const char *dev = std::getenv("ISSL_DEVICE");
    issl_genome *g = nullptr;
    if (api.issl_genome_open_files(pos.data() + 1, static_cast<int>(pos.size() - 1), dev ? std::atoi(dev) : 0, &g)) return fail("cannot open genome");
    std::vector<uint64_t> offsets(distinct.size() + 1);
    std::vector<issl_location> locs;
    size_t total = 0;
    if (api.issl_genome_locate(g, distinct.data(), distinct.size(), offsets.data(), nullptr, 0, &total)) return fail("locate failed");
    if (total) {
        locs.resize(total);
        if (api.issl_genome_locate(g, distinct.data(), distinct.size(), offsets.data(), locs.data(), locs.size(), &total)) return fail("locate failed");
    }
    StdoutText so;
    std::string &out = so.text;
    char site[64], buf[64];
    bool ok = true;
    for (size_t k = 0; ok && k < distinct.size(); ++k) {
        if (offsets[k] == offsets[k + 1]) continue;
        if (api.issl_decode_guide(distinct[k], 20, site)) return fail("cannot decode site");
        for (uint64_t j = offsets[k]; j < offsets[k + 1]; ++j) {
            const char *name = nullptr;
            size_t name_len = 0;
            uint64_t length = 0;
            if (api.issl_genome_record(g, locs[j].record, &name, &name_len, &length)) return fail("record out of range");
            out += site;
            out += '\t';
            out.append(name, name_len);
            std::snprintf(buf, sizeof buf, "\t%llu\t%c\n", static_cast<unsigned long long>(locs[j].pos), locs[j].strand ? '-' : '+');
            out += buf;
        }
        ok = so.wrote();
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    api.issl_genome_close(g);
    return 0;
}
