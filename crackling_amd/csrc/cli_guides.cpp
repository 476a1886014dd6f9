// bin/cracklingGuides -- the candidate guides of FASTA inputs, as Crackling's extraction step finds them
// (src/crackling/Crackling.py:151-305):
//
//   cracklingGuides [--unique] <FASTA ...|directory>
//
// One line per distinct 23-mer, in the order the reference first meets it:
//   <target23>\t<header>\t<start>\t<end>\t<+|->\t<isUnique>\n
// start is 0-based inside the record, end = start + 23, '-' is a match of the reverse pattern (the guide is the reverse
// complement of the matched characters).  A guide seen more than once has isUnique 0 and '-' for header, start, end and
// strand -- the row the reference keeps but never scores; --unique drops these rows.  The inputs are read in the order
// given; a lone directory stands for the files in it in reverse sorted name order (include/issl_hip.h, issl_guides_*).
// stdout carries data only, diagnostics go to stderr, exit status 1 on any error; any other argument that starts with "--"
// is answered with the usage line (a file of such a name: ./--name).
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslLocateOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "cracklingGuides"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_decode_guide) X(issl_guides_extract_files) X(issl_guides_info)            \
    X(issl_guides_record) X(issl_guides_copy) X(issl_guides_close)
#include "cli_api.hpp"

namespace {

// The set released on every way out of main.
struct SetCloser {
    issl_guide_set *&g;
    ~SetCloser() { if (g) api.issl_guides_close(g); }
};

} // namespace

int main(int argc, char **argv)
{
    bool only_unique = false, bad_option = false;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--unique")) only_unique = true;
        else if (!std::strncmp(argv[i], "--", 2)) bad_option = true;
        else pos.push_back(argv[i]);
    }
    if (pos.empty() || bad_option) {
        std::fprintf(stderr, "Usage: %s [--unique] <FASTA ...|directory>\n", argv[0]);
        return 1;
    }
    if (!load_api()) return 1;
    const char *dev = std::getenv("ISSL_DEVICE");
    issl_guide_set *g = nullptr;
    SetCloser closer{g};
    if (api.issl_guides_extract_files(pos.data(), static_cast<int>(pos.size()), dev ? std::atoi(dev) : 0, &g)) return fail("extraction failed");
    uint64_t n_guides = 0, n_unique = 0, n_matches = 0, n_records = 0;
    if (api.issl_guides_info(g, &n_guides, &n_unique, &n_matches, &n_records)) return fail("no guide set");
    std::vector<issl_guide> guides(n_guides);
    if (api.issl_guides_copy(g, guides.data(), guides.size())) return fail("cannot copy the guides");
    StdoutText so;
    std::string &out = so.text;
    char seq[64], buf[96];
    bool ok = true;
    for (size_t k = 0; ok && k < guides.size(); ++k) {
        const issl_guide &gd = guides[k];
        if (gd.seen != 1 && only_unique) continue;
        if (api.issl_decode_guide(gd.guide23, 23, seq)) return fail("cannot decode guide");
        out += seq;
        if (gd.seen == 1) {
            const char *name = nullptr;
            size_t name_len = 0;
            uint64_t length = 0;
            if (api.issl_guides_record(g, gd.record, &name, &name_len, &length)) return fail("record out of range");
            out += '\t';
            out.append(name, name_len);
            std::snprintf(buf, sizeof buf, "\t%llu\t%llu\t%c\t1\n", static_cast<unsigned long long>(gd.start),
                          static_cast<unsigned long long>(gd.start + 23), gd.strand ? '-' : '+');
            out += buf;
        } else {
            out += "\t-\t-\t-\t-\t0\n";
        }
        ok = so.wrote();
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    return 0;
}
