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
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <dlfcn.h>
#include <unistd.h>

#include "../../include/issl_hip.h"

namespace {

#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_decode_guide) X(issl_guides_extract_files) X(issl_guides_info)            \
    X(issl_guides_record) X(issl_guides_copy) X(issl_guides_close)
struct Api {
#define X(f) decltype(&::f) f = nullptr;
    ISSL_CLI_API(X)
#undef X
};
Api api;

bool load_api()
{
    std::vector<std::string> tried;
    void *h = nullptr;
    auto attempt = [&](const std::string &path) {
        if (h || path.empty()) return;
        h = ::dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) tried.push_back(path + ": " + ::dlerror());
    };
    if (const char *e = std::getenv("ISSL_LIBRARY")) attempt(e);
    char exe[PATH_MAX];
    const ssize_t k = ::readlink("/proc/self/exe", exe, sizeof exe - 1);
    if (k > 0) {
        exe[k] = 0;
        std::string dir(exe);
        dir.erase(dir.find_last_of('/') == std::string::npos ? 0 : dir.find_last_of('/'));
        attempt(dir + "/../crackling_amd/libissl_hip.so");
        attempt(dir + "/libissl_hip.so");
        attempt(dir + "/../lib/libissl_hip.so");
    }
    attempt("libissl_hip.so");
    if (!h) {
        std::fprintf(stderr, "cracklingGuides: cannot load libissl_hip.so (set ISSL_LIBRARY):\n");
        for (const auto &t : tried) std::fprintf(stderr, "  %s\n", t.c_str());
        return false;
    }
#define X(f)                                                                                                              \
    api.f = reinterpret_cast<decltype(api.f)>(::dlsym(h, #f));                                                            \
    if (!api.f) { std::fprintf(stderr, "cracklingGuides: libissl_hip.so lacks %s (another version of the library?)\n", #f); return false; }
    ISSL_CLI_API(X)
#undef X
    if (api.issl_abi_version() != ISSL_ABI_VERSION) {
        std::fprintf(stderr, "cracklingGuides: libissl_hip.so has ABI %d, this executable was built for %d\n", api.issl_abi_version(), ISSL_ABI_VERSION);
        return false;
    }
    return true;
}

// The message of the failed call, the set released: every way out of main closes it.
int fail(const char *what, issl_guide_set *g = nullptr)
{
    const char *e = api.issl_last_error ? api.issl_last_error() : nullptr;
    std::fprintf(stderr, "%s\n", (e && e[0]) ? e : what);
    if (g) api.issl_guides_close(g);
    return 1;
}

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
    if (api.issl_guides_extract_files(pos.data(), static_cast<int>(pos.size()), dev ? std::atoi(dev) : 0, &g)) return fail("extraction failed");
    uint64_t n_guides = 0, n_unique = 0, n_matches = 0, n_records = 0;
    if (api.issl_guides_info(g, &n_guides, &n_unique, &n_matches, &n_records)) return fail("no guide set", g);
    std::vector<issl_guide> guides(n_guides);
    if (api.issl_guides_copy(g, guides.data(), guides.size())) return fail("cannot copy the guides", g);
    std::string out;
    char seq[64], buf[96];
    bool ok = true;
    for (size_t k = 0; ok && k < guides.size(); ++k) {
        const issl_guide &gd = guides[k];
        if (gd.seen != 1 && only_unique) continue;
        if (api.issl_decode_guide(gd.guide23, 23, seq)) return fail("cannot decode guide", g);
        out += seq;
        if (gd.seen == 1) {
            const char *name = nullptr;
            size_t name_len = 0;
            uint64_t length = 0;
            if (api.issl_guides_record(g, gd.record, &name, &name_len, &length)) return fail("record out of range", g);
            out += '\t';
            out.append(name, name_len);
            std::snprintf(buf, sizeof buf, "\t%llu\t%llu\t%c\t1\n", static_cast<unsigned long long>(gd.start),
                          static_cast<unsigned long long>(gd.start + 23), gd.strand ? '-' : '+');
            out += buf;
        } else {
            out += "\t-\t-\t-\t-\t0\n";
        }
        if (out.size() >= (size_t(1) << 20)) {
            ok = std::fwrite(out.data(), 1, out.size(), stdout) == out.size();
            out.clear();
        }
    }
    ok = ok && std::fwrite(out.data(), 1, out.size(), stdout) == out.size() && std::fflush(stdout) == 0;
    api.issl_guides_close(g);
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    return 0;
}
