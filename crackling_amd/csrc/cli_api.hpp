// What the executables that load libissl_hip.so with dlopen share (cli_score.cpp, cli_report.cpp, cli_locate.cpp,
// cli_guides.cpp, cli_bowtie.cpp, cli_transcripts.cpp): the search for the library, the symbols the executable needs, the
// ABI check, the way out with a message, reading a text file and writing stdout in pieces.  Host code, no HIP.
//
// Before the include the executable defines
//   ISSL_CLI_NAME     its name in the loader's messages ("isslScoreOfftargets")
//   ISSL_CLI_API(X)   the entry points it calls, X(issl_last_error) X(issl_abi_version) first: it fails on the first
//                     one of its own list the library lacks, and on no other
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <dlfcn.h>
#include <unistd.h>

#include "../../include/issl_hip.h"

namespace {

struct Api {
#define X(f) decltype(&::f) f = nullptr;
    ISSL_CLI_API(X)
#undef X
};
Api api;

// Loads libissl_hip.so: $ISSL_LIBRARY, then ../crackling_amd/, ./ and ../lib/ next to the executable, then the loader's
// path.  false + message on stderr when it cannot be had, lacks a symbol or has another ABI (the caller exits 1).
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
        std::fprintf(stderr, ISSL_CLI_NAME ": cannot load libissl_hip.so (set ISSL_LIBRARY):\n");
        for (const auto &t : tried) std::fprintf(stderr, "  %s\n", t.c_str());
        return false;
    }
#define X(f)                                                                                                              \
    api.f = reinterpret_cast<decltype(api.f)>(::dlsym(h, #f));                                                            \
    if (!api.f) { std::fprintf(stderr, ISSL_CLI_NAME ": libissl_hip.so lacks %s (another version of the library?)\n", #f); return false; }
    ISSL_CLI_API(X)
#undef X
    if (api.issl_abi_version() != ISSL_ABI_VERSION) {
        std::fprintf(stderr, ISSL_CLI_NAME ": libissl_hip.so has ABI %d, this executable was built for %d\n", api.issl_abi_version(), ISSL_ABI_VERSION);
        return false;
    }
    return true;
}

// The message the failed library call left, or `fallback` when it left none.
inline std::string last_error(const char *fallback)
{
    const char *e = api.issl_last_error ? api.issl_last_error() : nullptr;
    return (e && e[0]) ? e : fallback;
}

// The way out of main after a failed library call: its message on stderr, exit status 1.
inline int fail(const char *fallback)
{
    std::fprintf(stderr, "%s\n", last_error(fallback).c_str());
    return 1;
}

// The whole file appended to `text`; false when it cannot be opened or read.
inline bool read_text_file(const char *path, std::string &text)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return false;
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, k);
    const bool ok = !std::ferror(fp);
    std::fclose(fp);
    return ok;
}

// stdout in pieces of 1 MiB: the lines are appended to `text`, wrote() after each hands a full piece on, finish() the rest.
// Both return false once a write came up short ("short write on stdout" is the caller's to print).
struct StdoutText {
    std::string text;
    bool wrote(bool all = false)
    {
        if (text.size() < (size_t(1) << 20) && !all) return true;
        const bool ok = std::fwrite(text.data(), 1, text.size(), stdout) == text.size();
        text.clear();
        return ok;
    }
    bool finish() { return wrote(true) && std::fflush(stdout) == 0; }
};

} // namespace
