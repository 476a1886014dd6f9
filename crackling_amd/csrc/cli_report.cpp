// bin/isslReportOfftargets -- the off-target report of every guide of a query file:
//
//   isslReportOfftargets [issltable] [query file] [max distance] [--profile]
//
// Default: one line per off-target, guides in input order, a guide's off-targets in the reference's scoring order
// (isslScoreOfftargets.cpp:330,344: slice, then position in the bucket):
//   <guide 20-mer>\t<site 20-mer>\t<mismatches>\t<occurrences>\t<MIT term>\t<CFD term>\n
// with the terms as "%.17g", so that the text gives the f64 values back: adding a guide's terms in line order and
// applying 10000 / (100 + sum) reproduces what isslScoreOfftargets prints for it at threshold 0.
// --profile: one line per guide, <guide 20-mer>\t<sites at 0..max distance>\t<occurrences at 0..max distance>\n.
// Same query-file rules as isslScoreOfftargets (issl_read_query_file); max distance 0..6.  stdout carries data only,
// diagnostics go to stderr, exit status 1 on any error.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslScoreOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "isslReportOfftargets"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_index_open) X(issl_index_header) X(issl_index_upload) X(issl_index_close) \
    X(issl_read_query_file) X(issl_free) X(issl_decode_guide) X(issl_offtarget_profile) X(issl_offtargets)
#include "cli_api.hpp"

int main(int argc, char **argv)
{
    bool profile = false;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--profile")) profile = true;
        else pos.push_back(argv[i]);
    }
    if (pos.size() != 3) {
        std::fprintf(stderr, "Usage: %s [issltable] [query file] [max distance] [--profile]\n", argv[0]);
        return 1;
    }
    char *end = nullptr;
    const long max_dist = std::strtol(pos[2], &end, 10);
    if (end == pos[2] || *end || max_dist < 0 || max_dist >= ISSL_PROFILE_BINS) {
        std::fprintf(stderr, "max distance must be a number from 0 to %d\n", ISSL_PROFILE_BINS - 1);
        return 1;
    }
    if (!load_api()) return 1;
    // same order of checks as isslScoreOfftargets: index file, query file, then the device
    issl_index *idx = nullptr;
    if (api.issl_index_open(pos[0], &idx)) return fail("cannot open index");
    issl_header hdr{};
    if (api.issl_index_header(idx, &hdr)) return fail("cannot read index header");
    uint64_t *guides = nullptr;
    size_t n = 0;
    if (api.issl_read_query_file(pos[1], hdr.seq_len, &guides, &n)) return fail("cannot read query file");
    const char *dev = std::getenv("ISSL_DEVICE");
    if (api.issl_index_upload(idx, dev ? std::atoi(dev) : 0)) return fail("cannot upload index");
    std::vector<char> seq(n * (hdr.seq_len + 1));
    for (size_t i = 0; i < n; ++i)
        if (api.issl_decode_guide(guides[i], hdr.seq_len, seq.data() + i * (hdr.seq_len + 1))) return fail("cannot decode guide");
    StdoutText so;
    std::string &out = so.text;
    char buf[128];
    bool ok = true;
    if (profile) {
        std::vector<issl_profile> prof(n);
        if (api.issl_offtarget_profile(idx, guides, n, static_cast<int>(max_dist), prof.data())) return fail("profile failed");
        for (size_t i = 0; ok && i < n; ++i) {
            out += seq.data() + i * (hdr.seq_len + 1);
            for (long d = 0; d <= max_dist; ++d) { std::snprintf(buf, sizeof buf, "\t%u", prof[i].sites[d]); out += buf; }
            for (long d = 0; d <= max_dist; ++d) { std::snprintf(buf, sizeof buf, "\t%llu", static_cast<unsigned long long>(prof[i].occurrences[d])); out += buf; }
            out += '\n';
            ok = so.wrote();
        }
    } else {
        // the query in runs of guides, so that the records of one run are in memory at a time
        const size_t run = size_t(1) << 14;
        std::vector<uint64_t> offsets;
        std::vector<issl_offtarget> recs;
        char site[64];
        for (size_t at = 0; ok && at < n; at += run) {
            const size_t cnt = n - at < run ? n - at : run;
            offsets.resize(cnt + 1);
            size_t total = 0;
            if (api.issl_offtargets(idx, guides + at, cnt, static_cast<int>(max_dist), offsets.data(), recs.data(), recs.size(), &total))
                return fail("report failed");
            if (total > recs.size()) {
                recs.resize(total + total / 4);
                if (api.issl_offtargets(idx, guides + at, cnt, static_cast<int>(max_dist), offsets.data(), recs.data(), recs.size(), &total))
                    return fail("report failed");
            }
            for (size_t k = 0; ok && k < total; ++k) {
                const issl_offtarget &r = recs[k];
                if (api.issl_decode_guide(r.site, hdr.seq_len, site)) return fail("cannot decode site");
                out += seq.data() + (at + r.guide) * (hdr.seq_len + 1);
                std::snprintf(buf, sizeof buf, "\t%s\t%u\t%u\t%.17g\t%.17g\n", site, unsigned(r.dist), r.occ, r.mit, r.cfd);
                out += buf;
                ok = so.wrote();
            }
        }
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    api.issl_free(guides);
    api.issl_index_close(idx);
    return 0;
}
