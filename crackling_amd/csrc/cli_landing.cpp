// bin/isslLandOfftargets -- where the off-targets of every guide of a query file lie in the genome, and what they cut:
//
//   isslLandOfftargets [--annotation genes.gff3] [--profile] <issl> <query file> <max_dist> <FASTA ...|directory>
//
// Default: one line per landing -- one occurrence in the genome of one off-target of one guide --, guides in input order,
// a guide's off-targets in the reference's scoring order (as bin/isslReportOfftargets lists them), an off-target's
// landings by record, position and strand (as bin/isslLocateOfftargets lists them):
//   <guide 20-mer>\t<site 20-mer>\t<mismatches>\t<occurrences>\t<record name>\t<pos>\t<+|->\n
// The record name is the header as isslLocateOfftargets prints it; pos is 0-based inside the record.  With --annotation
// there is an eighth column, hits, as countHitTranscripts prints it for (the name up to its first blank, pos + 1):
// <hit>/<total>, or ?/? where the reference could not tell.
// --profile: one line per guide,
//   <guide 20-mer>\t<located at 0..max_dist>\t<in exon at 0..max_dist>\t<absent at 0..max_dist>\n
// (include/issl_hip.h, issl_landing_profile; in exon is 0 without --annotation).
// Same query-file rules as isslScoreOfftargets (issl_read_query_file); max_dist 0..6; the FASTA arguments follow
// bin/isslLocateOfftargets.  stdout carries data only, diagnostics go to stderr, exit status 1 on any error.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslReportOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "isslLandOfftargets"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_index_open) X(issl_index_header) X(issl_index_upload) X(issl_index_close) \
    X(issl_read_query_file) X(issl_free) X(issl_decode_guide) X(issl_genome_open_files) X(issl_genome_record)               \
    X(issl_genome_close) X(issl_annotation_open_file) X(issl_annotation_close) X(issl_offtarget_landings)                   \
    X(issl_offtarget_landing_profile)
#include "cli_api.hpp"

int main(int argc, char **argv)
{
    bool profile = false, bad = false;
    const char *gff = nullptr;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--profile")) profile = true;
        else if (!std::strcmp(argv[i], "--annotation")) {
            if (i + 1 < argc) gff = argv[++i];
            else bad = true;
        } else pos.push_back(argv[i]);
    }
    if (bad || pos.size() < 4) {
        std::fprintf(stderr, "Usage: %s [--annotation genes.gff3] [--profile] <issl> <query file> <max_dist> <FASTA ...|directory>\n", argv[0]);
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
    const int device = dev ? std::atoi(dev) : 0;
    if (api.issl_index_upload(idx, device)) return fail("cannot upload index");
    issl_genome *g = nullptr;
    if (api.issl_genome_open_files(pos.data() + 3, static_cast<int>(pos.size() - 3), device, &g)) return fail("cannot open genome");
    issl_annotation *ann = nullptr;
    if (gff && api.issl_annotation_open_file(gff, device, &ann)) return fail("cannot open annotation");
    std::vector<char> seq(n * (hdr.seq_len + 1));
    for (size_t i = 0; i < n; ++i)
        if (api.issl_decode_guide(guides[i], hdr.seq_len, seq.data() + i * (hdr.seq_len + 1))) return fail("cannot decode guide");
    StdoutText so;
    std::string &out = so.text;
    char buf[128];
    bool ok = true;
    if (profile) {
        std::vector<issl_landing_profile> prof(n);
        if (api.issl_offtarget_landing_profile(idx, g, ann, guides, n, static_cast<int>(max_dist), prof.data())) return fail("profile failed");
        for (size_t i = 0; ok && i < n; ++i) {
            out += seq.data() + i * (hdr.seq_len + 1);
            for (long d = 0; d <= max_dist; ++d) { std::snprintf(buf, sizeof buf, "\t%llu", static_cast<unsigned long long>(prof[i].located[d])); out += buf; }
            for (long d = 0; d <= max_dist; ++d) { std::snprintf(buf, sizeof buf, "\t%llu", static_cast<unsigned long long>(prof[i].in_exon[d])); out += buf; }
            for (long d = 0; d <= max_dist; ++d) { std::snprintf(buf, sizeof buf, "\t%u", prof[i].absent[d]); out += buf; }
            out += '\n';
            ok = so.wrote();
        }
    } else {
        // the query in runs of guides, so that the landings of one run are in memory at a time
        const size_t run = size_t(1) << 10;
        std::vector<uint64_t> offsets;
        std::vector<issl_landing> rows;
        char site[64];
        for (size_t at = 0; ok && at < n; at += run) {
            const size_t cnt = n - at < run ? n - at : run;
            offsets.resize(cnt + 1);
            size_t total = 0;
            if (api.issl_offtarget_landings(idx, g, ann, guides + at, cnt, static_cast<int>(max_dist), offsets.data(), rows.data(), rows.size(), &total))
                return fail("landings failed");
            if (total > rows.size()) {
                rows.resize(total + total / 4);
                if (api.issl_offtarget_landings(idx, g, ann, guides + at, cnt, static_cast<int>(max_dist), offsets.data(), rows.data(), rows.size(), &total))
                    return fail("landings failed");
            }
            for (size_t k = 0; ok && k < total; ++k) {
                const issl_landing &r = rows[k];
                const char *name = nullptr;
                size_t name_len = 0;
                uint64_t length = 0;
                if (api.issl_decode_guide(r.site, hdr.seq_len, site)) return fail("cannot decode site");
                if (api.issl_genome_record(g, r.record, &name, &name_len, &length)) return fail("record out of range");
                out += seq.data() + (at + r.guide) * (hdr.seq_len + 1);
                std::snprintf(buf, sizeof buf, "\t%s\t%u\t%u\t", site, unsigned(r.dist), r.occ);
                out += buf;
                out.append(name, name_len);
                std::snprintf(buf, sizeof buf, "\t%llu\t%c", static_cast<unsigned long long>(r.pos), r.strand ? '-' : '+');
                out += buf;
                if (ann) {
                    if (r.hits.status == 0) std::snprintf(buf, sizeof buf, "\t%u/%u", r.hits.hit, r.hits.total);
                    else std::snprintf(buf, sizeof buf, "\t?/?");
                    out += buf;
                }
                out += '\n';
                ok = so.wrote();
            }
        }
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    api.issl_free(guides);
    if (ann) api.issl_annotation_close(ann);
    api.issl_genome_close(g);
    api.issl_index_close(idx);
    return 0;
}
