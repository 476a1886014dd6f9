// bin/cracklingBowtie -- the Bowtie step of Crackling (Crackling.py:600-725) for a list of guides:
//
//   cracklingBowtie [--page-length N] <guides file> <FASTA ...|directory>
//
// The guides file holds one guide per line, all 20 or all 23 characters long (the first line decides), under the scorer's
// query-file rules (issl_read_query_file: the characters and a line end per line); of a 23-mer the first 20 count.  The
// guides are the reference's candidates in its order, N its [bowtie2] page-length (default 0: one page).  One line per
// guide, in the order given:
//   <guide>\t<passedBowtie>\t<nb>\t<chr>\t<start>\t<end>\n
// passedBowtie, chr, start and end as the reference prints them (1, 0 or ?; the record's name up to the first blank, the
// 1-based start and start + 22 of the first perfect occurrence of <20-mer>AGG; *, 0, 22 when it does not occur; ? for an
// untested guide), nb the perfect alignments the reference counts for the guide's own eight reads (include/issl_hip.h,
// issl_genome_occurrences).  The FASTA arguments follow bin/extractOfftargets: one input or several, a lone directory
// stands for its non-hidden entries.  stdout carries data only, diagnostics go to stderr, exit status 1 on any error.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslLocateOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#define ISSL_CLI_NAME "cracklingBowtie"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_read_query_file) X(issl_free) X(issl_decode_guide)                        \
    X(issl_genome_open_files) X(issl_genome_record) X(issl_genome_occurrences) X(issl_genome_close)
#include "cli_api.hpp"

namespace {

// Length of the file's first line without its end, -1 when the file cannot be read.
long first_line_length(const char *path)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return -1;
    long k = 0;
    for (int c; (c = std::fgetc(fp)) != EOF && c != '\n';) ++k;
    std::fclose(fp);
    return k;
}

} // namespace

int main(int argc, char **argv)
{
    unsigned long long page_length = 0;
    std::vector<const char *> pos;
    bool usage = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--page-length")) {
            char *end = nullptr;
            if (i + 1 >= argc) { usage = true; break; }
            page_length = std::strtoull(argv[++i], &end, 10);
            if (!argv[i][0] || *end || argv[i][0] == '-') usage = true;
        } else {
            pos.push_back(argv[i]);
        }
    }
    if (usage || pos.size() < 2) {
        std::fprintf(stderr, "Usage: %s [--page-length N] <guides file> <FASTA ...|directory>\n", argv[0]);
        return 1;
    }
    if (!load_api()) return 1;
    // the guides file first, then the genome and the device
    const size_t width = first_line_length(pos[0]) == 23 ? 23 : 20;
    uint64_t *guides = nullptr;
    size_t n = 0;
    if (api.issl_read_query_file(pos[0], width, &guides, &n)) return fail("cannot read guides file");
    std::vector<uint64_t> sites(n);
    for (size_t k = 0; k < n; ++k) sites[k] = guides[k] & ((1ull << 40) - 1);
    const char *dev = std::getenv("ISSL_DEVICE");
    issl_genome *g = nullptr;
    if (api.issl_genome_open_files(pos.data() + 1, static_cast<int>(pos.size() - 1), dev ? std::atoi(dev) : 0, &g)) return fail("cannot open genome");
    std::vector<issl_occurrence> rows(n);
    if (api.issl_genome_occurrences(g, sites.data(), n, static_cast<size_t>(page_length), rows.data())) return fail("occurrences failed");
    StdoutText so;
    std::string &out = so.text;
    char guide[64], buf[96];
    bool ok = true;
    for (size_t k = 0; ok && k < n; ++k) {
        if (api.issl_decode_guide(guides[k], width, guide)) return fail("cannot decode guide");
        const issl_occurrence &r = rows[k];
        out += guide;
        if (r.code == 2) {
            std::snprintf(buf, sizeof buf, "\t?\t%u\t?\t?\t?\n", static_cast<unsigned>(r.nb));
            out += buf;
        } else if (r.record == 0xFFFFFFFFu) {
            std::snprintf(buf, sizeof buf, "\t%u\t%u\t*\t0\t22\n", static_cast<unsigned>(r.code), static_cast<unsigned>(r.nb));
            out += buf;
        } else {
            const char *name = nullptr;
            size_t name_len = 0, first = 0;
            uint64_t length = 0;
            if (api.issl_genome_record(g, r.record, &name, &name_len, &length)) return fail("record out of range");
            // as Bowtie2 names a record: its header up to the first blank
            while (first < name_len && std::strchr(" \t\n\v\f\r", name[first])) ++first;
            size_t last = first;
            while (last < name_len && !std::strchr(" \t\n\v\f\r", name[last])) ++last;
            std::snprintf(buf, sizeof buf, "\t%u\t%u\t", static_cast<unsigned>(r.code), static_cast<unsigned>(r.nb));
            out += buf;
            out.append(name + first, last - first);
            std::snprintf(buf, sizeof buf, "\t%llu\t%llu\n", static_cast<unsigned long long>(r.pos + 1),
                          static_cast<unsigned long long>(r.pos + 23));
            out += buf;
        }
        ok = so.wrote();
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    api.issl_free(guides);
    api.issl_genome_close(g);
    return 0;
}
