// The GFF3 parser of the transcript hit counts (crackling_amd/csrc/issl_annotation.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone CPU program, no device code and no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/annotation_sanitize.cpp \
//       crackling_amd/csrc/issl_annotation.cpp crackling_amd/csrc/issl_host.cpp -lpthread -o <tmp>/annotation_sanitize
//   <tmp>/annotation_sanitize tests/golden/transcripts/*/annotation.gff
// Every file is parsed as it stands, at every truncation, and in a few thousand byte-mutated copies (a byte replaced by
// one of the characters the parser gives a meaning, by a random byte, removed or doubled); what parses is turned into
// intervals and checked for consistency.  Each result must be ISSL_OK, ISSL_E_FORMAT or ISSL_E_UNSUPPORTED with a
// message -- never a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../crackling_amd/csrc/issl_annotation.hpp"
#include "../crackling_amd/csrc/issl_host.hpp"

extern "C" void issl_free(void *p) { std::free(p); } // (lives in issl_capi.cpp, built with the HIP runtime)

static unsigned long g_ok = 0, g_format = 0, g_unsupported = 0;

static void check(const std::string &text)
{
    issl::AnnotationTables t;
    const int rc = issl::parse_annotation(text.data(), text.size(), t);
    if (rc == ISSL_E_FORMAT) {
        if (!issl::get_error()[0]) { std::fprintf(stderr, "format error without a message\n"); std::exit(1); }
        ++g_format;
        return;
    }
    if (rc != ISSL_OK) { std::fprintf(stderr, "unexpected code %d\n", rc); std::exit(1); }
    if (t.tr_seq.size() != t.tr_gene.size()) { std::fprintf(stderr, "transcript tables differ in length\n"); std::exit(1); }
    for (const uint32_t s : t.tr_seq)
        if (s >= t.seqs.size()) { std::fprintf(stderr, "transcript on a sequence that is not listed\n"); std::exit(1); }
    for (const uint32_t g : t.tr_gene)
        if (g != issl::kNoGene && g >= t.gene_count.size()) { std::fprintf(stderr, "gene out of range\n"); std::exit(1); }
    for (const issl::AnnotationExon &x : t.exons)
        if (x.seq >= t.seqs.size() || x.transcript >= t.tr_seq.size() || t.tr_seq[x.transcript] != x.seq) {
            std::fprintf(stderr, "exon out of range\n");
            std::exit(1);
        }
    issl::AnnotationIntervals iv;
    const int rc2 = issl::annotation_intervals(t, iv);
    if (rc2 == ISSL_E_UNSUPPORTED) { ++g_unsupported; return; }
    if (rc2 != ISSL_OK || iv.lo.size() != iv.hi.size() || iv.lo.size() != iv.tr.size() || iv.lo.size() > t.exons.size()) {
        std::fprintf(stderr, "intervals inconsistent\n");
        std::exit(1);
    }
    for (size_t i = 0; i < iv.lo.size(); ++i) {
        const bool follows = i && iv.tr[i - 1] == iv.tr[i];
        if (iv.lo[i] >= iv.hi[i] || (iv.lo[i] >> issl::kCoordBits) != (iv.hi[i] >> issl::kCoordBits) || (follows && iv.hi[i - 1] > iv.lo[i])) {
            std::fprintf(stderr, "intervals of a transcript overlap or are empty\n");
            std::exit(1);
        }
    }
    ++g_ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <annotation.gff ...>\n", argv[0]); return 2; }
    std::mt19937_64 rng(20261018);
    static const char special[] = "\t\n\r;=.- +0919eIDParentmRNAgx\0\x1f\xff";
    for (int f = 1; f < argc; ++f) {
        std::string text;
        FILE *fp = std::fopen(argv[f], "rb");
        if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
        char buf[4096];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, k);
        std::fclose(fp);
        check(text);
        for (size_t cut = 0; cut < text.size(); ++cut) check(text.substr(0, cut));
        for (int round = 0; round < 3000 && !text.empty(); ++round) {
            std::string m = text;
            for (int edits = 1 + static_cast<int>(rng() % 3); edits > 0 && !m.empty(); --edits) {
                const size_t at = rng() % m.size();
                switch (rng() % 4) {
                case 0: m[at] = special[rng() % (sizeof special - 1)]; break;
                case 1: m[at] = static_cast<char>(rng()); break;
                case 2: m.erase(at, 1); break;
                default: m.insert(at, 1, m[at]); break;
                }
            }
            check(m);
        }
    }
    // coordinates at and beyond the bounds
    check("s\tx\texon\t-9223372036854775808\t9223372036854775807\t.\t+\t.\tID=e;Parent=t\n");
    check("s\tx\texon\t-5\t-1\t.\t+\t.\tID=e;Parent=t\ns\tx\texon\t-5\t1099511627774\t.\t+\t.\tID=f;Parent=t\n");
    check("s\tx\texon\t9223372036854775808\t1\t.\t+\t.\tID=e;Parent=t\n");
    std::printf("annotation_sanitize: %lu parsed, %lu format errors, %lu unsupported, no sanitizer report\n", g_ok, g_format, g_unsupported);
    return g_ok && g_format && g_unsupported ? 0 : 1;
}
