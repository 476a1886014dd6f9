// bin/isslSearchGenome -- where queries bind in a genome with up to max_dist mismatches, for any PAM pattern:
//
//   isslSearchGenome [--profile] [--guide START:LEN --dna-bulge D --rna-bulge R [--guide-variants N] [--guide-vcf FILE]] [--variants N] [--vcf FILE] [--indel-vcf FILE] <pattern> <query file> <max_dist> <FASTA ...|directory>
//
// pattern: 1 to 32 IUPAC codes (ACGTRYSWKMBDHVN), e.g. NNNNNNNNNNNNNNNNNNNNNGG or TTTVNNNNNNNNNNNNNNNNNNNN.  The query file has
// one query per line over ACGTN ("\n" or "\r\n" line ends, a trailing blank line is ignored), every line of the pattern's
// length; N is a position that is not compared.  The definitions are those of issl_genome_search (include/issl_hip.h).
// One line per hit, the queries in file order, a query's hits by record, position and strand:
//   <query text>\t<record name>\t<pos>\t<+|->\t<dist>\t<site>\n
// pos is the 0-based start of the window inside the record on the forward strand for both strands; the site is what the
// query is compared with ('-': the reverse complement of the window), its mismatching positions in lower case.
// With --profile one line per query: <query text>\t<hits at distance 0>\t...\t<hits at max_dist>\n
// With --guide START:LEN the search allows bulges beside the mismatches (issl_genome_search_bulges): START:LEN are the
// pattern positions where the protospacer lies, --dna-bulge D and --rna-bulge R (0..3, 1 when not given) the most bases of
// the site and of the query that pair with nothing.  One line per row, a query's rows by record, position, strand, bulge:
//   <query aligned>\t<record name>\t<pos>\t<+|->\t<dist>\t<bulge>\t<site aligned>\n
// bulge is 0, D1..D3 or R1..R3; the query carries '-' x d and the site '-' x r at the break point; the site's mismatching
// bases are in lower case, its unpaired bases in upper case.  Nothing is filtered: a locus that matches without a bulge is
// listed under the shifted windows of the other bulges too.  --profile then prints <query text> and the R + D + 1 groups
// (R3.., 0, ..D3) of max_dist + 1 counts, tab-separated.  --dna-bulge or --rna-bulge without --guide is a usage error.
// With --variants N the search reads IUPAC ambiguity codes in the genome as sets of bases (issl_genome_search_variants):
// a window of the codes ACGTRYSWKMBDHV with at most N ambiguous positions is compared, and dist is the least distance over
// the sequences it stands for.  --vcf FILE first writes the SNPs of a plain-text VCF into the resident genome as such codes
// (issl_genome_apply_vcf; CHROM is a record's name up to its first blank) and prints one line of counts to stderr; without
// --variants it implies --variants L, the pattern's length.  A row line is as without the option, the site in IUPAC
// letters: lower case where the position does not match, upper case elsewhere.  --profile lines are as without the option.
// --variants or --vcf together with --guide is a usage error.
// With --guide, --guide-variants N and --guide-vcf FILE are their counterparts for the search with bulges
// (issl_genome_search_bulges_variants): the window of L + bulge codes may hold at most N ambiguous positions, its unpaired
// bases included; --guide-vcf applies the VCF first and prints the counts line to stderr, and alone it implies N = L.  A row
// line is --guide's with the site in IUPAC letters: lower case where the position does not match, upper case elsewhere,
// '-' at an RNA bulge.  --profile prints --guide's groups.  Either option without --guide is a usage error.
// With --indel-vcf FILE the search runs on the ALT haplotypes of FILE's indels instead of the reference text
// (issl_haplotypes_search): every ALT allele over ACGT that is no SNP, one at a time, at the windows of the pattern's length
// that overlap its edit.  --vcf is applied first, so the bases around an edit carry its SNPs; without --variants it implies
// --variants L.  One line of counts goes to stderr.  A row line is --variants' followed by
//   \t<POS>:<REF>><ALT>\t<edit_at>
// POS 1-based and REF, ALT of the edit with its common suffix and then its common prefix removed ('-' for none), edit_at the
// window index of the first ALT base or of the first base behind a deletion (negative: the window starts inside ALT).
// --profile lines are as without the option.  Together with --guide it is a usage error: bulges on haplotypes are not built.
// The FASTA arguments follow bin/extractOfftargets: one input or several, a lone directory stands for its non-hidden
// entries.  stdout carries data only, diagnostics go to stderr, exit status 1 on any error.
//   ISSL_DEVICE=<n>       HIP device to use (default 0)
//   ISSL_LIBRARY=<path>   libissl_hip.so to load (default: ../crackling_amd/ next to the executable, then the loader's path)
// The executable does not link the library: it is loaded with dlopen, as isslLocateOfftargets does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define ISSL_CLI_NAME "isslSearchGenome"
#define ISSL_CLI_API(X)                                                                                                   \
    X(issl_last_error) X(issl_abi_version) X(issl_genome_open_files) X(issl_genome_record)                                  \
    X(issl_genome_search) X(issl_genome_search_profile) X(issl_genome_search_bulges) X(issl_genome_search_bulges_profile)             \
    X(issl_genome_search_variants) X(issl_genome_search_variants_profile) X(issl_genome_apply_vcf)                          \
    X(issl_genome_search_bulges_variants) X(issl_genome_search_bulges_variants_profile)                                     \
    X(issl_genome_info) X(issl_vcf_indels) X(issl_haplotypes_open) X(issl_haplotypes_search) X(issl_haplotypes_search_profile)  \
    X(issl_haplotypes_close)                                                                                              \
    X(issl_genome_close)
#include "cli_api.hpp"
#include "issl_bulge_variants_text.hpp"
#include "issl_haplotypes_text.hpp"
#include "issl_search_text.hpp"
#include "issl_variants_text.hpp"

// The rows of one search, one line each: search(hits, cap, &total) is the library call -- asked for the total first, then
// with room for it -- and line(record name, its length, row) appends a row's text.  ok: false after a short write on
// stdout.  -> false after a failure, which is reported.
template <class Row, class Search, class Line> bool print_rows(issl_genome *g, StdoutText &so, bool &ok, Search &&search, Line &&line)
{
    std::vector<Row> hits;
    size_t total = 0;
    if (search(nullptr, 0, &total)) return !fail("search failed");
    if (total) {
        hits.resize(total);
        if (search(hits.data(), hits.size(), &total)) return !fail("search failed");
    }
    for (const Row &hit : hits) {
        const char *name = nullptr;
        size_t name_len = 0;
        uint64_t length = 0;
        if (api.issl_genome_record(g, hit.record, &name, &name_len, &length)) return !fail("record out of range");
        line(name, name_len, hit);
        if (!(ok = so.wrote())) break;
    }
    return true;
}

int main(int argc, char **argv)
{
    namespace st = issl::search_text;
    bool profile = false, usage = false;
    const char *guide = nullptr, *dna = nullptr, *rna = nullptr, *variants = nullptr, *vcf = nullptr, *guide_variants = nullptr,
               *guide_vcf = nullptr, *indel_vcf = nullptr;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        const char **value = !std::strcmp(argv[i], "--guide") ? &guide : !std::strcmp(argv[i], "--dna-bulge") ? &dna
                             : !std::strcmp(argv[i], "--rna-bulge") ? &rna : !std::strcmp(argv[i], "--variants") ? &variants
                             : !std::strcmp(argv[i], "--vcf") ? &vcf : !std::strcmp(argv[i], "--guide-variants") ? &guide_variants
                             : !std::strcmp(argv[i], "--guide-vcf") ? &guide_vcf : !std::strcmp(argv[i], "--indel-vcf") ? &indel_vcf
                             : nullptr;
        if (value) {
            if (i + 1 < argc) *value = argv[++i];
            else usage = true;
        } else if (!std::strcmp(argv[i], "--profile")) profile = true;
        else pos.push_back(argv[i]);
    }
    if (usage || pos.size() < 4 || ((dna || rna || guide_variants || guide_vcf) && !guide) || ((variants || vcf || indel_vcf) && guide)) {
        std::fprintf(stderr, "Usage: %s [--profile] [--guide START:LEN --dna-bulge D --rna-bulge R [--guide-variants N] [--guide-vcf FILE]] [--variants N] [--vcf FILE] [--indel-vcf FILE] <pattern> <query file> <max_dist> <FASTA ...|directory>\n",
                     argv[0]);
        return 1;
    }
    // the span and the limits as numbers; what they may be is the library's check (check_bulges), made below
    issl_search_bulges bg{0, 0, 1, 1};
    if (guide) {
        auto number = [](const char *text, char stop, uint32_t *out, const char **rest) {
            char *e = nullptr;
            const unsigned long v = std::strtoul(text, &e, 10);
            if (e == text || *text == '-' || *text == '+' || *e != stop || v > 0xFFFFFFFFul) return false;
            *out = static_cast<uint32_t>(v);
            if (rest) *rest = e + 1;
            return true;
        };
        const char *rest = nullptr;
        if (!number(guide, ':', &bg.guide_start, &rest) || !number(rest, 0, &bg.guide_length, nullptr)) {
            std::fprintf(stderr, "--guide '%s': START:LEN, two numbers\n", guide);
            return 1;
        }
        if ((dna && !number(dna, 0, &bg.max_dna, nullptr)) || (rna && !number(rna, 0, &bg.max_rna, nullptr))) {
            std::fprintf(stderr, "--dna-bulge and --rna-bulge take a number from 0 to 3\n");
            return 1;
        }
    }
    // the pattern, max_dist and the query file first, then the library, the genome and the device
    issl_search_pattern pat;
    std::string err;
    if (!st::parse_pattern(pos[0], &pat, err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    char *end = nullptr;
    const long max_dist = std::strtol(pos[2], &end, 10);
    if (end == pos[2] || *end || max_dist < 0 || max_dist > static_cast<long>(pat.length)) {
        std::fprintf(stderr, "max_dist '%s': a number from 0 to the pattern's length %u\n", pos[2], pat.length);
        return 1;
    }
    long max_variants = static_cast<long>(pat.length); // (--vcf or --guide-vcf alone)
    if (variants || guide_variants) {
        const char *given = variants ? variants : guide_variants;
        max_variants = std::strtol(given, &end, 10);
        if (end == given || *end || max_variants < 0 || max_variants > static_cast<long>(pat.length)) {
            std::fprintf(stderr, "%s '%s': a number from 0 to the pattern's length %u\n", variants ? "--variants" : "--guide-variants", given,
                         pat.length);
            return 1;
        }
    }
    if (guide_vcf) vcf = guide_vcf; // (read and applied the same way)
    std::string text, packed, vcf_text, indel_text;
    if (indel_vcf && !read_text_file(indel_vcf, indel_text)) {
        std::fprintf(stderr, "cannot open '%s'\n", indel_vcf);
        return 1;
    }
    if (vcf && !read_text_file(vcf, vcf_text)) {
        std::fprintf(stderr, "cannot open '%s'\n", vcf);
        return 1;
    }
    if (!read_text_file(pos[1], text)) {
        std::fprintf(stderr, "cannot open '%s'\n", pos[1]);
        return 1;
    }
    if (guide && !st::check_bulges(&pat, &bg, err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    size_t n = 0;
    if (!st::split_query_lines(text, pat.length, packed, n, err)) {
        std::fprintf(stderr, "'%s' %s\n", pos[1], err.c_str());
        return 1;
    }
    std::vector<issl_search_query> queries(n);
    if (!st::prepare(pos[0], packed.data(), n, pat.length, &pat, queries.data(), err)) {
        std::fprintf(stderr, "'%s' %s\n", pos[1], err.c_str());
        return 1;
    }
    if (!load_api()) return 1;
    const char *dev = std::getenv("ISSL_DEVICE");
    issl_genome *g = nullptr;
    if (api.issl_genome_open_files(pos.data() + 3, static_cast<int>(pos.size() - 3), dev ? std::atoi(dev) : 0, &g)) return fail("cannot open genome");
    if (vcf) {
        issl_vcf_counts vc{};
        uint64_t changed = 0;
        if (api.issl_genome_apply_vcf(g, vcf_text.data(), vcf_text.size(), &vc, &changed)) return fail("cannot apply the VCF");
        std::fprintf(stderr, "vcf: lines %llu snps %llu alleles_skipped %llu no_allele %llu unknown_chrom %llu beyond_record %llu changed %llu\n",
                     static_cast<unsigned long long>(vc.lines), static_cast<unsigned long long>(vc.snps),
                     static_cast<unsigned long long>(vc.alleles_skipped), static_cast<unsigned long long>(vc.no_allele),
                     static_cast<unsigned long long>(vc.unknown_chrom), static_cast<unsigned long long>(vc.beyond_record),
                     static_cast<unsigned long long>(changed));
    }
    StdoutText so;
    bool ok = true;
    std::vector<uint64_t> offsets(n + 1);
    const uint32_t L = pat.length, D = static_cast<uint32_t>(max_dist);
    if (indel_vcf) {
        // the indels against the handle's records, then their strips for windows of the pattern's length
        uint64_t n_records = 0, n_bases = 0;
        if (api.issl_genome_info(g, &n_records, &n_bases)) return fail("cannot read the genome's records");
        std::vector<const char *> names(n_records);
        std::vector<size_t> name_lens(n_records);
        std::vector<uint64_t> lengths(n_records);
        for (uint64_t r = 0; r < n_records; ++r)
            if (api.issl_genome_record(g, r, &names[r], &name_lens[r], &lengths[r])) return fail("record out of range");
        size_t n_indels = 0, n_alleles = 0;
        issl_vcf_indel_counts ic{};
        if (api.issl_vcf_indels(indel_text.data(), indel_text.size(), names.data(), name_lens.data(), lengths.data(), n_records, nullptr, 0,
                                &n_indels, nullptr, 0, &n_alleles, &ic))
            return fail("cannot read the indel VCF");
        std::vector<issl_indel> indels(n_indels);
        std::string alleles(n_alleles, '\0');
        if (n_indels && api.issl_vcf_indels(indel_text.data(), indel_text.size(), names.data(), name_lens.data(), lengths.data(), n_records,
                                            indels.data(), indels.size(), &n_indels, &alleles[0], alleles.size(), &n_alleles, &ic))
            return fail("cannot read the indel VCF");
        std::fprintf(stderr, "indel-vcf: lines %llu indels %llu alleles_skipped %llu no_allele %llu unknown_chrom %llu beyond_record %llu too_long %llu\n",
                     static_cast<unsigned long long>(ic.lines), static_cast<unsigned long long>(ic.indels),
                     static_cast<unsigned long long>(ic.alleles_skipped), static_cast<unsigned long long>(ic.no_allele),
                     static_cast<unsigned long long>(ic.unknown_chrom), static_cast<unsigned long long>(ic.beyond_record),
                     static_cast<unsigned long long>(ic.too_long));
        issl_haplotypes *h = nullptr;
        if (api.issl_haplotypes_open(g, indels.data(), indels.size(), alleles.data(), alleles.size(), static_cast<int>(L), &h))
            return fail("cannot build the haplotypes");
        if (profile) {
            std::vector<uint64_t> counts(n * (D + 1));
            if (api.issl_haplotypes_search_profile(h, &pat, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants), counts.data()))
                return fail("search failed");
            for (size_t k = 0; ok && k < n; ++k) {
                st::append_profile_line(so.text, packed.data() + k * L, L, counts.data() + k * (D + 1), D);
                ok = so.wrote();
            }
        } else {
            auto search = [&](issl_haplotype_hit *hits, size_t cap, size_t *total) {
                return api.issl_haplotypes_search(h, &pat, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants), offsets.data(),
                                                  hits, cap, total);
            };
            if (!print_rows<issl_haplotype_hit>(g, so, ok, search, [&](const char *name, size_t name_len, const issl_haplotype_hit &hit) {
                issl::haplotypes_text::append_haplotype_line(so.text, packed.data() + static_cast<size_t>(hit.query) * L, L, name, name_len, hit,
                                                             indels[hit.indel], alleles.data());
                }))
                return 1;
        }
        api.issl_haplotypes_close(h);
    } else if (guide && (guide_variants || guide_vcf) && profile) {
        const uint32_t bins = (bg.max_rna + bg.max_dna + 1) * (D + 1);
        std::vector<uint64_t> counts(n * bins);
        if (api.issl_genome_search_bulges_variants_profile(g, &pat, &bg, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants),
                                                           counts.data()))
            return fail("search failed");
        for (size_t k = 0; ok && k < n; ++k) {
            st::append_profile_line(so.text, packed.data() + k * L, L, counts.data() + k * bins, bins - 1);
            ok = so.wrote();
        }
    } else if (guide && (guide_variants || guide_vcf)) {
        auto search = [&](issl_bulge_variant_hit *hits, size_t cap, size_t *total) {
            return api.issl_genome_search_bulges_variants(g, &pat, &bg, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants),
                                                          offsets.data(), hits, cap, total);
        };
        if (!print_rows<issl_bulge_variant_hit>(g, so, ok, search, [&](const char *name, size_t name_len, const issl_bulge_variant_hit &hit) {
            issl::bulge_variants_text::append_bulge_variant_line(so.text, packed.data() + static_cast<size_t>(hit.query) * L, L, bg.guide_start,
                                                                 name, name_len, hit);
            }))
            return 1;
    } else if (guide && profile) {
        const uint32_t bins = (bg.max_rna + bg.max_dna + 1) * (D + 1);
        std::vector<uint64_t> counts(n * bins);
        if (api.issl_genome_search_bulges_profile(g, &pat, &bg, queries.data(), n, static_cast<int>(D), counts.data())) return fail("search failed");
        for (size_t k = 0; ok && k < n; ++k) {
            st::append_profile_line(so.text, packed.data() + k * L, L, counts.data() + k * bins, bins - 1);
            ok = so.wrote();
        }
    } else if (guide) {
        auto search = [&](issl_bulge_hit *hits, size_t cap, size_t *total) {
            return api.issl_genome_search_bulges(g, &pat, &bg, queries.data(), n, static_cast<int>(D), offsets.data(), hits, cap, total);
        };
        if (!print_rows<issl_bulge_hit>(g, so, ok, search, [&](const char *name, size_t name_len, const issl_bulge_hit &hit) {
            st::append_bulge_line(so.text, packed.data() + static_cast<size_t>(hit.query) * L, L, bg.guide_start, name, name_len, hit);
            }))
            return 1;
    } else if ((variants || vcf) && profile) {
        std::vector<uint64_t> counts(n * (D + 1));
        if (api.issl_genome_search_variants_profile(g, &pat, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants), counts.data()))
            return fail("search failed");
        for (size_t k = 0; ok && k < n; ++k) {
            st::append_profile_line(so.text, packed.data() + k * L, L, counts.data() + k * (D + 1), D);
            ok = so.wrote();
        }
    } else if (variants || vcf) {
        auto search = [&](issl_variant_hit *hits, size_t cap, size_t *total) {
            return api.issl_genome_search_variants(g, &pat, queries.data(), n, static_cast<int>(D), static_cast<int>(max_variants),
                                                   offsets.data(), hits, cap, total);
        };
        if (!print_rows<issl_variant_hit>(g, so, ok, search, [&](const char *name, size_t name_len, const issl_variant_hit &hit) {
            issl::variants_text::append_variant_line(so.text, packed.data() + static_cast<size_t>(hit.query) * L, L, name, name_len, hit);
            }))
            return 1;
    } else if (profile) {
        std::vector<uint64_t> counts(n * (D + 1));
        if (api.issl_genome_search_profile(g, &pat, queries.data(), n, static_cast<int>(D), counts.data())) return fail("search failed");
        for (size_t k = 0; ok && k < n; ++k) {
            st::append_profile_line(so.text, packed.data() + k * L, L, counts.data() + k * (D + 1), D);
            ok = so.wrote();
        }
    } else {
        auto search = [&](issl_search_hit *hits, size_t cap, size_t *total) {
            return api.issl_genome_search(g, &pat, queries.data(), n, static_cast<int>(D), offsets.data(), hits, cap, total);
        };
        if (!print_rows<issl_search_hit>(g, so, ok, search, [&](const char *name, size_t name_len, const issl_search_hit &hit) {
            st::append_hit_line(so.text, packed.data() + static_cast<size_t>(hit.query) * L, L, name, name_len, hit);
            }))
            return 1;
    }
    ok = ok && so.finish();
    if (!ok) { std::fprintf(stderr, "short write on stdout\n"); return 1; }
    api.issl_genome_close(g);
    return 0;
}
