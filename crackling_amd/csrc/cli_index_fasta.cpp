// bin/isslIndexFromFasta -- genome FASTA to .issl in one process, the site list never written out:
//
//   isslIndexFromFasta <output.issl> <slice width (bits)> <input FASTA ...| input directory>
//
// Writes the bytes of `extractOfftargets sites.txt <inputs>` followed by `isslCreateIndex sites.txt 20 <width> <output>`
// (issl_index_build_from_fasta_files).  Inputs as extractOfftargets takes them; widths 8, 4 or 2.  ISSL_DEVICE selects
// the GPU.  Exit status 2 for a usage error, 1 (with the library's message) for any other; no output file is left
// behind on failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/issl_hip.h"
#include "cli_inputs.hpp"

int main(int argc, char **argv)
{
    char *end = nullptr;
    const unsigned long width = argc >= 4 ? std::strtoul(argv[2], &end, 10) : 0;
    if (argc < 4 || end == argv[2] || *end != 0) {
        std::fprintf(stderr, "usage: %s <output.issl> <slice width (bits)> <input FASTA ...| input directory>\n", argv[0]);
        return 2;
    }
    const std::vector<std::string> inputs = expand_fasta_inputs(std::vector<std::string>(argv + 3, argv + argc));
    std::vector<const char *> ptrs;
    for (auto &s : inputs) ptrs.push_back(s.c_str());
    const char *dev = std::getenv("ISSL_DEVICE");
    const char *out = argv[1];
    issl_index *ix = nullptr;
    if (ptrs.empty()) {
        std::fprintf(stderr, "no input files\n");
        return 1;
    }
    if (issl_index_build_from_fasta_files(ptrs.data(), static_cast<int>(ptrs.size()), width, dev ? std::atoi(dev) : 0,
                                          nullptr, &ix)) {
        std::fprintf(stderr, "%s\n", issl_last_error());
        return 1;
    }
    issl_header h{};
    int rc = issl_index_header(ix, &h);
    if (rc == 0) rc = issl_index_write(ix, out);
    if (rc) {
        std::fprintf(stderr, "%s\n", issl_last_error());
        issl_index_close(ix);
        ::unlink(out);
        return 1;
    }
    issl_index_close(ix);
    std::fprintf(stderr, "%llu sites, %llu distinct, %llu slices of %llu bits -> %s\n", (unsigned long long)h.n_lines,
                 (unsigned long long)h.n_sites, (unsigned long long)h.n_slices, (unsigned long long)h.slice_width, out);
    return 0;
}
