// Input list of the FASTA-reading executables (bin/extractOfftargets, bin/isslIndexFromFasta): the arguments as given,
// or, when the one argument is a directory, its non-hidden entries in sorted order (extractOfftargets.py:201-207).
// The number of inputs left decides the rules the library reads them by: one -> the reference's explode rules,
// several -> its per-file rules (issl_extract.hip, append_records).
#pragma once
#include <algorithm>
#include <dirent.h>
#include <string>
#include <sys/stat.h>
#include <vector>

inline std::vector<std::string> expand_fasta_inputs(std::vector<std::string> inputs)
{
    struct stat st;
    if (inputs.size() == 1 && ::stat(inputs[0].c_str(), &st) == 0 && S_ISDIR(st.st_mode)) {
        const std::string dir = inputs[0];
        inputs.clear();
        if (DIR *d = ::opendir(dir.c_str())) {
            while (dirent *e = ::readdir(d)) {
                if (e->d_name[0] == '.') continue;
                inputs.push_back(dir + "/" + e->d_name);
            }
            ::closedir(d);
        }
        std::sort(inputs.begin(), inputs.end());
    }
    return inputs;
}
