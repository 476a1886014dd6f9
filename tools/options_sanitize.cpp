// The option parser of an index handle (crackling_amd/csrc/issl_options.cpp) under AddressSanitizer + UBSan (CPU build
// only).  Built and run by tests/test_host_sanitizers.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/options_sanitize.cpp \
//       crackling_amd/csrc/issl_options.cpp crackling_amd/csrc/issl_host.cpp -lpthread -o <tmp>/options_sanitize
// Malformed values (empty, not a number, trailing junk, overflowing, negative) must be refused and change nothing.
#include <cstdio>
#include <cstring>

#include "../crackling_amd/csrc/issl_device.hpp"

int main()
{
    issl::Tuning t = issl::Tuning::from_env();
    const issl::Tuning before = t;
    for (const char *key : {"scan_blocks", "scan_threads", "item_guides", "upload_chunk_kib", "raw_chunks", "lanes", "prune",
                            "scan_generic", "no_such_key", ""})
        for (const char *bad : {"", "x", "12x", " ", "-", "99999999999999999999999", "-99999999999999999999999", "-2", "0x10"}) {
            const bool unbounded = std::strcmp(key, "raw_chunks") == 0 && bad[0] == '9'; // (no upper bound: strtoll's clamp is in range)
            if (t.set(key, bad) && !unbounded) {
                std::fprintf(stderr, "Tuning::set(%s, \"%s\") accepted\n", key, bad);
                return 1;
            }
        }
    long long v = 0;
    if (!t.get("scan_blocks", &v) || v != before.scan_blocks || !t.get("lanes", &v) || v != before.lanes ||
        t.set(nullptr, "1") || t.set("lanes", nullptr) || t.get("scan_stamps", &v) || t.set_list("lanes=2,prune") == ISSL_OK) {
        std::fprintf(stderr, "Tuning: malformed input changed an option or was accepted\n");
        return 1;
    }
    std::printf("ok: option parser\n");
    return 0;
}
