// The options of an index handle (include/issl_hip.h: issl_index_set_option / issl_index_get_option): one table of the
// settable ones, read from the environment when a handle is made, and the read-only keys that describe its image.
// Plain C++: no HIP runtime behind it.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "issl_device.hpp"

namespace issl {

namespace {

enum Kind { kInt, kFlag, kTri, kPath }; // integer range, 0|1, -1|0|1, file name

// The Tuning member an option sets, whatever its integer type (bool included: the values are 0 and 1 there).
template <class T, T Tuning::*M> void put(Tuning &t, long long v) { t.*M = static_cast<T>(v); }
template <class T, T Tuning::*M> long long get(const Tuning &t) { return static_cast<long long>(t.*M); }
#define MEMBER(m) put<decltype(Tuning::m), &Tuning::m>, get<decltype(Tuning::m), &Tuning::m>

struct Option {
    const char *key, *env;
    Kind kind;
    long long lo, hi, def; // range (kFlag: 0..1, kTri: -1..1) and default; kPath: Tuning::stamps_path, default empty
    void (*put)(Tuning &, long long);
    long long (*get)(const Tuning &);
    long long multiple = 1; // a value must be a multiple of this ...
    long long round = 1;    // ... and is kept rounded down to a multiple of this
};

constexpr long long kNoMax = LLONG_MAX;

const Option kOptions[] = {
    {"scan_blocks", "ISSL_SCAN_BLOCKS", kInt, 1, kScanMaxBlocks, kScanGridBlocks, MEMBER(scan_blocks)},
    {"scan_threads", "ISSL_SCAN_THREADS", kInt, 64, 1024, 1024, MEMBER(scan_threads), 64},
    {"upload_chunk_kib", "ISSL_UPLOAD_CHUNK_KIB", kInt, 4, 1 << 20, 16384, MEMBER(upload_chunk_kib)},
    {"upload_ring_min_kib", "ISSL_UPLOAD_RING_MIN_KIB", kInt, 0, kNoMax, 65536, MEMBER(upload_ring_min_kib)},
    {"upload_threads", "ISSL_UPLOAD_THREADS", kInt, 1, 32, 8, MEMBER(upload_threads)},
    {"item_guides", "ISSL_ITEM_GUIDES", kInt, 8, kItemGuides, kItemGuides, MEMBER(item_guides), 1, 8},
    {"scan_generic", "ISSL_SCAN_GENERIC", kFlag, 0, 1, 0, MEMBER(scan_generic)},
    {"stage_timing", "ISSL_STAGE_TIMING", kFlag, 0, 1, 0, MEMBER(stage_timing)},
    {"scan_events", "ISSL_SCAN_EVENTS", kInt, 0, 2, 2, MEMBER(scan_events)},
    {"raw_chunks", "ISSL_RAW_CHUNKS", kInt, 0, kNoMax, 0, MEMBER(raw_chunks)},
    {"inline_sigs", "ISSL_INLINE_SIGS", kTri, -1, 1, -1, MEMBER(inline_sigs)},
    {"host_cold", "ISSL_FORCE_HOST_COLD", kTri, -1, 1, -1, MEMBER(host_cold)},
    {"scan_stamps", "ISSL_SCAN_STAMPS", kPath, 0, 0, 0, nullptr, nullptr},
    {"sorted_layout", "ISSL_SORTED_LAYOUT", kTri, -1, 1, -1, MEMBER(sorted_layout)},
    {"prune", "ISSL_PRUNE", kTri, -1, 1, -1, MEMBER(prune)},
    {"lanes", "ISSL_LANES", kInt, 1, 3, 1, MEMBER(lanes)},
    {"compact", "ISSL_COMPACT", kTri, -1, 1, -1, MEMBER(compact)},
    {"tail_shapes", "ISSL_TAIL_SHAPES", kFlag, 0, 1, 1, MEMBER(tail_shapes)},
    {"hit_slots", "ISSL_HIT_SLOTS", kInt, 0, 2, 1, MEMBER(hit_slots)},
    {"lean_tail", "ISSL_LEAN_TAIL", kFlag, 0, 1, 1, MEMBER(lean_tail)},
    {"small_bin", "ISSL_SMALL_BIN", kFlag, 0, 1, 1, MEMBER(small_bin)},
    {"expect_guides", "ISSL_EXPECT_GUIDES", kInt, 0, kNoMax, 0, MEMBER(expect_guides)},
    {"fine_items", "ISSL_FINE_ITEMS", kInt, 0, kNoMax, 0, MEMBER(fine_items)},
    {"keep_lists", "ISSL_KEEP_LISTS", kTri, -1, 1, -1, MEMBER(keep_lists)},
};
#undef MEMBER

const Option *find(const char *key)
{
    for (const Option &o : kOptions)
        if (std::strcmp(o.key, key) == 0) return &o;
    return nullptr;
}

// Read-only keys: the layout of the uploaded image (-1 before an upload).
struct ImageKey {
    const char *key;
    long long (*get)(const ImageHeader &h);
};

const ImageKey kImageKeys[] = {
    {"is_sorted", [](const ImageHeader &h) -> long long { return (h.off_srec || h.off_sid) ? 1 : 0; }},
    {"is_compact", [](const ImageHeader &h) -> long long { return h.off_sid ? 1 : 0; }},
    {"cold_on_host", [](const ImageHeader &h) -> long long { return h.cold_on_host ? 1 : 0; }},
    {"cold_sections", [](const ImageHeader &h) -> long long { return h.cold_on_host; }}, // 0, 1 (lists), 3 (lists + sites)
    {"lists_absent", [](const ImageHeader &h) -> long long { return h.lists_absent; }},
    {"dense_mit", [](const ImageHeader &h) -> long long { return h.off_mit_dense ? 1 : 0; }},
    {"has_inline_sigs", [](const ImageHeader &h) -> long long { return h.off_esig ? 1 : 0; }},
};

} // namespace

Tuning Tuning::from_env()
{
    Tuning t;
    for (const Option &o : kOptions)
        if (o.put) o.put(t, o.def);
    const char *timing = std::getenv("ISSL_UPLOAD_TIMING"); // (environment only)
    t.upload_timing = timing && timing[0] == '1';
    const char *scan_verify = std::getenv("ISSL_SCAN_VERIFY"); // (environment only; 0 = the scan's waves verify nothing, 1 = also every wave's last chunk)
    t.scan_verify = !scan_verify ? -1 : std::strcmp(scan_verify, "0") == 0 ? 0 : std::strcmp(scan_verify, "1") == 0 ? 1 : -1; // (anything else: as unset)
    for (const Option &o : kOptions)
        if (const char *e = std::getenv(o.env)) (void)t.set(o.key, e); // values out of range leave the default
    return t;
}

bool Tuning::set(const char *key, const char *value)
{
    const Option *o = key && value ? find(key) : nullptr;
    if (!o) return false;
    if (o->kind == kPath) {
        stamps_path = value;
        return true;
    }
    char *end = nullptr;
    const long long n = std::strtoll(value, &end, 10);
    if (end == value || *end != 0 || n < o->lo || n > o->hi || n % o->multiple) return false;
    o->put(*this, n / o->round * o->round);
    return true;
}

bool Tuning::get(const char *key, long long *value) const
{
    const Option *o = find(key);
    if (!o || o->kind == kPath) return false; // (scan_stamps can be set, not read)
    *value = o->get(*this);
    return true;
}

int Tuning::set_list(const char *options)
{
    for (std::string rest = options ? options : ""; !rest.empty();) { // "key=value,key=value"
        const size_t comma = rest.find(',');
        const std::string item = rest.substr(0, comma);
        rest = comma == std::string::npos ? std::string() : rest.substr(comma + 1);
        const size_t eq = item.find('=');
        if (eq == std::string::npos || !set(item.substr(0, eq).c_str(), item.substr(eq + 1).c_str())) {
            set_error("unknown option or value out of range: " + item);
            return ISSL_E_ARG;
        }
    }
    return ISSL_OK;
}

bool image_option(const ImageHeader *h, const char *key, long long *value)
{
    for (const ImageKey &k : kImageKeys)
        if (std::strcmp(k.key, key) == 0) {
            *value = h ? k.get(*h) : -1;
            return true;
        }
    return false;
}

} // namespace issl
