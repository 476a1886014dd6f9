// The host-side plumbing around a kernel launch, one copy for every unit of the library: the HIP error check, device
// selection, the owners of device memory, streams and events, the stage timer and the small helpers next to them.  Host
// code only (no __global__, no __device__), all of it inline: a unit that needs a DevBuf includes this and nothing else.
#pragma once
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "issl_host.hpp"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            issl::set_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr);    \
            return ISSL_E_DEVICE;                                                                  \
        }                                                                                          \
    } while (0)

namespace issl {

// The visible devices -> *count; ISSL_E_DEVICE when there is none: `what` ("the ISSL scorer", "the extraction", ...) has
// no CPU fallback.
inline int count_devices(const char *what, int *count)
{
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess || *count <= 0) {
        set_error(std::string("no HIP device available: ") + what + " has no CPU fallback");
        return ISSL_E_DEVICE;
    }
    return ISSL_OK;
}

// Select `device`: ISSL_E_DEVICE when there is none, ISSL_E_ARG when it is out of range.
inline int select_device(int device, const char *what)
{
    int count = 0;
    if (int rc = count_devices(what, &count)) return rc;
    if (device < 0 || device >= count) {
        set_error("device " + std::to_string(device) + " out of range (" + std::to_string(count) + " visible)");
        return ISSL_E_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    return ISSL_OK;
}

// Device buffers are released on every path out of the functions that hold them.
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// Sections of one allocation, 256-byte aligned.
struct Arena {
    DevBuf buf;
    size_t size = 0;
    size_t reserve(size_t bytes) { const size_t at = size; size = (size + bytes + 255) & ~size_t(255); return at; }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(static_cast<char *>(buf.p) + off); }
};

// The stream of one call or one handle: its work neither waits for nor holds up what the caller's process has on the
// default stream.  A member ahead of the buffers it serves is destroyed after them.
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
};

// N events around the launches of one call, destroyed with the scope.
template <int N> struct Events {
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int create()
    {
        for (hipEvent_t &x : e) HIP_TRY(hipEventCreate(&x));
        return ISSL_OK;
    }
};

// Stage times of one call, for the stderr lines of ISSL_LOCATE_TIMING / ISSL_GUIDES_TIMING / ISSL_UPLOAD_TIMING.  When it
// is off, note() does nothing and the call waits nowhere for the clock.  On a stream: the stream is synchronised at
// every note() and " <stage> <ms> ms" is collected in `line` for the caller to print.  With a tag ("[issl genome]"): the
// device is synchronised and every stage is printed at once as "<tag> <stage> <ms> ms".
struct StageTimer {
    bool on;
    hipStream_t stream = nullptr;
    const char *tag = nullptr;
    double t0 = 0;
    std::string line;
    StageTimer(bool on_, hipStream_t s) : on(on_), stream(s) { if (on) { (void)hipStreamSynchronize(stream); t0 = now_ms(); } }
    StageTimer(bool on_, const char *tag_) : on(on_), tag(tag_) { if (on) t0 = now_ms(); }
    void note(const char *stage)
    {
        if (!on) return;
        if (tag) (void)hipDeviceSynchronize();
        else (void)hipStreamSynchronize(stream);
        const double t = now_ms();
        if (tag) {
            std::fprintf(stderr, "%s %s %.1f ms\n", tag, stage, t - t0);
        } else {
            char buf[64];
            std::snprintf(buf, sizeof buf, " %s %.3f ms", stage, t - t0);
            line += buf;
        }
        t0 = t;
    }
};

// Workgroups of `threads` that cover n items.
inline uint32_t blocks_for(uint64_t n, uint32_t threads) { return static_cast<uint32_t>((n + threads - 1) / threads); }

// `bytes` from `src` on `device` into host memory, blocking.
inline int copy_to_host(int device, void *out, const void *src, size_t bytes)
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

// The whole file at `path` -> out.  ISSL_E_IO with "cannot open <what>'<path>': <strerror>" (or "cannot read ...");
// `what` is the caller's noun ahead of the path ("annotation "), blank included.
inline int read_whole_file(const char *path, std::vector<char> &out, const char *what = "")
{
    auto refuse = [&](const char *verb) {
        set_error(std::string("cannot ") + verb + " " + what + "'" + path + "': " + std::strerror(errno));
        return ISSL_E_IO;
    };
    out.clear();
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return refuse("open");
    struct stat st;
    // a regular file is read with one allocation of its size and one fread; what a file holds beyond the size it
    // stated (it grew, or it is no regular file and stated none) comes through a small side buffer
    const size_t size = ::fstat(::fileno(fp), &st) == 0 && S_ISREG(st.st_mode) ? static_cast<size_t>(st.st_size) : 0;
    out.resize(size);
    out.resize(size ? std::fread(out.data(), 1, size, fp) : 0); // (shrinks at most: no reallocation)
    char tail[1 << 16];
    size_t got;
    if (out.size() == size)
        while ((got = std::fread(tail, 1, sizeof tail, fp)) > 0) out.insert(out.end(), tail, tail + got);
    const bool bad = std::ferror(fp) != 0;
    const int err = errno;
    std::fclose(fp);
    errno = err;
    if (bad) return refuse("read");
    return ISSL_OK;
}

} // namespace issl
