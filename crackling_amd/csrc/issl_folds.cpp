// RNAfold's exchange, host side (issl_folds_*, include/issl_hip.h): the handle, the argument checks, the arena the pages'
// text stays in, the launches of issl_folds.hip and the two files RNAfold reads and writes.  The host waits once per read,
// for the error word.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_folds.hpp"
#include "issl_folds_text.hpp"
#include "issl_host.hpp"

namespace issl {
namespace {

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

int in_list(const issl_folds *f, uint64_t first, uint64_t n)
{
    if (first > f->src.n_fold || n > f->src.n_fold - first) {
        set_error("rows " + std::to_string(first) + " and the " + std::to_string(n) + " behind it of a fold list of " +
                  std::to_string(f->src.n_fold));
        return ISSL_E_ARG;
    }
    return ISSL_OK;
}

int folds_open(const issl_consensus *c, issl_folds **out)
{
    std::unique_ptr<issl_folds> f(new issl_folds());
    f->consensus = c;
    f->src = consensus_fold_source(c);
    if (f->src.n_fold) {
        if (int rc = select_device(f->src.device, "the extraction")) return rc;
        HIP_TRY(hipStreamCreateWithFlags(&f->stream.s, hipStreamNonBlocking));
        HIP_TRY(hipMalloc(&f->folds.p, 16ull * f->src.n_fold));
        HIP_TRY(hipMalloc(&f->spans.p, 48ull * f->src.n_fold));
        HIP_TRY(hipMalloc(&f->error.p, 8));
        launch_folds_clear(static_cast<issl_fold *>(f->folds.p), static_cast<issl_text_span *>(f->spans.p), 0, f->src.n_fold,
                           f->stream.s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(f->stream.s));
    }
    *out = f.release();
    return ISSL_OK;
}

// The lines of rows [first, first + n) into f->input.
int folds_input(issl_folds *f, uint64_t first, uint64_t n)
{
    f->input.release();
    f->ms_input = 0;
    if (n == 0) return ISSL_OK;
    if (int rc = select_device(f->src.device, "the extraction")) return rc;
    HIP_TRY(hipMalloc(&f->input.p, up16(n * kFoldLineBytes)));
    Events<2> ev;
    if (int rc = ev.create()) return rc;
    HIP_TRY(hipEventRecord(ev.e[0], f->stream.s));
    launch_folds_input(f->src, first, n, static_cast<char *>(f->input.p), f->stream.s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], f->stream.s));
    HIP_TRY(hipStreamSynchronize(f->stream.s));
    HIP_TRY(hipEventElapsedTime(&f->ms_input, ev.e[0], ev.e[1]));
    return ISSL_OK;
}

int folds_input_copy(issl_folds *f, uint64_t first, uint64_t n, char *out)
{
    if (int rc = folds_input(f, first, n)) return rc;
    if (n) HIP_TRY(hipMemcpy(out, f->input.p, n * kFoldLineBytes, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

int folds_input_write(issl_folds *f, uint64_t first, uint64_t n, const char *path)
{
    std::unique_ptr<char[]> host(new char[n ? n * kFoldLineBytes : 1]);
    if (int rc = folds_input_copy(f, first, n, host.get())) return rc;
    FILE *fp = std::fopen(path, "wb");
    if (!fp) {
        set_error(std::string("cannot open ") + path + ": " + std::strerror(errno));
        return ISSL_E_IO;
    }
    const size_t wrote = std::fwrite(host.get(), 1, n * kFoldLineBytes, fp);
    const int closed = std::fclose(fp);
    if (wrote != n * kFoldLineBytes || closed != 0) {
        set_error(std::string("cannot write ") + path + ": " + std::strerror(errno));
        return ISSL_E_IO;
    }
    return ISSL_OK;
}

// Room for `need` bytes of arena; what is there moves along (the spans count from the arena's start).
int reserve_text(issl_folds *f, uint64_t need, uint64_t guess)
{
    if (need <= f->text_cap) return ISSL_OK;
    uint64_t cap = guess > need ? guess : need;
    if (cap < 2 * f->text_cap) cap = 2 * f->text_cap;
    DevBuf grown;
    if (hipMalloc(&grown.p, cap) != hipSuccess) { // the guess was generous: what this page needs, then
        (void)hipGetLastError();
        cap = need;
        HIP_TRY(hipMalloc(&grown.p, cap));
    }
    if (f->text_used) HIP_TRY(hipMemcpyAsync(grown.p, f->text.p, f->text_used, hipMemcpyDeviceToDevice, f->stream.s));
    HIP_TRY(hipStreamSynchronize(f->stream.s));
    std::swap(f->text.p, grown.p);
    f->text_cap = cap;
    return ISSL_OK;
}

int folds_read(issl_folds *f, uint64_t first, uint64_t n, const char *text, uint64_t len)
{
    f->ms_read = 0;
    if (n == 0) return ISSL_OK;
    if (int rc = select_device(f->src.device, "the extraction")) return rc;
    hipStream_t stream = f->stream.s;
    const uint64_t base = up16(f->text_used);
    const uint64_t padded = (len + kFoldGroupBytes - 1) / kFoldGroupBytes * kFoldGroupBytes + kFoldGroupBytes;
    // the pages still to come are taken to look like this one, up to four times RNAfold's own 211 bytes per row: a page
    // with a superset of pairs or one long line must not reserve memory by its own measure for every row behind it
    const uint64_t rest = f->src.n_fold - f->n_read - n;
    uint64_t per_row = (len + len / 16) / n + 1; // (integers: nothing to overflow, len < 2^63)
    if (per_row > 4 * 211) per_row = 4 * 211;
    const uint64_t guess = base + padded + (rest ? per_row * rest + 4096 : 0);
    if (int rc = reserve_text(f, base + padded, guess)) return rc;
    uint8_t *d_text = static_cast<uint8_t *>(f->text.p) + base;
    if (len) HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_text + len, 0, padded - len, stream));
    DevBuf work;
    HIP_TRY(hipMalloc(&work.p, folds_read_work(n, len) + 256));
    const uint64_t fine = kFoldNoError;
    HIP_TRY(hipMemcpyAsync(f->error.p, &fine, 8, hipMemcpyHostToDevice, stream));
    FoldRead r{};
    r.text = d_text;
    r.len = len;
    r.base = base;
    r.last_line = folds_text::last_line_start(reinterpret_cast<const uint8_t *>(text), len);
    r.first = first;
    r.n = n;
    r.folds = static_cast<issl_fold *>(f->folds.p);
    r.spans = static_cast<issl_text_span *>(f->spans.p);
    r.error = static_cast<uint64_t *>(f->error.p);
    r.work = work.p;
    Events<2> ev;
    if (int rc = ev.create()) return rc;
    HIP_TRY(hipEventRecord(ev.e[0], stream));
    HIP_TRY(launch_folds_read(f->src, r, stream));
    HIP_TRY(hipEventRecord(ev.e[1], stream));
    uint64_t error = kFoldNoError;
    HIP_TRY(hipMemcpyAsync(&error, f->error.p, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // the one wait: the rows are written and the work buffer may go
    HIP_TRY(hipEventElapsedTime(&f->ms_read, ev.e[0], ev.e[1]));
    if (error != kFoldNoError) { // nothing of this page is kept: its rows can be read again
        launch_folds_clear(r.folds, r.spans, first, n, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t row = error >> 8;
        const uint32_t kind = static_cast<uint32_t>(error & 0xFF);
        if (kind == folds_text::kFormat) {
            set_error("RNAfold's lines for row " + std::to_string(row) +
                      " of the fold list: no blank between structure and energy, or no number in the parentheses");
            return ISSL_E_FORMAT;
        }
        set_error("RNAfold's lines for row " + std::to_string(row) +
                  " of the fold list: a number of more than 15 digits, or a line of 2^32 - 1 bytes or more");
        return ISSL_E_UNSUPPORTED;
    }
    f->text_used = base + padded;
    f->text_bytes += len;
    f->n_read += n;
    auto at = f->read.begin();
    while (at != f->read.end() && at->first < first) ++at;
    f->read.insert(at, std::make_pair(first, first + n));
    return ISSL_OK;
}

int folds_read_file(issl_folds *f, uint64_t first, uint64_t n, const char *path)
{
    std::vector<char> text;
    if (int rc = read_whole_file(path, text)) return rc;
    return folds_read(f, first, n, text.data(), text.size());
}

} // namespace
} // namespace issl

extern "C" {

int issl_folds_open(const issl_consensus *c, issl_folds **out)
{
    if (out) *out = nullptr;
    if (!c || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::folds_open(c, out); });
}

int issl_folds_info(const issl_folds *f, uint64_t *n_fold, uint64_t *n_read, uint64_t *text_bytes, uint32_t *bytes_per_group)
{
    if (!f) return issl::fail(ISSL_E_ARG, "null argument");
    if (n_fold) *n_fold = f->src.n_fold;
    if (n_read) *n_read = f->n_read;
    if (text_bytes) *text_bytes = f->text_bytes;
    if (bytes_per_group) *bytes_per_group = issl::kFoldGroupBytes;
    return ISSL_OK;
}

int issl_folds_times(const issl_folds *f, double *ms_input, double *ms_read)
{
    if (!f) return issl::fail(ISSL_E_ARG, "null argument");
    if (ms_input) *ms_input = f->ms_input;
    if (ms_read) *ms_read = f->ms_read;
    return ISSL_OK;
}

int issl_folds_input(issl_folds *f, uint64_t first, uint64_t n, const char **d_text, uint64_t *n_bytes)
{
    if (d_text) *d_text = nullptr;
    if (n_bytes) *n_bytes = 0;
    if (!f || !d_text || !n_bytes) return issl::fail(ISSL_E_ARG, "null argument");
    if (int rc = issl::in_list(f, first, n)) return rc;
    const int rc = issl::abi_call([&] { return issl::folds_input(f, first, n); });
    if (rc) return rc;
    *d_text = static_cast<const char *>(f->input.p);
    *n_bytes = n * issl::kFoldLineBytes;
    return ISSL_OK;
}

int issl_folds_input_copy(issl_folds *f, uint64_t first, uint64_t n, char *out, size_t cap)
{
    if (!f) return issl::fail(ISSL_E_ARG, "null argument");
    if (int rc = issl::in_list(f, first, n)) return rc;
    if (!out && n) return issl::fail(ISSL_E_ARG, "null argument");
    if (cap < n * issl::kFoldLineBytes) {
        issl::set_error("room for " + std::to_string(cap) + " bytes, the lines have " + std::to_string(n * issl::kFoldLineBytes));
        return ISSL_E_ARG;
    }
    return issl::abi_call([&] { return issl::folds_input_copy(f, first, n, out); });
}

int issl_folds_input_write(issl_folds *f, uint64_t first, uint64_t n, const char *path)
{
    if (!f || !path) return issl::fail(ISSL_E_ARG, "null argument");
    if (int rc = issl::in_list(f, first, n)) return rc;
    return issl::abi_call([&] { return issl::folds_input_write(f, first, n, path); });
}

static int readable(const issl_folds *f, uint64_t first, uint64_t n)
{
    if (int rc = issl::in_list(f, first, n)) return rc;
    for (const auto &run : f->read)
        if (n && first < run.second && run.first < first + n) {
            issl::set_error("rows " + std::to_string(run.first) + " .. " + std::to_string(run.second) + " of the fold list are read already");
            return ISSL_E_STATE;
        }
    return ISSL_OK;
}

int issl_folds_read(issl_folds *f, uint64_t first, uint64_t n, const char *text, size_t len)
{
    if (!f || (!text && len)) return issl::fail(ISSL_E_ARG, "null argument");
    if (int rc = readable(f, first, n)) return rc;
    return issl::abi_call([&] { return issl::folds_read(f, first, n, text ? text : "", len); });
}

int issl_folds_read_file(issl_folds *f, uint64_t first, uint64_t n, const char *path)
{
    if (!f || !path) return issl::fail(ISSL_E_ARG, "null argument");
    if (int rc = readable(f, first, n)) return rc;
    return issl::abi_call([&] { return issl::folds_read_file(f, first, n, path); });
}

int issl_folds_device(const issl_folds *f, const issl_fold **d_folds, const issl_text_span **d_spans)
{
    if (!f || !d_folds || !d_spans) return issl::fail(ISSL_E_ARG, "null argument");
    *d_folds = static_cast<const issl_fold *>(f->folds.p);
    *d_spans = static_cast<const issl_text_span *>(f->spans.p);
    return ISSL_OK;
}

int issl_folds_text_device(const issl_folds *f, const char **d_text, uint64_t *n_bytes)
{
    if (!f || !d_text || !n_bytes) return issl::fail(ISSL_E_ARG, "null argument");
    *d_text = static_cast<const char *>(f->text.p);
    *n_bytes = f->text_used;
    return ISSL_OK;
}

int issl_folds_copy(const issl_folds *f, issl_fold *folds, issl_text_span *spans, size_t cap)
{
    if (!f) return issl::fail(ISSL_E_ARG, "null argument");
    if (cap < f->src.n_fold) {
        issl::set_error("room for " + std::to_string(cap) + " rows, the fold list has " + std::to_string(f->src.n_fold));
        return ISSL_E_ARG;
    }
    if (f->src.n_fold == 0) return ISSL_OK;
    return issl::abi_call([&]() -> int {
        if (folds)
            if (int rc = issl::copy_to_host(f->src.device, folds, f->folds.p, 16 * f->src.n_fold)) return rc;
        if (spans)
            if (int rc = issl::copy_to_host(f->src.device, spans, f->spans.p, 48 * f->src.n_fold)) return rc;
        return ISSL_OK;
    });
}

int issl_folds_text_copy(const issl_folds *f, uint64_t fold_row, int which, char *out, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (!f || !len || which < 0 || which > 2) return issl::fail(ISSL_E_ARG, "null argument, or a column other than 0, 1, 2");
    if (int rc = issl::in_list(f, fold_row, 1)) return rc;
    return issl::abi_call([&]() -> int {
        issl_text_span s;
        if (int rc = issl::copy_to_host(f->src.device, &s, static_cast<const issl_text_span *>(f->spans.p) + 3 * fold_row + which, 16)) return rc;
        if (s.length == issl::folds_text::kNoText) {
            *len = ~size_t(0);
            return ISSL_OK;
        }
        *len = s.length;
        if (s.length > cap || (s.length && !out)) {
            issl::set_error("room for " + std::to_string(cap) + " bytes, the text has " + std::to_string(s.length));
            return ISSL_E_ARG;
        }
        if (s.offset > f->text_used || s.length > f->text_used - s.offset) return issl::fail(ISSL_E_DEVICE, "a span outside the pages' text");
        if (s.length) return issl::copy_to_host(f->src.device, out, static_cast<const char *>(f->text.p) + s.offset, s.length);
        return ISSL_OK;
    });
}

int issl_folds_close(issl_folds *f)
{
    if (!f) return ISSL_OK;
    if (f->src.device >= 0) (void)hipSetDevice(f->src.device);
    delete f;
    return ISSL_OK;
}

} // extern "C"
