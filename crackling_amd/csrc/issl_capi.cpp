// The extern "C" surface of libissl_hip.so (include/issl_hip.h).  Every entry point checks its arguments and calls into
// issl_upload.cpp (the HBM image) or issl_pipeline.cpp (scoring) through abi_call, which turns what the C++ underneath
// throws into an error code.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "issl_index.hpp"

using namespace issl;

namespace issl {

int build_from_device_sites(const uint64_t *d_sigs, const uint32_t *d_occ, size_t n_sites, size_t n_lines, size_t seq_len,
                            size_t slice_width, int device, const char *options, issl_index **out)
{
    int rc = select_device(device, "the ISSL scorer");
    if (rc) return rc;
    const uint32_t n_slices = static_cast<uint32_t>((seq_len * 2) / slice_width);
    std::vector<uint64_t> sizes(size_t(n_slices) << slice_width);
    rc = launch_bucket_sizes(d_sigs, n_sites, static_cast<uint32_t>(slice_width), n_slices, sizes.data());
    if (rc) return rc;
    std::unique_ptr<HostIndex> h(new HostIndex());
    rc = h->init_from_bucket_sizes(sizes.data(), n_sites, n_lines, seq_len, slice_width);
    if (rc) return rc;
    return build_on_device(std::move(h), d_sigs, d_occ, true, device, options, out);
}

} // namespace issl

extern "C" {

const char *issl_last_error(void) { return get_error(); }
int issl_abi_version(void) { return ISSL_ABI_VERSION; }

int issl_index_open(const char *path, issl_index **out)
{
    if (!path || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return new_index([&](HostIndex &h) { return h.open_file(path); }, out); });
}

int issl_index_from_memory(const void *image, size_t len, issl_index **out)
{
    if (!image || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return new_index([&](HostIndex &h) { return h.from_memory(image, len); }, out); });
}

int issl_index_build_from_text(const char *text, size_t n_lines, size_t seq_len, size_t slice_width,
                               issl_index **out)
{
    if (!text || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return new_index([&](HostIndex &h) { return h.build_from_text(text, n_lines, seq_len, slice_width); }, out); });
}

int issl_index_build_from_sites(const uint64_t *sigs, const uint32_t *occ, size_t n_sites, size_t n_lines,
                                size_t seq_len, size_t slice_width, issl_index **out)
{
    if (!sigs || !occ || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return new_index([&](HostIndex &h) { return h.build_from_sites(sigs, occ, n_sites, n_lines, seq_len, slice_width); }, out); });
}

int issl_index_write(const issl_index *idx, const char *path)
{
    if (!idx || !path) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&]() -> int {
        if (!idx->host) { set_error("index was attached from a device image and has no host arrays"); return ISSL_E_STATE; }
        if (idx->host->has_arrays()) return idx->host->write_file(path);
        // built on the device: header, score table and bucket sizes come from the host side, sites and slice lists are
        // streamed out of the HBM image
        if (!idx->d_image) { set_error("index has neither host arrays nor a device image"); return ISSL_E_STATE; }
        HIP_TRY(hipSetDevice(idx->device));
        FILE *fp = std::fopen(path, "wb");
        if (!fp) {
            set_error(std::string("cannot write index file '") + path + "': " + std::strerror(errno));
            return ISSL_E_IO;
        }
        bool ok = idx->host->write_leading_sections(fp) == ISSL_OK;
        const uint8_t *base = static_cast<const uint8_t *>(idx->d_image);
        const uint8_t *cold = static_cast<const uint8_t *>(idx->h_cold);
        std::vector<uint8_t> stage;
        bool sig_words = false;
        auto stream_dev = [&](const uint8_t *src, uint64_t bytes) { // device memory, through a 64 MiB staging buffer
            stage.resize(size_t(64) << 20);
            for (uint64_t at = 0; ok && at < bytes; at += stage.size()) {
                const size_t len = static_cast<size_t>(std::min<uint64_t>(stage.size(), bytes - at));
                ok = hipMemcpy(stage.data(), src + at, len, hipMemcpyDeviceToHost) == hipSuccess;
                if (ok && sig_words) { // the site table of a sorted image carries a copy of the counts above the signatures
                    uint64_t *w = reinterpret_cast<uint64_t *>(stage.data());
                    for (size_t i = 0; i < len / 8; ++i) w[i] &= kSigMask;
                }
                ok = ok && std::fwrite(stage.data(), 1, len, fp) == len;
            }
        };
        auto stream_out = [&](uint64_t off, uint64_t bytes, bool in_host) {
            if (in_host) { // the section already sits in host memory
                ok = ok && std::fwrite(cold + off, 1, bytes, fp) == bytes;
                return;
            }
            stream_dev(base + off, bytes);
        };
        sig_words = idx->hdr.off_sub_start != 0;
        stream_out(idx->hdr.off_sites, 8 * idx->geo.n_sites, (idx->hdr.cold_on_host & 2u) != 0);
        sig_words = false;
        ok = ok && std::fwrite(idx->host->sizes, 8, idx->geo.n_buckets(), fp) == idx->geo.n_buckets();
        if (idx->hdr.lists_absent) {
            // The image holds no slice lists: on a sorted layout they are a function of the site table and the counts -- the
            // stable counting sort of isslCreateIndex.cpp:218-234 --, made again here, one slice at a time.
            std::unique_ptr<void, hipError_t (*)(void *)> list_mem(nullptr, hipFree);
            const uint64_t n = idx->geo.n_sites;
            void *p = nullptr;
            if (hipMalloc(&p, std::max<uint64_t>(8 * n, 8)) != hipSuccess) {
                (void)hipGetLastError();
                std::fclose(fp);
                set_error("no device memory to rebuild the slice lists of this image (8 B per site)");
                return ISSL_E_DEVICE;
            }
            list_mem.reset(p);
            for (uint64_t sl = 0; ok && sl < idx->geo.n_slices; ++sl) {
                int brc = launch_build_entries(reinterpret_cast<const uint64_t *>(base + idx->hdr.off_sites),
                                               reinterpret_cast<const uint32_t *>(base + idx->hdr.off_site_occ), n, static_cast<uint32_t>(sl),
                                               static_cast<uint32_t>(sl + 1), static_cast<uint32_t>(idx->geo.slice_width),
                                               static_cast<uint64_t *>(list_mem.get()));
                if (brc) { std::fclose(fp); return brc; }
                stream_dev(static_cast<const uint8_t *>(list_mem.get()), 8 * n);
            }
        } else {
            stream_out(idx->hdr.off_entries, 8 * idx->geo.n_sites * idx->geo.n_slices, (idx->hdr.cold_on_host & 1u) != 0);
        }
        ok = (std::fclose(fp) == 0) && ok;
        if (!ok) {
            set_error(std::string("could not write '") + path + "' from the device image");
            return ISSL_E_IO;
        }
        return ISSL_OK;
    });
}

int issl_index_header(const issl_index *idx, issl_header *out)
{
    if (!idx || !out) return issl::fail(ISSL_E_ARG, "null argument");
    out->n_sites = idx->geo.n_sites;
    out->seq_len = idx->geo.seq_len;
    out->n_lines = idx->geo.n_lines;
    out->slice_width = idx->geo.slice_width;
    out->n_slices = idx->geo.n_slices;
    out->n_scores = idx->geo.n_scores;
    return ISSL_OK;
}

int issl_index_bucket_sizes(const issl_index *idx, uint64_t *out, size_t n)
{
    if (!idx || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (n < idx->bucket_sizes.size()) { set_error("bucket size buffer too small"); return ISSL_E_ARG; }
    std::copy(idx->bucket_sizes.begin(), idx->bucket_sizes.end(), out);
    return ISSL_OK;
}

int issl_index_close(issl_index *idx)
{
    if (!idx) return ISSL_OK;
    release_device(idx);
    delete idx;
    return ISSL_OK;
}

int issl_index_device_bytes(const issl_index *idx, size_t *out)
{
    if (!idx || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (idx->d_image) { *out = idx->hdr.total_bytes; return ISSL_OK; }
    if (!idx->host) { set_error("index has neither host arrays nor a device image"); return ISSL_E_STATE; }
    return abi_call([&] { return planned_image_bytes(idx, out); });
}

// Read-only keys that describe lane 0's scoring workspace (0 before the first batch): what a caller -- a test of a
// long-lived handle -- reads to see which state the handle has reached.  Resolved here, where the handle is known;
// the option table (issl_options.cpp) knows nothing of workspaces.
static bool workspace_option(const issl_index *idx, const char *key, long long *value)
{
    const Workspace &w = idx->lane.ws;
    const bool used = w.cap_guides != 0;
    const struct { const char *key; long long v; } keys[] = {
        {"ws_cap_guides", static_cast<long long>(w.cap_guides)},
        {"ws_slot_width", used ? static_cast<long long>(w.slot_width) : 0}, // (the member starts at kSlotHits)
        {"ws_fine_ways", static_cast<long long>(w.fine_ways)},
        {"ws_cap_chunks", static_cast<long long>(w.cap_chunks)},
        {"ws_cap_fitems", static_cast<long long>(w.cap_fitems)},
        {"ws_lean", idx->lane.lean ? 1 : 0},
        {"ws_scan_verified", static_cast<long long>(idx->lane.scan_verified)},
        {"ws_scan_lds_buffers", static_cast<long long>(idx->lane.scan_lds_buffers)},
        {"ws_scan_raw_top", static_cast<long long>(idx->lane.scan_raw_top)},
        {"ws_raw_chunks", static_cast<long long>(idx->lane.raw_chunks)},
    };
    for (const auto &k : keys)
        if (std::strcmp(k.key, key) == 0) {
            if (value) *value = k.v;
            return true;
        }
    return false;
}

int issl_index_set_option(issl_index *idx, const char *key, const char *value)
{
    if (!idx || !key || !value) return issl::fail(ISSL_E_ARG, "null argument");
    if (workspace_option(idx, key, nullptr)) {
        return abi_call([&]() -> int {
            set_error(std::string("read-only option: ") + key);
            return ISSL_E_ARG;
        });
    }
    if (idx->n_pending) { set_error("issl_index_set_option: batches are in flight, call issl_score_finish first"); return ISSL_E_STATE; }
    return abi_call([&]() -> int {
        Tuning t = idx->tuning;
        if (!t.set(key, value)) {
            set_error(std::string("unknown option or value out of range: ") + key + "=" + value);
            return ISSL_E_ARG;
        }
        if (idx->d_image && t.scan_blocks != idx->tuning.scan_blocks) {
            // every scan wave owns the raw chunk with its own number: keep at least that many
            HIP_TRY(hipSetDevice(idx->device));
            for (Lane *lp : {&idx->lane, &idx->lane2})
                if (lp->ws.cap_chunks && lp->ws.cap_chunks < size_t(scan_waves(t)) * 2) {
                    int rc = ensure_raw_capacity(lp->ws, size_t(scan_waves(t)) * 4);
                    if (rc) return rc;
                }
        }
        idx->tuning = t;
        return ISSL_OK;
    });
}

int issl_index_get_option(const issl_index *idx, const char *key, long long *value)
{
    if (!idx || !key || !value) return issl::fail(ISSL_E_ARG, "null argument");
    if (idx->tuning.get(key, value) || image_option(idx->d_image ? &idx->hdr : nullptr, key, value) || workspace_option(idx, key, value)) return ISSL_OK;
    return abi_call([&]() -> int {
        set_error(std::string("unknown option: ") + key);
        return ISSL_E_ARG;
    });
}

int issl_index_build_on_device_opt(const uint64_t *sigs, const uint32_t *occ, size_t n_sites, size_t n_lines,
                                   size_t seq_len, size_t slice_width, int device, const char *options, issl_index **out)
{
    if (!sigs || !occ || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&]() -> int {
        std::unique_ptr<HostIndex> h(new HostIndex());
        int rc = h->init_without_arrays(sigs, n_sites, n_lines, seq_len, slice_width);
        if (rc) return rc;
        return build_on_device(std::move(h), sigs, occ, false, device, options, out);
    });
}


int issl_index_build_from_device_sites(const uint64_t *d_sigs, const uint32_t *d_occ, size_t n_sites, size_t n_lines,
                                       size_t seq_len, size_t slice_width, int device, const char *options, issl_index **out)
{
    if (!d_sigs || !d_occ || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (seq_len == 0 || seq_len > 32 || slice_width < 2 || slice_width > 8 || (seq_len * 2) / slice_width == 0 ||
        (seq_len * 2) / slice_width > kMaxSlices) {
        set_error("bad sequence length or slice width");
        return ISSL_E_ARG;
    }
    return abi_call([&] { return build_from_device_sites(d_sigs, d_occ, n_sites, n_lines, seq_len, slice_width, device, options, out); });
}

int issl_index_build_on_device(const uint64_t *sigs, const uint32_t *occ, size_t n_sites, size_t n_lines,
                               size_t seq_len, size_t slice_width, int device, issl_index **out)
{
    return issl_index_build_on_device_opt(sigs, occ, n_sites, n_lines, seq_len, slice_width, device, nullptr, out);
}

int issl_device_memory(int device, size_t *free_bytes, size_t *total_bytes)
{
    if (!free_bytes || !total_bytes) return issl::fail(ISSL_E_ARG, "null argument");
    int rc = select_device(device, "the ISSL scorer");
    if (rc) return rc;
    HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return ISSL_OK;
}

int issl_index_upload(issl_index *idx, int device)
{
    if (!idx) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return upload_common(idx, device, nullptr, 0); });
}

int issl_index_upload_into(issl_index *idx, int device, void *dev_buf, size_t bytes)
{
    if (!dev_buf) { set_error("null device buffer"); return ISSL_E_ARG; }
    if (!idx) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return upload_common(idx, device, dev_buf, bytes); });
}


int issl_index_attach_image(int device, void *dev_buf, size_t bytes, issl_index **out)
{
    return abi_call([&] { return attach_common(device, dev_buf, bytes, nullptr, 0, out); });
}

int issl_index_attach_image_cold(int device, void *dev_buf, size_t bytes, void *cold_host, size_t cold_bytes,
                                 issl_index **out)
{
    return abi_call([&] { return attach_common(device, dev_buf, bytes, cold_host, cold_bytes, out); });
}

int issl_index_cold(const issl_index *idx, void **host_ptr, size_t *bytes)
{
    if (!idx || !host_ptr || !bytes) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image"); return ISSL_E_STATE; }
    *host_ptr = idx->hdr.cold_on_host ? idx->h_cold : nullptr;
    *bytes = idx->hdr.cold_on_host ? idx->hdr.cold_bytes : 0;
    return ISSL_OK;
}

int issl_index_image(const issl_index *idx, void **dev_ptr, size_t *bytes)
{
    if (!idx || !dev_ptr || !bytes) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image"); return ISSL_E_STATE; }
    *dev_ptr = idx->d_image;
    *bytes = idx->hdr.total_bytes;
    return ISSL_OK;
}

int issl_index_copy_image_to(const issl_index *idx, void *dev_dst, size_t bytes)
{
    if (!idx || !dev_dst) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image"); return ISSL_E_STATE; }
    if (bytes < idx->hdr.total_bytes || (reinterpret_cast<uintptr_t>(dev_dst) & 255u)) {
        set_error("destination too small or not 256-byte aligned");
        return ISSL_E_ARG;
    }
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipMemcpy(dev_dst, idx->d_image, idx->hdr.total_bytes, hipMemcpyDeviceToDevice));
    return ISSL_OK;
}

// (issl_encode_guides, issl_decode_guide, issl_method_from_string, issl_verdicts, issl_read_query_file,
// issl_format_scores: issl_text.cpp)

void issl_free(void *p) { std::free(p); }

int issl_score_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, double threshold,
                      int method, double *d_mit, double *d_cfd, void *stream)
{
    if (!idx || (n && (!d_guides || !d_mit || !d_cfd))) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&]() -> int {
        return score_core(idx, d_guides, n, max_dist, threshold, method, d_mit, d_cfd, static_cast<hipStream_t>(stream), false);
    });
}

int issl_score_device_async(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, double threshold,
                            int method, double *d_mit, double *d_cfd, void *stream)
{
    if (!idx || (n && (!d_guides || !d_mit || !d_cfd))) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image: call issl_index_upload first"); return ISSL_E_STATE; }
    if (n == 0) return ISSL_OK;
    if (n > kMaxBatch) { // before any workspace is sized for it
        set_error("at most 2^24 guides per device batch (issl_score splits larger batches itself)");
        return ISSL_E_ARG;
    }
    return abi_call([&]() -> int {
        return score_async(idx, d_guides, n, max_dist, threshold, method, d_mit, d_cfd, static_cast<hipStream_t>(stream));
    });
}

int issl_score_wait(issl_index *idx, void *stream)
{
    if (!idx) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return wait_batches(idx, static_cast<hipStream_t>(stream)); });
}

int issl_score_finish(issl_index *idx, void *stream)
{
    if (!idx) return issl::fail(ISSL_E_ARG, "null argument");
    return abi_call([&] { return finish_batches(idx, static_cast<hipStream_t>(stream)); });
}

int issl_score(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
               double *mit, double *cfd)
{
    if (!idx || (n && (!guides || !mit || !cfd))) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image: call issl_index_upload first"); return ISSL_E_STATE; }
    if (n == 0) return ISSL_OK;
    return abi_call([&] { return score_host(idx, guides, n, max_dist, threshold, method, mit, cfd); });
}

int issl_dump_hits(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
                   issl_hit *hits, size_t cap, size_t *n_hits)
{
    if (!idx || !n_hits || (n && !guides) || (cap && !hits)) return issl::fail(ISSL_E_ARG, "null argument");
    if (!idx->d_image) { set_error("index has no device image: call issl_index_upload first"); return ISSL_E_STATE; }
    *n_hits = 0;
    if (n == 0) return ISSL_OK;
    if (n > (size_t(1) << 22)) { set_error("issl_dump_hits takes at most 2^22 guides per call"); return ISSL_E_ARG; }
    return abi_call([&] { return dump_hits(idx, guides, n, max_dist, threshold, method, hits, cap, n_hits); });
}

// Off-target report: arguments first (without a device), then the state of the handle.
static int report_args(const issl_index *idx, bool pointers, int max_dist)
{
    if (!idx || !pointers) return issl::fail(ISSL_E_ARG, "null argument");
    if (max_dist < 0 || max_dist >= ISSL_PROFILE_BINS) { set_error("max_dist must lie in 0..6 for the off-target report"); return ISSL_E_ARG; }
    if (!idx->d_image) { set_error("index has no device image: call issl_index_upload first"); return ISSL_E_STATE; }
    return ISSL_OK;
}

int issl_offtarget_profile(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, issl_profile *out)
{
    if (int rc = report_args(idx, !n || (guides && out), max_dist)) return rc;
    if (n == 0) return ISSL_OK;
    return abi_call([&] { return profile_host(idx, guides, n, max_dist, out); });
}

int issl_offtarget_profile_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, issl_profile *d_out,
                                  void *stream)
{
    if (int rc = report_args(idx, !n || (d_guides && d_out), max_dist)) return rc;
    return abi_call([&] { return profile_device(idx, d_guides, n, max_dist, d_out, static_cast<hipStream_t>(stream)); });
}

int issl_offtargets(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, uint64_t *offsets, issl_offtarget *recs,
                    size_t cap, size_t *n_total)
{
    if (int rc = report_args(idx, offsets && n_total && (!n || guides) && (!cap || recs), max_dist)) return rc;
    return abi_call([&] { return offtargets_host(idx, guides, n, max_dist, offsets, recs, recs ? cap : 0, n_total); });
}

int issl_offtargets_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, uint64_t *d_offsets,
                           issl_offtarget *d_recs, size_t cap, size_t *n_total, void *stream)
{
    if (int rc = report_args(idx, d_offsets && n_total && (!n || d_guides) && (!cap || d_recs), max_dist)) return rc;
    return abi_call([&] {
        return offtargets_device(idx, d_guides, n, max_dist, d_offsets, d_recs, d_recs ? cap : 0, n_total, static_cast<hipStream_t>(stream));
    });
}

int issl_last_stats(const issl_index *idx, issl_stats *out)
{
    if (!idx || !out) return issl::fail(ISSL_E_ARG, "null argument");
    *out = idx->stats;
    return ISSL_OK;
}

int issl_count_candidates(const issl_index *idx, const uint64_t *guides, size_t n, uint64_t *out)
{
    if (!idx || !out || (n && !guides)) return issl::fail(ISSL_E_ARG, "null argument");
    const uint64_t per = idx->geo.buckets_per_slice();
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i)
        for (uint64_t s = 0; s < idx->geo.n_slices; ++s)
            total += idx->bucket_sizes[s * per + ((guides[i] >> (idx->geo.slice_width * s)) & (per - 1))];
    *out = total;
    return ISSL_OK;
}

} // extern "C"
