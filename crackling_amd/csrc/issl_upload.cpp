// The HBM image of an index: layout choice, upload (FileUploader's pinned ring for file-mapped indexes), attach of an
// image made elsewhere.  Host code; the kernels that build the image are in issl_build.hip and issl_bin.hip.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <unistd.h>

#include "issl_index.hpp"

namespace issl {

static uint64_t align256(uint64_t x) { return (x + 255ull) & ~255ull; }

void layout_image(ImageHeader &h, const Geometry &g, uint64_t n_scores_unique, uint64_t n_tiles, bool dense_mit,
                  const LayoutSpec &spec)
{
    std::memset(&h, 0, sizeof h);
    h.magic = kImageMagic;
    h.version = kImageVersion;
    h.kind = 0;
    h.n_sites = g.n_sites;
    h.seq_len = g.seq_len;
    h.n_lines = g.n_lines;
    h.slice_width = g.slice_width;
    h.n_slices = g.n_slices;
    h.n_scores_file = g.n_scores;
    h.n_buckets = g.n_buckets();
    h.n_scores_unique = n_scores_unique;
    h.n_tiles = n_tiles;
    h.tile_cands = kTileCands;
    const bool no_lists = spec.no_lists && spec.sorted != 0 && spec.cold == 0;
    const uint64_t sites_b = align256(8 * g.n_sites), lists_b = no_lists ? 0 : align256(8 * g.n_sites * g.n_slices);
    h.lists_absent = no_lists ? 1 : 0;
    const bool esig = spec.inline_sigs && spec.cold == 0 && spec.sorted == 0; // in-list signatures: list-order layouts in HBM
    uint64_t off = kHeaderBytes, cold_off = 0;
    h.off_bucket_start = off; off = align256(off + 8 * (h.n_buckets + 1));
    h.off_tile_first = off;   off = align256(off + 4 * (h.n_buckets + 1));
    h.off_score_mask = off;   off = align256(off + 8 * n_scores_unique);
    h.off_score_val = off;    off = align256(off + 8 * n_scores_unique);
    if (dense_mit) { h.off_mit_dense = off; off = align256(off + 8ull * (1u << 20)); }
    h.cold_on_host = spec.cold;
    // the cold sections form a buffer of their own (pinned host memory): site table first, then the slice lists
    if (spec.cold & 2u) { h.off_sites = cold_off; cold_off += sites_b; } else { h.off_sites = off; off += sites_b; }
    if (spec.cold & 1u) { h.off_entries = cold_off; cold_off += lists_b; } else { h.off_entries = off; off += lists_b; }
    h.cold_bytes = spec.cold ? cold_off : sites_b + lists_b + (esig ? lists_b : 0);
    h.off_scan = off;         off = align256(off + 4ull * kTileCands * n_tiles);
    if (esig) { h.off_esig = off; off += lists_b; }
    if (spec.cold == 3u) { h.off_occ8 = off; off = align256(off + g.n_sites * g.n_slices); }
    if (spec.sorted) {
        h.off_sub_start = off; off = align256(off + 4 * h.n_buckets * 257);
        if (spec.sorted == 1) { h.off_srec = off; off = align256(off + sizeof(StreamRec) * kTileCands * n_tiles); }
        else                  { h.off_sid = off;  off = align256(off + 4ull * kTileCands * n_tiles); }
        h.off_site_occ = off; off = align256(off + 4 * g.n_sites);
    }
    h.total_bytes = off;
}

ImageView make_view(const ImageHeader &h, void *base, void *cold)
{
    uint8_t *p = static_cast<uint8_t *>(base);
    uint8_t *c = static_cast<uint8_t *>(cold);
    ImageView v;
    v.bucket_start = reinterpret_cast<const uint64_t *>(p + h.off_bucket_start);
    v.tile_first = reinterpret_cast<const uint32_t *>(p + h.off_tile_first);
    v.score_mask = reinterpret_cast<const uint64_t *>(p + h.off_score_mask);
    v.score_val = reinterpret_cast<const double *>(p + h.off_score_val);
    v.mit_dense = h.off_mit_dense ? reinterpret_cast<const double *>(p + h.off_mit_dense) : nullptr;
    v.sites = reinterpret_cast<const uint64_t *>(((h.cold_on_host & 2u) ? c : p) + h.off_sites);
    v.entries = h.lists_absent ? nullptr : reinterpret_cast<const uint64_t *>(((h.cold_on_host & 1u) ? c : p) + h.off_entries);
    v.esig = h.off_esig ? reinterpret_cast<const uint64_t *>(p + h.off_esig) : nullptr;
    v.occ8 = h.off_occ8 ? reinterpret_cast<const uint8_t *>(p + h.off_occ8) : nullptr;
    v.sub_start = h.off_sub_start ? reinterpret_cast<const uint32_t *>(p + h.off_sub_start) : nullptr;
    v.srec = h.off_srec ? reinterpret_cast<const StreamRec *>(p + h.off_srec) : nullptr;
    v.sid = h.off_sid ? reinterpret_cast<const uint32_t *>(p + h.off_sid) : nullptr;
    v.site_occ = h.off_site_occ ? reinterpret_cast<const uint32_t *>(p + h.off_site_occ) : nullptr;
    v.scan = reinterpret_cast<const uint32_t *>(p + h.off_scan);
    v.n_sites = h.n_sites;
    v.n_buckets = static_cast<uint32_t>(h.n_buckets);
    v.n_scores = static_cast<uint32_t>(h.n_scores_unique);
    v.slice_width = static_cast<uint32_t>(h.slice_width);
    v.n_slices = static_cast<uint32_t>(h.n_slices);
    v.n_tiles = static_cast<uint32_t>(h.n_tiles);
    return v;
}

// The local MIT table can be indexed directly by the 20 mismatch flags when every mask keeps to the even bits
// below bit 40 (always true for tables written by isslCreateIndex.cpp:239-252).
static bool masks_are_dense(const std::vector<uint64_t> &masks)
{
    for (uint64_t m : masks)
        if (m & ~0x5555555555ull) return false;
    return true;
}

static uint32_t dense_index(uint64_t mask)
{
    uint32_t idx = 0;
    for (uint32_t p = 0; p < 20; ++p) idx |= static_cast<uint32_t>((mask >> (2 * p)) & 1ull) << p;
    return idx;
}

// upload_timing knob (ISSL_UPLOAD_TIMING=1): one diagnostic line per upload stage on stderr
static void upload_note(const issl_index *ix, const char *what, double t0)
{
    if (ix->tuning.upload_timing) std::fprintf(stderr, "[issl upload] %s %.1f ms\n", what, now_ms() - t0);
}

// Non-null when the slice lists are to be built on the device (the host index then has no arrays).
struct DeviceBuildInput {
    const uint64_t *sigs;
    const uint32_t *occ;
    bool on_device; // the two arrays are device memory of the upload's device (issl_index_build_from_device_sites)
};

struct DevTemp { // device allocation freed on every path out of a function
    void *p = nullptr;
    ~DevTemp() { if (p) (void)hipFree(p); }
};

// Sections of a file-mapped index into device memory.  hipMemcpy from a FRESH private file mapping moves 11 GB/s on an
// MI355X host (every page of the mapping is faulted in on the way; 56 GB/s once they are), so the 14 GB of a human-scale
// .issl took 0.6 - 0.8 s of a one-shot scorer's second.  Here a few threads pread() the file into a ring of pinned chunks
// and every chunk goes out with its own asynchronous copy: 48 - 53 GB/s, the link's rate (tools/ubench_h2d.cpp,
// profiles/r05_ubench_h2d.txt).  Anything that is not file-backed, or small, takes the plain copy.
// Sections are QUEUED (begin) and waited for one by one (wait): the readers go from the last chunk of one section
// straight to the first of the next while the caller launches the kernels that consume the section that has landed.
// Every reader pins its own two slots when it first needs them (pinning costs ~0.3 ms per MiB: 80 ms for the whole ring
// in one go, before the first byte moved); the ring is given back at the end of the upload, on the uploading thread
// (release(): ~40 ms, upload_note "pinned ring given back").
class FileUploader {
  public:
    // chunk_kib: bytes per pinned slot (default 16 MiB); min_kib: sections smaller than this take the plain copy (default 64 MiB).
    // Both from the upload_chunk_kib / upload_ring_min_kib knobs: tests send a 10 MB golden index through a ring of 64 KiB slots.
    FileUploader(size_t chunk_kib, size_t min_kib, int threads)
        : chunk_(std::max<size_t>(chunk_kib, 4) << 10), min_bytes_(min_kib << 10), n_threads_(static_cast<uint32_t>(std::min(std::max(threads, 1), static_cast<int>(kMaxThreads)))) {}
    ~FileUploader() { abandon_ = true; release(); } // (an upload that failed half way: what is still queued is dropped)
    FileUploader(const FileUploader &) = delete;
    FileUploader &operator=(const FileUploader &) = delete;

    // Queue a section; *ticket names it for wait().  Plain copies are done before this returns.
    int begin(const HostIndex &h, void *dst, const void *src, size_t bytes, int *ticket)
    {
        int fd = -1;
        uint64_t off = 0;
        std::unique_ptr<Job> job(new (std::nothrow) Job());
        if (!job) { set_error("out of memory"); return ISSL_E_NOMEM; }
        if (bytes < std::max<size_t>(min_bytes_, 1) || !h.file_range(src, bytes, &fd, &off) || !ensure()) {
            HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            job->recorded = true; // (nothing to wait for)
            std::lock_guard<std::mutex> lock(mu_);
            jobs_.push_back(std::move(job));
            *ticket = static_cast<int>(jobs_.size() - 1);
            return ISSL_OK;
        }
        job->fd = fd;
        job->off = off;
        job->dst = static_cast<char *>(dst);
        job->src = static_cast<const char *>(src);
        job->bytes = bytes;
        job->n_chunks = (bytes + chunk_ - 1) / chunk_;
        if (hipEventCreateWithFlags(&job->landed, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            set_error("HIP error: cannot create an event for a section of the index");
            return ISSL_E_DEVICE;
        }
        {
            std::lock_guard<std::mutex> lock(mu_);
            jobs_.push_back(std::move(job));
            *ticket = static_cast<int>(jobs_.size() - 1);
            if (pool_.empty()) { // (a thread that cannot be started throws: the destructor joins those that run)
                (void)hipGetDevice(&device_);
                pool_.reserve(n_threads_);
                for (uint32_t w = 0; w < n_threads_; ++w) pool_.emplace_back([this, w] { work(w); });
            }
        }
        cv_work_.notify_all();
        return ISSL_OK;
    }
    // Returns when the section has landed in device memory (or could not be read).
    int wait(int ticket)
    {
        Job *j = nullptr;
        {
            std::unique_lock<std::mutex> lock(mu_);
            if (ticket < 0 || static_cast<size_t>(ticket) >= jobs_.size()) { set_error("internal: no such upload section"); return ISSL_E_STATE; }
            j = jobs_[static_cast<size_t>(ticket)].get();
            cv_done_.wait(lock, [&] { return j->recorded; });
        }
        if (j->landed && !j->failed.load()) HIP_TRY(hipEventSynchronize(j->landed));
        if (j->failed.load() == 2) { set_error("Error reading index: the file shrank or could not be read while it was uploaded"); return ISSL_E_IO; }
        if (j->failed.load()) { (void)hipGetLastError(); set_error("HIP error while a section of the index was uploaded"); return ISSL_E_DEVICE; }
        return ISSL_OK;
    }
    int copy(const HostIndex &h, void *dst, const void *src, size_t bytes)
    {
        int t = -1;
        if (int rc = begin(h, dst, src, bytes, &t)) return rc;
        return wait(t);
    }
    // Stops the readers (they finish what is queued, or drop it once abandoned) and frees everything.  Allocates nothing:
    // the destructor runs it on the way out of an upload that threw.
    void release()
    {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stop_ = true;
        }
        cv_work_.notify_all();
        for (auto &th : pool_) th.join();
        pool_.clear();
        if (stream_) (void)hipStreamSynchronize(stream_);
        for (uint32_t i = 0; i < 2 * kMaxThreads; ++i) {
            if (pin_[i]) (void)hipHostFree(pin_[i]);
            pin_[i] = nullptr;
            if (ev_[i]) (void)hipEventDestroy(ev_[i]);
            ev_[i] = nullptr;
            no_pin_[i] = false;
        }
        for (auto &j : jobs_) if (j->landed) { (void)hipEventDestroy(j->landed); j->landed = nullptr; }
        jobs_.clear();
        head_ = 0;
        if (stream_) (void)hipStreamDestroy(stream_);
        stream_ = nullptr;
        stop_ = false;
        tried_ = false;
    }
    double pin_ms() const { return pin_us_.load() * 1e-3; } // summed over the readers (they pin side by side)

  private:
    static constexpr uint32_t kMaxThreads = 32;
    struct Job {
        int fd = -1;
        uint64_t off = 0;
        char *dst = nullptr;
        const char *src = nullptr;
        size_t bytes = 0, n_chunks = 0;
        size_t next = 0, issued = 0; // under mu_
        std::atomic<int> failed{0};
        hipEvent_t landed = nullptr; // recorded behind the section's last copy
        bool recorded = false;       // under mu_: every chunk has been issued (or given up)
    };
    const size_t chunk_; // 16 slots of 16 MiB by default: 256 MiB of pinned memory while an upload lasts
    const size_t min_bytes_;
    const uint32_t n_threads_; // readers (upload_threads knob, default 8)

    bool ensure() // the copy stream; false: plain copies from here on
    {
        if (stream_) return true;
        if (tried_) return false;
        tried_ = true;
        if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); stream_ = nullptr; return false; }
        return true;
    }
    void work(uint32_t w)
    {
        (void)hipSetDevice(device_);
        for (uint32_t turn = 0;; ++turn) {
            Job *j = nullptr;
            size_t c = 0;
            {
                std::unique_lock<std::mutex> lock(mu_);
                for (;;) {
                    while (head_ < jobs_.size() && jobs_[head_]->next >= jobs_[head_]->n_chunks) ++head_;
                    if (head_ < jobs_.size()) break;
                    if (stop_) return;
                    cv_work_.wait(lock);
                }
                j = jobs_[head_].get();
                c = j->next++;
            }
            const uint32_t slot = w + (turn & 1u) * kMaxThreads; // every reader alternates between its two slots
            const size_t len = std::min(chunk_, j->bytes - c * chunk_);
            bool issued_here = false;
            if (!j->failed.load() && !abandon_.load()) {
                if (!pin_[slot] && !no_pin_[slot]) { // first use: pin it (side by side with the other readers)
                    const double t0 = now_ms();
                    if (hipHostMalloc(&pin_[slot], chunk_, hipHostMallocDefault) != hipSuccess ||
                        hipEventCreateWithFlags(&ev_[slot], hipEventDisableTiming) != hipSuccess) {
                        (void)hipGetLastError();
                        if (pin_[slot]) (void)hipHostFree(pin_[slot]);
                        pin_[slot] = nullptr;
                        no_pin_[slot] = true;
                    }
                    pin_us_ += static_cast<long long>((now_ms() - t0) * 1e3);
                }
                if (!pin_[slot]) { // no pinned memory to be had: this chunk straight from the mapping
                    if (hipMemcpy(j->dst + c * chunk_, j->src + c * chunk_, len, hipMemcpyHostToDevice) != hipSuccess) j->failed = 1;
                } else if (hipEventSynchronize(ev_[slot]) != hipSuccess) { // the slot's previous copy has left it
                    j->failed = 1;
                } else {
                    size_t got = 0;
                    while (got < len) {
                        const ssize_t k = ::pread(j->fd, static_cast<char *>(pin_[slot]) + got, len - got, static_cast<off_t>(j->off + c * chunk_ + got));
                        if (k < 0 && errno == EINTR) continue;
                        if (k <= 0) { j->failed = 2; break; }
                        got += static_cast<size_t>(k);
                    }
                    if (got == len) {
                        std::lock_guard<std::mutex> lock(mu_); // one thread at a time talks to the stream
                        if (hipMemcpyAsync(j->dst + c * chunk_, pin_[slot], len, hipMemcpyHostToDevice, stream_) != hipSuccess ||
                            hipEventRecord(ev_[slot], stream_) != hipSuccess) j->failed = 1;
                        finish_chunk(j);
                        issued_here = true;
                    }
                }
            }
            if (!issued_here) {
                std::lock_guard<std::mutex> lock(mu_);
                finish_chunk(j);
            }
        }
    }
    void finish_chunk(Job *j) // under mu_
    {
        if (++j->issued < j->n_chunks) return;
        if (!j->failed.load() && hipEventRecord(j->landed, stream_) != hipSuccess) j->failed = 1;
        j->recorded = true;
        cv_done_.notify_all();
    }
    void *pin_[2 * kMaxThreads] = {};   // slot w and w + kMaxThreads belong to reader w alone
    hipEvent_t ev_[2 * kMaxThreads] = {};
    bool no_pin_[2 * kMaxThreads] = {};
    hipStream_t stream_ = nullptr;
    int device_ = 0;
    std::mutex mu_; // the queue, the sections' counts, the stream
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::unique_ptr<Job>> jobs_;
    size_t head_ = 0; // first section that still has chunks to hand out
    std::vector<std::thread> pool_;
    bool stop_ = false, tried_ = false;
    std::atomic<bool> abandon_{false};
    std::atomic<long long> pin_us_{0};
};

static int finish_upload(issl_index *ix, const DeviceBuildInput *dbi = nullptr)
{
    const HostIndex &h = *ix->host;
    const Geometry &g = h.geo;
    const uint64_t nb = g.n_buckets();
    const double t_tables = now_ms();
    const hipMemcpyKind dbi_kind = (dbi && dbi->on_device) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint8_t *base = static_cast<uint8_t *>(ix->d_image);
    // The big sections of a file-mapped index are queued first: the readers pin their slots and fill them while this
    // thread makes the tables below (the process's first copy also loads the runtime's copy kernels: 40 ms).
    FileUploader from_file(ix->tuning.upload_chunk_kib, ix->tuning.upload_ring_min_kib, ix->tuning.upload_threads);
    const bool lists_to_image = !dbi && !ix->hdr.lists_absent && !(ix->hdr.cold_on_host & 1u); // slice lists: file -> image, slice by slice
    const bool sites_to_image = !dbi && !(ix->hdr.cold_on_host & 2u);
    int t_sites = -1;
    std::vector<int> t_list(g.n_slices, -1);
    uint64_t *const img_entries = reinterpret_cast<uint64_t *>(base + ix->hdr.off_entries);
    auto begin_list = [&](uint64_t sl) -> int { // (two sections at most are queued ahead of the one waited for)
        if (!lists_to_image || sl >= g.n_slices || t_list[sl] >= 0) return ISSL_OK;
        return from_file.begin(h, img_entries + sl * g.n_sites, h.entries + sl * g.n_sites, 8 * g.n_sites, &t_list[sl]);
    };
    if (sites_to_image)
        if (int crc = from_file.begin(h, base + ix->hdr.off_sites, h.sites, 8 * g.n_sites, &t_sites)) return crc;
    if (int crc = begin_list(0)) return crc;
    // the head of the image -- header, bucket tables, score tables: contiguous -- as ONE copy
    std::vector<uint64_t> masks;
    std::vector<double> vals;
    h.unique_scores(masks, vals);
    std::vector<uint32_t> tfirst(nb + 1);
    {
        const uint64_t head_end = ix->hdr.off_mit_dense ? ix->hdr.off_mit_dense + 8ull * (1u << 20) : ix->hdr.off_score_val + 8 * masks.size();
        std::vector<uint8_t> head(head_end, 0);
        std::memcpy(head.data(), &ix->hdr, sizeof(ImageHeader));
        uint64_t *bstart = reinterpret_cast<uint64_t *>(head.data() + ix->hdr.off_bucket_start);
        bstart[0] = 0;
        tfirst[0] = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            bstart[b + 1] = bstart[b] + h.sizes[b];
            tfirst[b + 1] = tfirst[b] + static_cast<uint32_t>((h.sizes[b] + kTileCands - 1) / kTileCands);
        }
        std::memcpy(head.data() + ix->hdr.off_tile_first, tfirst.data(), 4 * (nb + 1));
        if (!masks.empty()) {
            std::memcpy(head.data() + ix->hdr.off_score_mask, masks.data(), 8 * masks.size());
            std::memcpy(head.data() + ix->hdr.off_score_val, vals.data(), 8 * vals.size());
        }
        if (ix->hdr.off_mit_dense) {
            double *dense = reinterpret_cast<double *>(head.data() + ix->hdr.off_mit_dense);
            for (size_t i = 0; i < masks.size(); ++i) dense[dense_index(masks[i])] = vals[i];
        }
        HIP_TRY(hipMemcpy(base, head.data(), head_end, hipMemcpyHostToDevice));
    }
    ix->view = make_view(ix->hdr, ix->d_image, ix->d_cold);
    DevTemp flag_mem, occ_mem;
    HIP_TRY(hipMalloc(&flag_mem.p, 4));
    uint32_t *flag = static_cast<uint32_t *>(flag_mem.p);
    HIP_TRY(hipMemset(flag, 0, 4));
    uint32_t *scan_out = reinterpret_cast<uint32_t *>(base + ix->hdr.off_scan);
    if (dbi && !ix->hdr.off_sub_start) { // (the sorted layouts keep the counts in the image)
        HIP_TRY(hipMalloc(&occ_mem.p, 4 * g.n_sites));
        HIP_TRY(hipMemcpy(occ_mem.p, dbi->occ, 4 * g.n_sites, dbi_kind));
    }
    const uint32_t *d_occ = static_cast<const uint32_t *>(occ_mem.p);
    DevTemp seen_mem; // list-order layouts: one bit per (slice, site) -- every slice must list every site once
    uint32_t *seen = nullptr;
    if (!ix->hdr.off_sub_start) {
        const uint64_t words = (g.n_sites * g.n_slices + 31) / 32 + 1;
        if (hipMalloc(&seen_mem.p, 4 * words) != hipSuccess) { (void)hipGetLastError(); seen_mem.p = nullptr; return kSortNoRoom; } // the next layout
        HIP_TRY(hipMemset(seen_mem.p, 0, 4 * words));
        seen = static_cast<uint32_t *>(seen_mem.p);
    }
    upload_note(ix, "bucket tables, score table (the file's sections are on their way)", t_tables);
    double t0 = now_ms();
    if (ix->hdr.off_sub_start) {
        // Sorted layouts.  Site table and counts into the image, then one slice at a time: the slice's list (in the
        // image, or -- lists in pinned host memory -- in a temporary 8 B/site device copy), the successor-byte order
        // of its buckets, its part of the stream maps.
        const uint64_t n = g.n_sites;
        uint64_t *d_sites = reinterpret_cast<uint64_t *>(base + ix->hdr.off_sites);
        uint32_t *d_site_occ = reinterpret_cast<uint32_t *>(base + ix->hdr.off_site_occ);
        if (dbi) HIP_TRY(hipMemcpy(d_sites, dbi->sigs, 8 * n, dbi_kind));
        else if (int crc = from_file.wait(t_sites)) return crc;
        if (dbi) HIP_TRY(hipMemcpy(d_site_occ, dbi->occ, 4 * n, dbi_kind)); // (k_fill_maps writes the same again)
        upload_note(ix, "sites", t0);
        t0 = now_ms();
        // lists in pinned host memory, or nowhere (lists_absent): either way a slice's list exists on the device only while
        // the slice is worked on, in one 8 B/site temporary
        const bool lists_kept_cold = (ix->hdr.cold_on_host & 1u) != 0;
        const bool lists_cold = lists_kept_cold || ix->hdr.lists_absent != 0;
        // The scan stream is packed last (from the maps the slices leave behind): until then its section -- 20 B per site --
        // holds the sort keys and the one slice list, so that the construction needs 8 B per site beyond the image
        // (the radix passes' second buffer) and an index of the format's 2^32 - 1 sites (52 + 8 B per site) fits 288 GB.
        const uint64_t scan_bytes = ix->hdr.n_tiles * static_cast<uint64_t>(kTileCands) * 4ull, key_bytes = align256(8 * n);
        const bool lend = scan_bytes >= key_bytes + (lists_cold ? 8 * n : 0) && n > 0;
        SortTemp st;
        int src = st.alloc(n, lend ? scan_out : nullptr);
        if (src) return src;
        DevTemp list_mem;
        uint64_t *lent_list = (lend && lists_cold) ? reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(scan_out) + key_bytes) : nullptr;
        uint64_t *d_entries = lists_cold ? nullptr : reinterpret_cast<uint64_t *>(base + ix->hdr.off_entries);
        uint64_t *c_entries = lists_kept_cold ? reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(ix->h_cold) + ix->hdr.off_entries) : nullptr;
        if (lists_cold) {
            if (!lent_list && hipMalloc(&list_mem.p, std::max<uint64_t>(8 * n, 8)) != hipSuccess) { (void)hipGetLastError(); list_mem.p = nullptr; return kSortNoRoom; }
        } else if (dbi) { // isslCreateIndex.cpp:218-234 on the device
            int brc = launch_build_entries(d_sites, d_site_occ, n, 0, static_cast<uint32_t>(g.n_slices),
                                           static_cast<uint32_t>(g.slice_width), d_entries);
            if (brc) return brc;
            upload_note(ix, "slice lists built on the device", t0);
        }
        // Lists from the host: one slice at a time, so that the kernels that order slice s run while slice s + 1 is on
        // its way (the copy returns when the slice has landed; the kernels are asynchronous on the null stream, the
        // copies run on a stream of their own).
        const bool stream_lists = !lists_cold && !dbi;
        t0 = now_ms();
        for (uint64_t sl = 0; sl < g.n_slices; ++sl) {
            uint64_t *const t_list_mem = lent_list ? lent_list : static_cast<uint64_t *>(list_mem.p);
            const uint64_t *d_list = lists_cold ? t_list_mem : d_entries + sl * n;
            if (stream_lists) {
                if (int crc = begin_list(sl + 1)) return crc;
                if (int crc = from_file.wait(t_list[sl])) return crc;
            }
            if (lists_cold) {
                uint64_t *t_list = t_list_mem;
                if (dbi) {
                    int brc = launch_build_entries(d_sites, d_site_occ, n, static_cast<uint32_t>(sl), static_cast<uint32_t>(sl + 1),
                                                   static_cast<uint32_t>(g.slice_width), t_list);
                    if (brc) return brc;
                    if (c_entries) HIP_TRY(hipMemcpy(c_entries + sl * n, t_list, 8 * n, hipMemcpyDeviceToHost));
                } else if (c_entries) {
                    std::memcpy(c_entries + sl * n, h.entries + sl * n, 8 * n);
                    HIP_TRY(hipMemcpy(t_list, c_entries + sl * n, 8 * n, hipMemcpyHostToDevice));
                } else {
                    if (int crc = from_file.copy(h, t_list, h.entries + sl * n, 8 * n)) return crc;
                }
            }
            src = launch_sort_slice(st, d_sites, d_list, reinterpret_cast<const uint64_t *>(base + ix->hdr.off_bucket_start),
                                    reinterpret_cast<const uint32_t *>(base + ix->hdr.off_tile_first), n,
                                    static_cast<uint32_t>(g.n_slices), static_cast<uint32_t>(nb), static_cast<uint32_t>(g.slice_width),
                                    static_cast<uint32_t>(sl), reinterpret_cast<uint32_t *>(base + ix->hdr.off_sub_start),
                                    ix->hdr.off_srec ? reinterpret_cast<StreamRec *>(base + ix->hdr.off_srec) : nullptr,
                                    ix->hdr.off_sid ? reinterpret_cast<uint32_t *>(base + ix->hdr.off_sid) : nullptr, d_site_occ, flag);
            if (src) return src;
            if (lists_cold) HIP_TRY(hipDeviceSynchronize()); // the temporary list is overwritten by the next slice
        }
        src = finish_sort(flag);
        if (src) return src;
        st.release();
        upload_note(ix, stream_lists ? "entries, slice by slice, beside the sorted layout (successor-byte order of every bucket + stream maps)"
                                     : "sorted layout (successor-byte order of every bucket + stream maps)", t0);
        t0 = now_ms();
        launch_pack_scan_stream(ix->view, scan_out, nullptr, nullptr, flag, nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        launch_tag_sites(d_sites, d_site_occ, n); // (last: from here on `sites` carries a 24-bit copy of the counts)
        HIP_TRY(hipGetLastError());
    } else if (!ix->hdr.cold_on_host) {
        // (file-mapped host arrays go through FileUploader's pinned ring, everything else through plain copies)
        if (dbi) HIP_TRY(hipMemcpy(base + ix->hdr.off_sites, dbi->sigs, 8 * g.n_sites, dbi_kind));
        else if (int crc = from_file.wait(t_sites)) return crc;
        upload_note(ix, "sites", t0);
        t0 = now_ms();
        if (dbi) { // isslCreateIndex.cpp:218-234 on the device
            int brc = launch_build_entries(reinterpret_cast<const uint64_t *>(base + ix->hdr.off_sites), d_occ, g.n_sites,
                                           0, static_cast<uint32_t>(g.n_slices), static_cast<uint32_t>(g.slice_width),
                                           reinterpret_cast<uint64_t *>(base + ix->hdr.off_entries));
            if (brc) return brc;
            upload_note(ix, "slice lists built on the device", t0);
            t0 = now_ms();
            launch_pack_scan_stream(ix->view, scan_out,
                                    ix->hdr.off_esig ? reinterpret_cast<uint64_t *>(base + ix->hdr.off_esig) : nullptr, nullptr, flag,
                                    seen, nullptr);
            HIP_TRY(hipGetLastError());
        } else {
            // scan stream: built on the device from sites + entries, one slice at a time: the kernel that packs slice s runs
            // while the list of slice s + 1 is on its way (a slice's buckets own a contiguous run of tiles)
            for (uint64_t sl = 0; sl < g.n_slices; ++sl) {
                if (int crc = begin_list(sl + 1)) return crc;
                if (int crc = from_file.wait(t_list[sl])) return crc;
                launch_pack_scan_range(ix->view, scan_out, ix->hdr.off_esig ? reinterpret_cast<uint64_t *>(base + ix->hdr.off_esig) : nullptr,
                                       nullptr, flag, seen, tfirst[sl << g.slice_width], tfirst[(sl + 1) << g.slice_width], nullptr);
                HIP_TRY(hipGetLastError());
            }
            upload_note(ix, "entries, slice by slice, beside the packing of the scan stream", t0);
            t0 = now_ms();
        }
    } else {
        // List-order layout with sites and lists in pinned host memory: the scan stream is packed one slice at a time from temporary device
        // copies of the signatures (8 B/site) and of that slice's list (8 B/site); random reads of the site table
        // across PCIe would take minutes.  With a device-side build the lists are made here and copied out.
        uint8_t *cold = static_cast<uint8_t *>(ix->h_cold);
        uint64_t *c_sites = reinterpret_cast<uint64_t *>(cold + ix->hdr.off_sites);
        uint64_t *c_entries = reinterpret_cast<uint64_t *>(cold + ix->hdr.off_entries);
        const uint64_t n = g.n_sites;
        DevTemp sites_mem, list_mem;
        HIP_TRY(hipMalloc(&sites_mem.p, std::max<uint64_t>(8 * n, 8)));
        HIP_TRY(hipMalloc(&list_mem.p, std::max<uint64_t>(8 * n, 8)));
        uint64_t *t_sites = static_cast<uint64_t *>(sites_mem.p), *t_list = static_cast<uint64_t *>(list_mem.p);
        if (dbi && dbi->on_device) HIP_TRY(hipMemcpy(c_sites, dbi->sigs, 8 * n, hipMemcpyDeviceToHost));
        else std::memcpy(c_sites, dbi ? dbi->sigs : h.sites, 8 * n);
        HIP_TRY(hipMemcpy(t_sites, c_sites, 8 * n, hipMemcpyHostToDevice));
        upload_note(ix, "sites (pinned host copy + temporary device copy)", t0);
        t0 = now_ms();
        for (uint64_t sl = 0; sl < g.n_slices; ++sl) {
            if (dbi) {
                int brc = launch_build_entries(t_sites, d_occ, n, static_cast<uint32_t>(sl), static_cast<uint32_t>(sl + 1),
                                               static_cast<uint32_t>(g.slice_width), t_list);
                if (brc) return brc;
                HIP_TRY(hipMemcpy(c_entries + sl * n, t_list, 8 * n, hipMemcpyDeviceToHost));
            } else {
                std::memcpy(c_entries + sl * n, h.entries + sl * n, 8 * n);
                HIP_TRY(hipMemcpy(t_list, c_entries + sl * n, 8 * n, hipMemcpyHostToDevice));
            }
            ImageView pv = ix->view;
            pv.sites = t_sites;
            pv.entries = t_list - sl * n; // bucket_start of the slice's first bucket is sl * n: every site sits in one bucket per slice
            launch_pack_scan_range(pv, scan_out, nullptr, reinterpret_cast<uint8_t *>(base + ix->hdr.off_occ8), flag, seen,
                                   tfirst[sl << g.slice_width], tfirst[(sl + 1) << g.slice_width], nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
        }
        upload_note(ix, "slice lists into pinned host memory", t0);
        t0 = now_ms();
    }
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, flag, 4, hipMemcpyDeviceToHost));
    upload_note(ix, "scan stream", t0);
    if (ix->tuning.upload_timing) std::fprintf(stderr, "[issl upload] (pinning the ring: %.1f ms, summed over the readers)\n", from_file.pin_ms());
    const double t_ring = now_ms();
    from_file.release();
    upload_note(ix, "pinned ring given back", t_ring);
    if (err & 1u) {
        set_error("Error reading index: a slice entry refers to an off-target id beyond the site table");
        return ISSL_E_FORMAT;
    }
    if (err) {
        set_error("Error reading index: a slice list holds an off-target in a bucket its signature does not select, or twice");
        return ISSL_E_FORMAT;
    }
    return ISSL_OK;
}

// The optional in-list signatures cost 8 B per list entry (40 B per site next to the 68 B of the rest): worth it while
// the image stays a modest part of the HBM (inline_sigs knob / ISSL_INLINE_SIGS=0/1 overrides).
static bool want_inline_sigs(const Tuning &tn, const Geometry &g)
{
    if (tn.inline_sigs >= 0) return tn.inline_sigs == 1;
    return g.n_sites <= 600000000ull;
}

// The layouts an upload tries, in turn, until one fits the free HBM.  Bytes per site next to the 20 B of the scan
// stream: sorted 132 (16-byte stream records, site table, counts, slice lists), compact sorted 72 or -- slice lists in
// pinned host memory -- 32; list order 88 / 48 (with / without the in-list signatures) or, all cold sections in host
// memory, 5.  The sorted ones let the scan skip 243 of every 256 successor-byte groups; they need lists that ascend by
// site id (list_order_only: this index's do not).  Explicit options are honoured or the upload fails.
static std::vector<LayoutSpec> layout_choices(const Tuning &tn, const Geometry &g, bool list_order_only)
{
    std::vector<LayoutSpec> c;
    auto spec = [](bool esig, uint32_t cold, uint32_t sorted, bool no_lists = false) { LayoutSpec s; s.inline_sigs = esig; s.cold = cold; s.sorted = sorted; s.no_lists = no_lists; return s; };
    // Narrow slices (4 / 2 bits; round 4): the sorted layouts order a bucket by the byte of the next two / four slices (succ_byte),
    // so everything sorted applies; only the list-order layout with ALL cold sections in host memory does not -- it rebuilds a
    // candidate's signature from the stream's 16 positions + the bucket's byte, and a narrow slice leaves 18 / 19 outside.
    const bool narrow = g.slice_width != 8;
    const bool may_sort = !list_order_only && tn.sorted_layout != 0 && tn.inline_sigs != 1;
    const bool must_sort = tn.sorted_layout == 1 || tn.compact == 1 || tn.keep_lists == 0; // (only a sorted image can do without its lists)
    if (may_sort || must_sort) {
        if (tn.host_cold == 1) {
            if ((tn.compact == 1 || tn.sorted_layout == 1) && tn.keep_lists != 0) c.push_back(spec(false, 1, 2));
        } else {
            if (tn.compact != 1 && tn.keep_lists != 0) c.push_back(spec(false, 0, 1));
            if (tn.compact != 0) {
                if (tn.keep_lists != 0) c.push_back(spec(false, 0, 2));
                // the smallest image: compact and without its slice lists -- 52 B/site, self-contained (nothing in host
                // memory, so it can still be broadcast and attached elsewhere); the variant with the lists in pinned
                // host memory (40 B/site there) is made on request only (host_cold=1)
                if (tn.keep_lists != 1) c.push_back(spec(false, 0, 2, true));
            }
        }
    }
    if (!must_sort) {
        if (tn.host_cold == 1) {
            if (!narrow) c.push_back(spec(false, 3, 0));
        } else {
            if (want_inline_sigs(tn, g)) c.push_back(spec(true, 0, 0));
            if (tn.inline_sigs != 1) c.push_back(spec(false, 0, 0));
            if (tn.host_cold == -1 && tn.inline_sigs != 1 && !narrow) c.push_back(spec(false, 3, 0));
        }
    }
    return c;
}

static uint64_t count_tiles(const HostIndex &h)
{
    uint64_t t = 0;
    for (uint64_t b = 0; b < h.geo.n_buckets(); ++b) t += (h.sizes[b] + kTileCands - 1) / kTileCands;
    return t;
}

void release_device(issl_index *ix)
{
    if (ix->device >= 0) (void)hipSetDevice(ix->device);
    release_lanes(ix);
    if (ix->d_image && ix->owns_image) (void)hipFree(ix->d_image);
    ix->d_image = nullptr;
    ix->owns_image = false;
    if (ix->h_cold && ix->owns_cold) (void)hipHostFree(ix->h_cold);
    ix->h_cold = nullptr;
    ix->d_cold = nullptr;
    ix->owns_cold = false;
}

int new_index_from_host(std::unique_ptr<HostIndex> h, issl_index **out)
{
    std::unique_ptr<issl_index> ix(new issl_index());
    ix->geo = h->geo;
    ix->bucket_sizes.assign(h->sizes, h->sizes + h->geo.n_buckets());
    ix->host = std::move(h);
    *out = ix.release();
    return ISSL_OK;
}

static int upload(issl_index *idx, int device, void *buf, size_t bytes, const DeviceBuildInput *dbi)
{
    if (!idx->host) { set_error("index has no host arrays to upload"); return ISSL_E_STATE; }
    if (!dbi && !idx->host->has_arrays()) {
        // built on the device: its arrays exist only in that image
        if (idx->d_image && idx->device == device && !buf) return ISSL_OK;
        set_error("index was built on the device and has no host arrays: replicate its image with issl_index_image + "
                  "issl_index_attach_image");
        return ISSL_E_STATE;
    }
    int rc = supported_geometry(idx->geo);
    if (rc) return rc;
    double t0 = now_ms();
    rc = select_device(device, "the ISSL scorer");
    if (rc) return rc;
    release_device(idx);
    (void)hipFree(nullptr); // creates the context
    upload_note(idx, "device runtime start", t0);
    t0 = now_ms();
    std::vector<uint64_t> m;
    std::vector<double> v;
    idx->host->unique_scores(m, v);
    const Tuning &tn = idx->tuning;
    const std::vector<LayoutSpec> choices = layout_choices(tn, idx->geo, idx->list_order_only);
    idx->device = device;
    const uint64_t n_tiles = count_tiles(*idx->host);
    const bool dense = masks_are_dense(m);
    std::string why = "the layout options of this index contradict each other";
    for (const LayoutSpec &c : choices) {
        layout_image(idx->hdr, idx->geo, m.size(), n_tiles, dense, c);
        // temporary device memory: while a list-order host-cold image is packed, signatures + one slice list; for the
        // sorted layouts two key arrays of 8 B per site (one slice at a time) and, lists in host memory, one slice list
        const uint64_t ns = idx->geo.n_sites;
        const uint64_t temp = c.sorted ? 8 * ns + (64ull << 20) // (keys and slice list live in the image's scan section while it is built)
                              : (c.cold ? 16 * ns : 0) + ns * idx->geo.n_slices / 8 + 8; // (list order: + the `seen` bitmap)
        if (buf) {
            if (bytes < idx->hdr.total_bytes || (reinterpret_cast<uintptr_t>(buf) & 255u)) {
                why = "device buffer too small or not 256-byte aligned";
                continue;
            }
            idx->d_image = buf;
            idx->owns_image = false;
        } else {
            // leave room for the scoring workspace: the larger of 2 GiB and 3 % of the device
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b)); // (nothing allocated yet on this turn of the loop)
            const uint64_t reserve = std::max<uint64_t>(uint64_t(2) << 30, total_b / 32);
            if (idx->hdr.total_bytes + temp + reserve > free_b) {
                why = "the image (" + std::to_string(idx->hdr.total_bytes >> 20) + " MiB) does not fit the free device memory (" +
                      std::to_string(free_b >> 20) + " MiB)";
                continue;
            }
            if (hipMalloc(&idx->d_image, idx->hdr.total_bytes) != hipSuccess) {
                (void)hipGetLastError();
                idx->d_image = nullptr;
                why = "hipMalloc of the image failed";
                continue;
            }
            idx->owns_image = true;
        }
        if (c.cold) {
            // portable + mapped: every device of the node can read the one host copy (issl_node)
            if (hipHostMalloc(&idx->h_cold, std::max<uint64_t>(idx->hdr.cold_bytes, 256), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
                (void)hipGetLastError();
                idx->h_cold = nullptr;
                if (idx->owns_image) (void)hipFree(idx->d_image);
                idx->d_image = nullptr;
                idx->owns_image = false;
                why = "cannot pin " + std::to_string(idx->hdr.cold_bytes >> 20) + " MiB of host memory for the cold sections";
                continue;
            }
            idx->owns_cold = true;
            if (hipHostGetDevicePointer(&idx->d_cold, idx->h_cold, 0) != hipSuccess) {
                (void)hipGetLastError();
                release_device(idx);
                set_error("HIP error: the pinned host buffer of the cold sections has no device address");
                return ISSL_E_DEVICE;
            }
        }
        upload_note(idx, c.cold ? "layout + allocation (cold sections in pinned host memory)" : "layout + allocation", t0);
        // expect_guides: the caller will score a batch of about this many guides right after the upload (the one-shot scorer
        // knows its page).  The scoring workspace -- streams, events, the buffers of a small batch -- is set up on a thread of
        // its own while the file's sections are on their way (the upload is bound by the PCIe link): 20 ms less in front of a
        // one-shot process's first kernel.  Only where image and temporaries leave the device half empty; a failure here is
        // the first scoring call's to report.
        ThreadGroup prep; // (one thread at most)
        if (tn.expect_guides && !buf) {
            size_t free_now = 0, total_now = 0;
            if (hipMemGetInfo(&free_now, &total_now) == hipSuccess && free_now > temp + (size_t(24) << 30) + total_now / 2)
                prep.add([idx] { // (reads the header the layout has just made; the view is finish_upload's)
                    (void)hipSetDevice(idx->device);
                    // (for at most 32 k guides: the streams, the events, the small buffers -- the first call's fixed 20 ms.  The
                    // gigabytes a page of a million guides needs are allocated by the scoring call itself: beside the upload they
                    // held its copies up for as long as they took, 27 ms moved from one stage to the other)
                    const size_t n = std::min<size_t>(idx->tuning.expect_guides, size_t(1) << 15);
                    if (ensure_workspace(idx, n, idx->lane) != ISSL_OK) (void)hipGetLastError();
                });
            else
                (void)hipGetLastError();
        }
        try {
            rc = finish_upload(idx, dbi);
        } catch (...) { // (no half-made image stays on the handle)
            prep.join();
            release_device(idx);
            throw;
        }
        prep.join();
        if (rc == ISSL_OK) return ISSL_OK;
        release_device(idx);
        if (rc == kSortNoRoom) { // the temporaries of the sort did not fit after all: the next, smaller layout
            why = "no device memory for the temporaries of the sorted layout";
            t0 = now_ms();
            continue;
        }
        if (rc == kSortNeedsListOrder) {
            // (keep_lists=0 forces a sorted layout like the other two -- only a sorted image can do without its lists --, and an
            // index that has been here before is not sent round again: the second turn would end where the first did)
            if (tn.sorted_layout == 1 || tn.compact == 1 || tn.keep_lists == 0 || idx->list_order_only) {
                set_error("this index cannot take the sorted layout that was asked for: a list is not ascending by site id, "
                          "holds a site in a bucket its signature does not select, or carries different counts for one site");
                return ISSL_E_UNSUPPORTED;
            }
            idx->list_order_only = true; // once more, with the stream in list order
            return upload(idx, device, buf, bytes, dbi);
        }
        return rc;
    }
    set_error("cannot place the index image: " + why);
    return buf ? ISSL_E_ARG : ISSL_E_DEVICE;
}

int upload_common(issl_index *idx, int device, void *buf, size_t bytes) { return upload(idx, device, buf, bytes, nullptr); }

int build_on_device(std::unique_ptr<HostIndex> h, const uint64_t *sigs, const uint32_t *occ, bool on_device, int device,
                    const char *options, issl_index **out)
{
    issl_index *ix = nullptr;
    int rc = new_index_from_host(std::move(h), &ix);
    if (rc) return rc;
    std::unique_ptr<issl_index, void (*)(issl_index *)> owned(ix, [](issl_index *p) { release_device(p); delete p; });
    rc = ix->tuning.set_list(options);
    if (rc) return rc;
    const DeviceBuildInput dbi{sigs, occ, on_device};
    rc = upload(ix, device, nullptr, 0, &dbi);
    if (rc) return rc;
    *out = owned.release();
    return ISSL_OK;
}

int planned_image_bytes(const issl_index *idx, size_t *out)
{
    int rc = supported_geometry(idx->geo);
    if (rc) return rc;
    std::vector<uint64_t> m;
    std::vector<double> v;
    idx->host->unique_scores(m, v);
    ImageHeader h;
    // the layout an upload tries first (issl_index_upload falls back to smaller ones when the HBM is short)
    const std::vector<LayoutSpec> choices = layout_choices(idx->tuning, idx->geo, idx->list_order_only);
    if (choices.empty()) { set_error("the layout options of this index contradict each other"); return ISSL_E_ARG; }
    layout_image(h, idx->geo, m.size(), count_tiles(*idx->host), masks_are_dense(m), choices.front());
    *out = h.total_bytes;
    return ISSL_OK;
}

int attach_common(int device, void *dev_buf, size_t bytes, void *cold_host, size_t cold_bytes, issl_index **out)
{
    if (!dev_buf || !out) return issl::fail(ISSL_E_ARG, "null argument");
    int rc = select_device(device, "the ISSL scorer");
    if (rc) return rc;
    if (bytes < kHeaderBytes || (reinterpret_cast<uintptr_t>(dev_buf) & 255u)) {
        set_error("device image too small or not 256-byte aligned");
        return ISSL_E_ARG;
    }
    ImageHeader h;
    HIP_TRY(hipMemcpy(&h, dev_buf, sizeof h, hipMemcpyDeviceToHost));
    if (h.magic != kImageMagic || h.version != kImageVersion || h.tile_cands != kTileCands ||
        h.total_bytes > bytes) {
        set_error("device buffer does not hold an ISSL image of this library version");
        return ISSL_E_FORMAT;
    }
    void *d_cold = nullptr;
    if (h.cold_on_host) {
        if (!cold_host || cold_bytes < h.cold_bytes) {
            set_error("this image keeps its cold sections (sites, slice lists) in pinned host memory: attach it with "
                      "issl_index_attach_image_cold and the buffer of issl_index_cold");
            return ISSL_E_STATE;
        }
        HIP_TRY(hipHostGetDevicePointer(&d_cold, cold_host, 0));
    }
    std::unique_ptr<issl_index> ix(new issl_index());
    ix->geo.n_sites = h.n_sites;
    ix->geo.seq_len = h.seq_len;
    ix->geo.n_lines = h.n_lines;
    ix->geo.slice_width = h.slice_width;
    ix->geo.n_slices = h.n_slices;
    ix->geo.n_scores = h.n_scores_file;
    ix->hdr = h;
    ix->device = device;
    ix->d_image = dev_buf;
    ix->owns_image = false;
    ix->h_cold = h.cold_on_host ? cold_host : nullptr;
    ix->d_cold = d_cold;
    ix->owns_cold = false;
    ix->view = make_view(h, dev_buf, d_cold);
    std::vector<uint64_t> bstart(h.n_buckets + 1);
    hipError_t e = hipMemcpy(bstart.data(), static_cast<uint8_t *>(dev_buf) + h.off_bucket_start,
                             8 * (h.n_buckets + 1), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("HIP error: ") + hipGetErrorString(e));
        return ISSL_E_DEVICE;
    }
    ix->bucket_sizes.resize(h.n_buckets);
    for (uint64_t b = 0; b < h.n_buckets; ++b) ix->bucket_sizes[b] = bstart[b + 1] - bstart[b];
    *out = ix.release();
    return ISSL_OK;
}

} // namespace issl
