// The index handle behind the C ABI (include/issl_hip.h) and what the units of the host library share:
// issl_upload.cpp (HBM image), issl_pipeline.cpp (scoring batches), issl_capi.cpp (the extern "C" entry points).
#pragma once
#include <hip/hip_runtime_api.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "issl_device.hpp"
#include "issl_hiputil.hpp"

namespace issl {

constexpr uint32_t kRing = 64;
constexpr size_t kMaxBatch = size_t(1) << 24; // guides per pipeline launch
constexpr size_t kSlotBytesMax = size_t(8) << 30; // hit slots of a workspace: up to 8 GiB (512 k guides per batch)

// One complete workspace + the internal streams its batches run on.  The synchronous entry points use one lane; with the
// lanes option at 2 or 3 asynchronous batches alternate between two of them (not the default: bench.py --full measures
// both beside lanes=1).
struct Lane {
    Workspace ws;
    hipEvent_t ev[6] = {};      // stage boundaries of the last batch
    hipEvent_t done = nullptr;  // end of the last batch
    hipStream_t stream = nullptr; // internal stream of asynchronous batches
    hipStream_t tail_stream = nullptr; // lanes = 2: the batch's verify / group / replay run here (high priority), beside the
                                // scan of the next batch on the other lane's stream
    bool ready = false;         // events and stream created
    uint32_t last_n = 0;
    uint32_t pending = 0;       // batches enqueued since the last finish
    bool staged = true;         // the last batch recorded its stage events
    bool done_recorded = false; // `done` stands behind the lane's last batch
    hipStream_t last_tail = nullptr; // the stream that batch's last kernels went to
    int last_max_dist = 0;
    uint32_t last_prune = 0;
    uint32_t scan_verified = 0; // Counters::scan_verified of the lane's last finished batch
    uint32_t scan_lds_buffers = 0, scan_raw_top = 0, raw_chunks = 0; // ... its lds_chunks, raw_top and raw_chunks (ws_scan_lds_buffers, ws_scan_raw_top, ws_raw_chunks)
    bool lean = false;          // the lane's finished batches had no guide beyond its hit slots: the next ones are enqueued
                                // without the grouping pass and the many-hit replays (Workspace::lean_tail)
};

} // namespace issl

struct issl_index {
    uint64_t worst_per_guide = 0;    // sum over the slices of their longest bucket: what one guide can be compared with at most (issl_score)
    std::unique_ptr<issl::HostIndex> host; // absent for attached images
    issl::Geometry geo;
    std::vector<uint64_t> bucket_sizes;
    issl::Tuning tuning = issl::Tuning::from_env(); // the environment is read here, once per handle
    // device state
    int device = -1;
    void *d_image = nullptr;
    bool owns_image = false;
    void *h_cold = nullptr;   // pinned host buffer of the cold sections (hdr.cold_on_host), else null
    void *d_cold = nullptr;   // the same buffer as the device addresses it
    bool owns_cold = false;
    issl::ImageHeader hdr{};
    issl::ImageView view{};
    issl::Lane lane;          // workspace + stream of the synchronous entry points and of every other asynchronous batch
    issl::Lane lane2;         // ... and of the batches in between (lanes option = 2)
    uint32_t n_async = 0;     // asynchronous batches enqueued so far: picks the lane
    issl::Lane *last_lane = nullptr; // lane of the most recent batch (whose counters issl_last_stats reports)
    hipEvent_t ring[2 * issl::kRing] = {}; // scan begin/end of the batches enqueued since the last finish (of those that recorded them: n_ring)
    uint32_t n_ring = 0;
    bool have_events = false;
    issl_stats stats{};
    uint32_t n_pending = 0;  // batches enqueued and not yet finished
    hipEvent_t prev_scan_end = nullptr; // lanes = 2: end of the previous batch's scan (scans run one after the other)
    hipEvent_t prev_batch_end = nullptr; // lanes = 3: end of the previous batch (its scan starts when that batch is through)
    bool list_order_only = false; // the lists of this index cannot be re-ordered (kSortNeedsListOrder)
    // issl_score: the largest piece that went through at once (no grow-and-rerun round) with record buffers of at least
    // proven_chunks chunks at a max_dist of at least proven_dist: pieces within that skip the per-guide estimate (0.9 ms per 500 k guides)
    size_t proven_guides = 0, proven_chunks = 0;
    int proven_dist = -1;
    // what the pruned plan of the last finished batch planned per guide, and for which prune mode (tail_worth_arming)
    double plan_cands_per_guide = 0.0;
    uint32_t plan_cands_prune = 0;
};

namespace issl {

// ---- issl_upload.cpp: the HBM image -----------------------------------------------------------
int new_index_from_host(std::unique_ptr<HostIndex> h, issl_index **out);
// A handle around a new host index that init(HostIndex &) fills (it returns ISSL_OK or an error code).
template <class Init> int new_index(Init &&init, issl_index **out)
{
    std::unique_ptr<HostIndex> h(new HostIndex());
    if (int rc = init(*h)) return rc;
    return new_index_from_host(std::move(h), out);
}
// issl_index_build_on_device_opt / _from_device_sites: upload of an index whose slice lists are built on the device.
int build_on_device(std::unique_ptr<HostIndex> h, const uint64_t *sigs, const uint32_t *occ, bool on_device, int device,
                    const char *options, issl_index **out);
// issl_index_build_from_device_sites after its argument checks (geometry: seq_len 1..32, slices of 2..8 bits)
int build_from_device_sites(const uint64_t *d_sigs, const uint32_t *d_occ, size_t n_sites, size_t n_lines, size_t seq_len,
                            size_t slice_width, int device, const char *options, issl_index **out);
int upload_common(issl_index *idx, int device, void *buf, size_t bytes);
int attach_common(int device, void *dev_buf, size_t bytes, void *cold_host, size_t cold_bytes, issl_index **out);
int planned_image_bytes(const issl_index *idx, size_t *out); // the image the next upload tries first
void release_device(issl_index *ix);

// ---- issl_pipeline.cpp: scoring batches ------------------------------------------------------
int supported_geometry(const Geometry &g);
void release_lanes(issl_index *ix);
inline uint32_t scan_waves(const Tuning &tn) { return tn.scan_blocks * 16u; }
int ensure_workspace(issl_index *ix, size_t n, Lane &lane, uint32_t fine_ways = kFineWays);
int ensure_raw_capacity(Workspace &w, size_t chunks);
int finish_batches(issl_index *ix, hipStream_t stream);
int score_core(issl_index *ix, const uint64_t *d_guides, size_t n, int max_dist, double threshold, int method,
               double *d_mit, double *d_cfd, hipStream_t stream, bool dump, issl_profile *d_profile = nullptr);
int score_async(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, double threshold, int method,
                double *d_mit, double *d_cfd, hipStream_t stream);
int wait_batches(issl_index *idx, hipStream_t stream);
int score_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
               double *mit, double *cfd);
int dump_hits(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
              issl_hit *hits, size_t cap, size_t *n_hits);
// Off-target report (issl_offtarget_profile*, issl_offtargets*): host batches of any size in issl_score's pieces.
int profile_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, issl_profile *out);
int profile_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, issl_profile *d_out, hipStream_t stream);
int offtargets_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, uint64_t *offsets, issl_offtarget *recs,
                    size_t cap, size_t *n_total);
int offtargets_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, uint64_t *d_offsets,
                      issl_offtarget *d_recs, size_t cap, size_t *n_total, hipStream_t stream);

// A device buffer of the call (the piece's profiles, the piece's records): grown, never shrunk, freed at the end.
struct CallBuffer : DevBuf {
    size_t bytes = 0;
    int reserve(size_t want)
    {
        if (want <= bytes) return ISSL_OK;
        release();
        bytes = 0;
        HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return ISSL_OK;
    }
};

// The off-target records of one batch of guides, left in device memory for a unit that reads them there
// (issl_landing.hip): records d_recs[0 .. n_recs) in issl_offtargets' order, their `guide` fields counted from
// guide_base; guide i of the batch owns d_recs[d_rec_off[i] .. d_rec_off[i + 1]).  d_rec_off is the workspace's and
// holds until the handle's next batch.
struct RecordBatch {
    const uint64_t *d_guides = nullptr;
    size_t n_guides = 0, guide_base = 0;
    const issl_offtarget *d_recs = nullptr;
    uint32_t n_recs = 0;
    const uint32_t *d_rec_off = nullptr;
};
// One batch of guides in device memory, enqueued on `stream`; the records land in `buf`.
int records_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, CallBuffer &buf, RecordBatch &out, hipStream_t stream);
// Guides in host memory, cut as issl_offtargets cuts them: use(batch) once per piece, on the default stream.
int records_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, CallBuffer &buf,
                 const std::function<int(const RecordBatch &)> &use);

} // namespace issl
