// The scoring pipeline: workspaces, the launch of a batch, its completion, and the host-pointer entry points' pieces.
// Host code; the kernels are in the stage files issl_bin.hip ... issl_report.hip (file map: issl_kernels.hip).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "issl_index.hpp"

namespace issl {

// 20 bp sequences cut into slices of 8, 4 or 2 bits (5, 10 or 20 slices): what isslCreateIndex can write correctly (it
// keeps slice values in a uint8_t, isslCreateIndex.cpp:228, and 40 bits only divide into whole positions for these
// widths).  Width 8 -- the README's recommendation, Crackling's default -- gets the sorted layouts and the pruned scan;
// the narrower ones the list-order layouts in HBM and the scan of whole buckets (the reference's own loop, :330-344).
int supported_geometry(const Geometry &g)
{
    if (g.seq_len == 20 && (g.slice_width == 8 || g.slice_width == 4 || g.slice_width == 2) && g.n_slices * g.slice_width == 40) return ISSL_OK;
    set_error("unsupported index geometry: the gfx950 scan kernels implement 20 bp sequences in slices of 8, 4 or 2 bits "
              "(got seq_len=" + std::to_string(g.seq_len) + " slice_width=" +
              std::to_string(g.slice_width) + " slices=" + std::to_string(g.n_slices) + ")");
    return ISSL_E_UNSUPPORTED;
}

static void free_workspace(Workspace &w)
{
    void *ptrs[] = {w.ng, w.gfill, w.gstart, w.gword, w.gidx, w.gbucket, w.gsig, w.items, w.plan, w.range_start, w.counters, w.scan_count, w.scan_span, w.sticky, w.stamps, w.gcur_big, w.gcur_big2, w.terms, w.sorted, w.gcount,
                    w.goff, w.blocksum, w.d_guides, w.d_mit, w.d_cfd, w.d_kept, w.d_hitrec, w.pay, w.rank, w.fword,
                    w.fitems, w.fcount, w.fcount0, w.fsum, w.slots};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (w.raw) (void)hipFree(w.raw);
    if (w.raw_used) (void)hipFree(w.raw_used);
    if (w.h_stage) (void)hipHostFree(w.h_stage);
    w = Workspace{};
}

// Streams, events and workspaces of both lanes, and what the handle remembers of its batches.
void release_lanes(issl_index *ix)
{
    for (Lane *lp : {&ix->lane, &ix->lane2}) {
        Lane &lane = *lp;
        if (lane.ready) {
            (void)hipStreamSynchronize(lane.stream);
            (void)hipStreamSynchronize(lane.tail_stream);
            for (auto &e : lane.ev) (void)hipEventDestroy(e);
            (void)hipEventDestroy(lane.done);
            (void)hipStreamDestroy(lane.stream);
            (void)hipStreamDestroy(lane.tail_stream);
            lane.ready = false;
        }
        free_workspace(lane.ws);
        lane.lean = false;
        lane.last_n = 0;
        lane.pending = 0;
    }
    ix->last_lane = nullptr;
    if (ix->have_events) {
        for (auto &e : ix->ring) (void)hipEventDestroy(e);
        ix->have_events = false;
    }
    ix->n_pending = 0;
    ix->n_ring = 0;
    ix->proven_guides = 0;
    ix->proven_chunks = 0;
    ix->proven_dist = -1;
    ix->plan_cands_per_guide = 0.0;
    ix->plan_cands_prune = 0;
    ix->prev_scan_end = nullptr;
    ix->prev_batch_end = nullptr;
}

// Pinned host memory for the host-pointer entry point: a copy from pageable memory is staged by the runtime piece by piece
// (three of them cost 0.5 ms per 100 k guides); from here it is one DMA each.  No pinned memory: the plain copies do.
static bool ensure_stage(Workspace &w, size_t bytes)
{
    if (w.h_stage_bytes >= bytes) return true;
    if (w.h_stage) (void)hipHostFree(w.h_stage);
    w.h_stage = nullptr;
    w.h_stage_bytes = 0;
    const size_t want = bytes + bytes / 4;
    if (hipHostMalloc(&w.h_stage, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); w.h_stage = nullptr; return false; }
    w.h_stage_bytes = want;
    return true;
}

template <typename T> static int dev_alloc(T *&p, size_t count)
{
    if (p) {
        (void)hipFree(p);
        p = nullptr;
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T)));
    return ISSL_OK;
}

static int ensure_hit_capacity(Workspace &w, size_t want)
{
    if (want <= w.cap_hits) return ISSL_OK;
    int rc;
    if ((rc = dev_alloc(w.sorted, want))) return rc;
    if ((rc = dev_alloc(w.terms, 2 * want))) return rc;
    if ((rc = dev_alloc(w.pay, 2 * want))) return rc;
    if ((rc = dev_alloc(w.rank, want))) return rc;
    w.cap_hits = want;
    return ISSL_OK;
}

int ensure_raw_capacity(Workspace &w, size_t chunks)
{
    if (chunks <= w.cap_chunks) return ISSL_OK;
    int rc = dev_alloc(w.raw, (chunks + 1) * kChunkRecs); // +1: spare chunk that absorbs writes after exhaustion
    if (rc) return rc;
    if ((rc = dev_alloc(w.raw_used, chunks + 1))) return rc;
    w.cap_chunks = chunks;
    return ISSL_OK;
}

int ensure_workspace(issl_index *ix, size_t n, Lane &lane, uint32_t fine_ways)
{
    Workspace &w = lane.ws;
    const Tuning &tn = ix->tuning;
    const size_t nb = ix->hdr.n_buckets;
    int rc;
    if (w.n_buckets != nb) {
        if ((rc = dev_alloc(w.ng, nb))) return rc;
        if ((rc = dev_alloc(w.gfill, nb))) return rc;
        HIP_TRY(hipMemset(w.ng, 0, 4 * nb)); // k_plan leaves both zeroed for the next batch
        HIP_TRY(hipMemset(w.gfill, 0, 4 * nb));
        if ((rc = dev_alloc(w.gstart, nb + 1))) return rc;
        if ((rc = dev_alloc(w.counters, 1))) return rc;
        if ((rc = dev_alloc(w.plan, 1))) return rc;
        if ((rc = dev_alloc(w.range_start, kMaxRanges + 2))) return rc;
        if ((rc = dev_alloc(w.scan_count, kScanMaxBlocks))) return rc;
        if ((rc = dev_alloc(w.scan_span, 2 * kSpanRing))) return rc;
        HIP_TRY(hipMemset(w.scan_span, 0, 16 * kSpanRing));
        HIP_TRY(hipMemset(w.scan_count, 0, 8 * kScanMaxBlocks));
        w.n_buckets = static_cast<uint32_t>(nb);
    }
    bool grew = false;
    // hit_slots = 2 (tests, A/B): wide hit slots from the first batch on, not only once a batch has shown that it needs them
    const bool force_wide = tn.hit_slots == 2 && w.slot_width != kSlotHitsWide &&
                            std::max<size_t>(std::max<size_t>(n, w.cap_guides), 1024) * kSlotHitsWide * sizeof(SlotRec) <= kSlotBytesMax;
    if (force_wide) w.slot_width = kSlotHitsWide;
    if (n > w.cap_guides || (force_wide && w.slots)) {
        grew = true;
        const size_t cap = std::max<size_t>(std::max<size_t>(n, w.cap_guides), 1024);
        const size_t slots = cap * ix->hdr.n_slices + kGuideGroup * nb;
        const size_t items = nb + cap * ix->hdr.n_slices / 8 + 2; // item sizes down to 8 guides (item_guides knob)
        if ((rc = dev_alloc(w.gword, slots))) return rc;
        if ((rc = dev_alloc(w.gidx, slots))) return rc;
        if ((rc = dev_alloc(w.gbucket, slots))) return rc;
        if ((rc = dev_alloc(w.gsig, slots))) return rc;
        if ((rc = dev_alloc(w.items, items + 1))) return rc;
        if ((rc = dev_alloc(w.gcount, cap + 1))) return rc;
        if ((rc = dev_alloc(w.goff, cap + 1))) return rc;
        if ((rc = dev_alloc(w.gcur_big, cap + 1))) return rc;
        if ((rc = dev_alloc(w.gcur_big2, cap + 1))) return rc;
        if ((rc = dev_alloc(w.blocksum, (cap + 1) / 2048 + 2))) return rc;
        if ((rc = dev_alloc(w.d_guides, cap))) return rc;
        if ((rc = dev_alloc(w.d_mit, cap))) return rc;
        if ((rc = dev_alloc(w.d_cfd, cap))) return rc;
        if ((rc = dev_alloc(w.d_kept, cap))) return rc;
        // hit slots (Workspace): kSlotHits x 32 bytes per guide -- 1.6 GB for 100 k guides; batches beyond kSlotBytesMax (or a
        // device short of memory) go without, every hit then passes through the grouping pass
        if (w.slots) { (void)hipFree(w.slots); w.slots = nullptr; }
        w.cap_slot_guides = 0;
        if (cap * w.slot_width * sizeof(SlotRec) > kSlotBytesMax) w.slot_width = kSlotHits; // (a larger batch: back to narrow slots)
        if (cap * w.slot_width * sizeof(SlotRec) <= kSlotBytesMax) {
            if (hipMalloc(reinterpret_cast<void **>(&w.slots), cap * w.slot_width * sizeof(SlotRec)) == hipSuccess) w.cap_slot_guides = cap;
            else { (void)hipGetLastError(); w.slots = nullptr; }
        }
        w.cap_guides = cap;
        w.cap_gslots = slots;
        w.cap_items = items;
    }
    // pruned scan: every guide sits in up to 13 (max_dist 5: 67) successor-byte groups of each of its 5 buckets.  These arrays
    // grow with the batch AND with the number of groups per bucket -- by themselves: the staging buffers above are in use by
    // the caller when a batch's max_dist asks for more groups.
    if (ix->hdr.off_sub_start && (grew || fine_ways > w.fine_ways)) {
        const size_t cap = w.cap_guides;
        const uint32_t ways = std::max(fine_ways, w.fine_ways);
        const size_t m = std::min<size_t>(cap, prune_max_guides(ways > kFineWays ? 3u : 2u, ix->hdr.n_slices));
        const size_t places = m * ix->hdr.n_slices * ways;
        const size_t groups = std::min<size_t>(nb * 256, places);
        const size_t fslots = places + kGuideGroup * groups;
        // one item per tile of a group (and per 512 guides of it): sized from the mean group length (uniform data has
        // sites / 65536 candidates per group -- sites / 4096 with 4-bit slices --, +1.2 tiles for the ends); a batch that needs more scans whole buckets
        // and reports it (sticky[3]), finish_batches() then enlarges the list for the next one
        const size_t tiles_per_group = static_cast<size_t>(ix->hdr.n_sites * ix->hdr.n_slices / (static_cast<uint64_t>(nb) * 256ull * kTileCands)) + 4;
        // (fine_items knob: start with a short list -- tests of the two ways out of a list that is too short)
        const size_t fitems = std::max<size_t>(tn.fine_items ? tn.fine_items : tiles_per_group * (groups + places / 64) + 2, w.cap_fitems);
        if ((rc = dev_alloc(w.fword, fslots + 64))) return rc; // (+ slack: short_unit_masks reads whole groups of 32 slots)
        if ((rc = dev_alloc(w.fitems, fitems + 1))) return rc;
        if ((rc = dev_alloc(w.fcount, nb * 256))) return rc;
        if ((rc = dev_alloc(w.fcount0, nb * 256))) return rc;
        if ((rc = dev_alloc(w.fsum, nb))) return rc;
        w.cap_fslots = fslots;
        w.cap_fitems = fitems;
        w.fine_ways = ways;
    }

    if (w.cap_chunks == 0) {
        // every scan wave may hold one partly filled chunk; beyond that ~1 record per 50k comparisons.
        // raw_chunks knob: start with a small raw buffer (tests of the grow-and-rerun path)
        const size_t want = tn.raw_chunks ? tn.raw_chunks : std::max<size_t>(size_t(scan_waves(tn)) * 6, n);
        if ((rc = ensure_raw_capacity(w, want))) return rc;
    }
    if (!ix->have_events) {
        for (auto &e : ix->ring) HIP_TRY(hipEventCreate(&e));
        ix->have_events = true;
    }
    if (!lane.ready) {
        for (auto &e : lane.ev) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventCreate(&lane.done));
        int prio_low = 0, prio_high = 0; // (numerically lowest = most urgent)
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        HIP_TRY(hipStreamCreateWithPriority(&lane.stream, hipStreamNonBlocking, prio_low));
        HIP_TRY(hipStreamCreateWithPriority(&lane.tail_stream, hipStreamNonBlocking, prio_high));
        lane.ready = true;
    }
    if (!w.stamps && !tn.stamps_path.empty()) { // diagnostics: per-wave start/end times of the scan
        if ((rc = dev_alloc(w.stamps, kStampsWords))) return rc;
        HIP_TRY(hipMemset(w.stamps, 0, 8ull * kStampsWords));
    }
    if (!w.sticky) {
        if ((rc = dev_alloc(w.sticky, 4))) return rc;
        HIP_TRY(hipMemset(w.sticky, 0, 16));
    }
    return ISSL_OK;
}

// The scoring pipeline.  Guides and outputs are device pointers on ix->device.
// enqueue_batch() only launches (no host round trip); finish_batches() synchronises, checks the sticky overflow
// words the pipelines leave behind, and fills the statistics.
// `staged`: record an event at every stage boundary (bin / scan / verify / group / replay times in issl_stats).  An event
// record costs ~4 us of stream time on MI355X -- 5 % of a 10 k-guide batch for the six of them -- so the asynchronous
// back-to-back path records only the pair around the scan and the end of the batch unless the stage_timing knob is set.
// `pipelined` (asynchronous batches with the lanes option = 2): a software pipeline over two workspaces.  Binning and scan of
// a batch run on the lane's stream, its verify / group / replay on the lane's high-priority tail stream; the scans of
// consecutive batches are chained by events, so that they run one after the other at full speed while the short, latency-
// bound tail of batch i runs beside the scan of batch i + 1 -- a step then costs max(bin + scan, tail) instead of their sum.
// Is a batch worth the builds of scan and verify that can run the verify tail (Workspace::scan_verify)?  The batch's plan
// decides on the device whether the tail is armed (PlanInfo::scan_tail: kScanTailCands planned comparisons per scan wave);
// the launch that merely could arm it is measurably slower than the one that cannot (64 guides +2 %, 10 k guides x 50 M
// sites +1.4 %, profiles/ab_scan_verify_bench.log), so the host asks the same question first with what it knows: the mean
// group length of the index (an even index plans n x slices x ways x that), with a factor two of slack -- or, where the
// handle has finished a batch under the same prune mode, what that batch's plan came to per guide (a clustered or skewed
// index plans far more than its mean says).  A "no" here only means k_verify does the batch's records, as it always did.
static uint32_t tail_worth_arming(const issl_index *ix, size_t n, uint32_t prune_mode)
{
    const Tuning &tn = ix->tuning;
    if (tn.scan_verify == 0 || prune_mode == 0 || !(ix->view.srec || ix->view.sid)) return 0u;
    if (tn.scan_verify > 0) return 2u;
    const double want = static_cast<double>(kScanTailCands) * scan_waves(tn);
    const double slices = static_cast<double>(ix->hdr.n_slices);
    const double mean_group = static_cast<double>(ix->hdr.n_sites) * slices / (static_cast<double>(ix->hdr.n_buckets) * 256.0);
    const double even = static_cast<double>(n) * slices * fine_ways_of(prune_mode) * mean_group;
    const double learnt = ix->plan_cands_prune == prune_mode ? ix->plan_cands_per_guide * static_cast<double>(n) : 0.0;
    return (2.0 * even >= want || learnt >= want) ? 1u : 0u;
}

static int enqueue_batch(issl_index *ix, Lane &lane, hipStream_t stream, const uint64_t *d_guides, size_t n, int max_dist,
                         double threshold, int method, double *d_mit, double *d_cfd, bool dump, bool staged,
                         int lanes_mode = 1, issl_profile *d_profile = nullptr)
{
    // lanes_mode 2: the software pipeline described above.  3 ("binning ahead"): two workspaces as well, but only the BINNING
    // of a batch -- seven short, latency-bound launches, 0.19 ms at 100 k guides -- runs beside the batch before it; its scan
    // waits for that batch's replay, so the heavy kernels never share the chip (which is what made mode 2 lose: they share
    // its power budget).
    const bool pipelined = lanes_mode == 2, bin_ahead = lanes_mode == 3;
    if (!ix->d_image) {
        set_error("index has no device image: call issl_index_upload first");
        return ISSL_E_STATE;
    }
    // guide slots are 27-bit fields of the raw records: one slot per guide and slice + padding
    const size_t max_batch = std::min<size_t>(kMaxBatch, ((size_t(1) << 27) - kGuideGroup * ix->hdr.n_buckets) / std::max<uint64_t>(ix->hdr.n_slices, 1));
    if (n > max_batch) {
        set_error("at most " + std::to_string(max_batch) + " guides per device batch on this index (issl_score splits larger batches itself)");
        return ISSL_E_ARG;
    }
    HIP_TRY(hipSetDevice(ix->device));
    if (n == 0) return ISSL_OK;
    const uint32_t prune_mode = prune_mode_for(ix->view, ix->tuning, static_cast<uint32_t>(n), max_dist);
    int rc = ensure_workspace(ix, n, lane, fine_ways_of(prune_mode ? prune_mode : 2u));
    if (rc) return rc;
    Workspace &ws = lane.ws;
    const Tuning &tn = ix->tuning;
    // `sorted` always has room for every raw slot, so the whole pipeline runs without a host round trip;
    // an exhausted raw buffer is detected in finish_batches() and the batch is re-run with a larger one.
    rc = ensure_hit_capacity(ws, ws.cap_chunks * (kChunkRecs - 1));
    if (rc) return rc;
    if (dump && ws.cap_hitrec < ws.cap_hits) {
        rc = dev_alloc(ws.d_hitrec, ws.cap_hits);
        if (rc) return rc;
        ws.cap_hitrec = ws.cap_hits;
    }
    // issl_dump_hits wants every hit of the batch in one array in guide order: no hit slots there
    ws.slot_hits = (!dump && tn.hit_slots && ws.cap_slot_guides >= n) ? ws.slot_width : 0u;
    ws.lean_tail = (lane.lean && ws.slot_hits >= kSlotHits && tn.lean_tail) ? 1u : 0u;
    ws.scan_verify = max_dist < 0 ? 0u : tail_worth_arming(ix, n, prune_mode);
    ScoreParams p;
    p.max_dist = max_dist;
    p.method = method;
    p.maximum_sum = (10000.0 - threshold * 100) / threshold; // isslScoreOfftargets.cpp:326
    const uint32_t n32 = static_cast<uint32_t>(n);
    // The event pair around the scan (issl_stats::ms_scan_events): around every batch's (scan_events = 1; always where the stage
    // events are recorded too), around the first batch's after a finish (2, the default: the kernel's own clock stamps time
    // every launch anyway, ms_scan) or never (0) -- an event record is ~5 us of stream time, two of them a seventh of a
    // 64-guide batch.  Pipelined lanes chain their scans by these events: there, always.
    const bool scan_pair = staged || pipelined || tn.scan_events == 1 || (tn.scan_events == 2 && ix->n_ring == 0);
    const uint32_t slot = ix->n_ring % kRing;
    lane.staged = staged;
    if (pipelined && lane.pending) HIP_TRY(hipStreamWaitEvent(stream, lane.done, 0)); // the workspace's previous batch (tail stream)
    // (bin_ahead: the workspace's previous batch ran on this very stream)
    if (staged) HIP_TRY(hipEventRecord(lane.ev[0], stream));
    ws.span_slot = lane.pending % kSpanRing;
    launch_bin_guides(ix->view, ws, tn, d_guides, n32, prune_mode, stream);
    if (staged) HIP_TRY(hipEventRecord(lane.ev[1], stream));
    if (pipelined && ix->prev_scan_end) HIP_TRY(hipStreamWaitEvent(stream, ix->prev_scan_end, 0)); // one scan at a time
    if (bin_ahead && ix->prev_batch_end) HIP_TRY(hipStreamWaitEvent(stream, ix->prev_batch_end, 0)); // the batch before is through
    if (scan_pair) HIP_TRY(hipEventRecord(ix->ring[2 * slot], stream));
    launch_scan(ix->view, ws, tn, d_guides, n32, p, prune_mode, stream);
    if (scan_pair) HIP_TRY(hipEventRecord(ix->ring[2 * slot + 1], stream));
    if (scan_pair) ix->n_ring += 1;
    if (staged) HIP_TRY(hipEventRecord(lane.ev[2], stream));
    hipStream_t tail = stream;
    if (pipelined) {
        tail = lane.tail_stream;
        HIP_TRY(hipStreamWaitEvent(tail, ix->ring[2 * slot + 1], 0));
        ix->prev_scan_end = ix->ring[2 * slot + 1];
    }
    launch_verify(ix->view, ws, tn, d_guides, static_cast<uint32_t>(n), p, tail);
    if (staged) HIP_TRY(hipEventRecord(lane.ev[3], tail));
    launch_group_hits(ws, n32, tail);
    if (staged) HIP_TRY(hipEventRecord(lane.ev[4], tail));
    // (the off-target profile: the same batch up to here, its hits binned by distance instead of added up)
    if (d_profile) launch_profile(ix->view, ws, d_guides, n32, d_profile, tail);
    else launch_replay(ix->view, ws, d_guides, n32, p, d_mit, d_cfd, dump ? ws.d_kept : nullptr,
                       dump ? ws.d_hitrec : nullptr, tail);
    if (staged) HIP_TRY(hipEventRecord(lane.ev[5], tail));
    if (pipelined || bin_ahead) HIP_TRY(hipEventRecord(lane.done, tail)); // (what the other lane's batches wait for)
    lane.done_recorded = pipelined || bin_ahead; // (one lane: issl_score_wait records it when somebody asks)
    lane.last_tail = tail;
    if (bin_ahead) ix->prev_batch_end = lane.done;
    ix->n_pending += 1;
    lane.pending += 1;
    lane.last_n = n32;
    lane.last_max_dist = max_dist;
    lane.last_prune = prune_mode;
    ix->last_lane = &lane;
    return ISSL_OK;
}

// Synchronises everything that was enqueued (the internal stream and, for synchronous calls, `stream`).  Returns
// ISSL_OK, or ISSL_E_RETRY when a batch since the last finish ran out of raw-record space (the buffers have been
// enlarged; the caller enqueues those batches again).
int finish_batches(issl_index *ix, hipStream_t stream)
{
    if (!ix->d_image || ix->n_pending == 0) return ISSL_OK;
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipStreamSynchronize(stream));
    for (Lane *lp : {&ix->lane, &ix->lane2})
        if (lp->ready && lp->pending) {
            HIP_TRY(hipStreamSynchronize(lp->stream));
            HIP_TRY(hipStreamSynchronize(lp->tail_stream));
        }
    ix->prev_scan_end = nullptr;
    ix->prev_batch_end = nullptr;
    HIP_TRY(hipGetLastError());
    const uint32_t batches = ix->n_pending;
    const uint32_t ring_pairs = ix->n_ring; // scan event pairs recorded since the last finish (scan_events)
    ix->n_pending = 0;
    ix->n_ring = 0;
    bool retry = false;
    uint32_t max_chunks = 0; // of the lane whose counters are reported
    Lane &lane = ix->last_lane ? *ix->last_lane : ix->lane;
    double span_sum = 0.0;   // scan launches by the kernel's own clock stamps (ticks of 10 ns)
    uint32_t span_count = 0;
    for (Lane *lp : {&ix->lane, &ix->lane2}) {
        if (!lp->pending) continue;
        {
            const uint32_t have = lp->pending < kSpanRing ? lp->pending : kSpanRing;
            unsigned long long spans[2 * kSpanRing];
            HIP_TRY(hipMemcpy(spans, lp->ws.scan_span, 16 * have, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < have; ++i)
                if (spans[2 * i + 1] > spans[2 * i]) { span_sum += static_cast<double>(spans[2 * i + 1] - spans[2 * i]); ++span_count; }
        }
        lp->pending = 0;
        uint32_t sticky[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(sticky, lp->ws.sticky, sizeof sticky, hipMemcpyDeviceToHost));
        if (lp == &lane) max_chunks = sticky[1];
        if (sticky[2] & 2u) {
            HIP_TRY(hipMemset(lp->ws.sticky, 0, 16));
            set_error("internal error: scan item list overflow");
            return ISSL_E_DEVICE;
        }
        if (sticky[3] > lp->ws.cap_fitems && lp->ws.fitems) { // a pruned plan did not fit its item list: room for the next batch
            const size_t want = static_cast<size_t>(sticky[3]) + sticky[3] / 4 + 2;
            uint32_t zero = 0;
            HIP_TRY(hipMemcpy(lp->ws.sticky + 3, &zero, 4, hipMemcpyHostToDevice));
            int rc = dev_alloc(lp->ws.fitems, want + 1);
            if (rc) return rc;
            lp->ws.cap_fitems = want;
        }
        // Hit slots: when a good part of the last batch's guides had more than kSlotHits hits -- an index of billions of sites, a
        // skewed genome -- the next batches get slots for kSlotHitsWide of them (6.5 GB per 100 k guides), so that only what
        // lies beyond THAT passes through the grouping pass.  A matter of speed only: the results do not depend on the width.
        Counters c{};
        HIP_TRY(hipMemcpy(&c, lp->ws.counters, sizeof c, hipMemcpyDeviceToHost));
        lp->scan_verified = c.scan_verified; // (ws_scan_verified: the records of the lane's last batch that the scan's own waves verified)
        // (ws_scan_lds_buffers, ws_scan_raw_top, ws_raw_chunks: which way that batch's records went -- buffers verified from LDS, one
        // past the last chunk a buffer was copied to, chunks handed out)
        lp->scan_lds_buffers = c.lds_chunks;
        lp->scan_raw_top = c.raw_top;
        lp->raw_chunks = c.raw_chunks;
        if (lp->ws.slots && lp->ws.slot_width == kSlotHits && ix->tuning.hit_slots && lp->last_n) {
            const size_t want = lp->ws.cap_slot_guides * size_t(kSlotHitsWide) * sizeof(SlotRec);
            size_t free_b = 0, total_b = 0;
            if (c.overflowed > lp->last_n / 8 && want <= kSlotBytesMax && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                free_b > want + (size_t(4) << 30)) {
                SlotRec *wide = nullptr;
                if (hipMalloc(reinterpret_cast<void **>(&wide), want) == hipSuccess) {
                    (void)hipFree(lp->ws.slots);
                    lp->ws.slots = wide;
                    lp->ws.slot_width = kSlotHitsWide;
                } else {
                    (void)hipGetLastError();
                }
            }
        }
        // the lane's next batches go without the grouping pass and the many-hit replays while no batch meets a guide beyond
        // its hit slots (bit 2: one did; bit 1: and it had been enqueued lean -- once more, with the whole tail)
        lp->lean = (sticky[0] & 6u) == 0u && lp->ws.slot_hits >= kSlotHits;
        if (sticky[0] & 2u) retry = true;
        // (a lean batch's waves verify full buffers of records from their LDS, and those take no chunk: sticky[1] counts them in
        // -- Counters::lds_chunks --, so the batch that is run again in full finds the chunks it needs)
        if ((sticky[0] & 1u) || ((sticky[0] & 2u) && sticky[1] > lp->ws.cap_chunks)) {
            // sticky[1] = largest number of chunks any batch asked for
            int rc = ensure_raw_capacity(lp->ws, static_cast<size_t>(sticky[1]) + sticky[1] / 8 + 1024);
            if (rc) return rc;
            retry = true;
        }
        if (sticky[0]) HIP_TRY(hipMemset(lp->ws.sticky, 0, 16));
    }
    if (retry) {
        // The caller enqueues the same batches again, and two workspaces need not get them the same way round (n_async runs on:
        // an odd number of batches changes sides).  A workspace that saw only clean batches would be lean for the many-hit batch
        // of the repeat while the other turns lean again over ITS clean ones -- "again" for ever.  No lane is lean for the repeat.
        ix->lane.lean = false;
        ix->lane2.lean = false;
        set_error("a batch has to be scored again: its raw record buffer was too small (it has been enlarged), or it was enqueued "
                  "without the many-hit part of the pipeline and met a guide that needs it");
        return ISSL_E_RETRY;
    }
    PlanInfo pl{};
    uint32_t total_hits = 0;
    HIP_TRY(hipMemcpy(&pl, lane.ws.plan, sizeof pl, hipMemcpyDeviceToHost));
    if (pl.fine != 0u && lane.last_n != 0u && lane.last_max_dist >= 0) { // (tail_worth_arming)
        ix->plan_cands_per_guide = static_cast<double>(pl.candidates) / lane.last_n;
        ix->plan_cands_prune = pl.fine;
    }
    {   // scored off-targets of the last batch before any early exit: the per-guide counts k_verify left
        std::vector<uint32_t> counts(lane.last_n);
        if (lane.last_n) HIP_TRY(hipMemcpy(counts.data(), lane.ws.gcount, 4 * counts.size(), hipMemcpyDeviceToHost));
        for (uint32_t c : counts) total_hits += c;
    }
    // comparisons the scan workgroups of the last batch counted while they made them
    std::vector<uint64_t> counted(ix->tuning.scan_blocks);
    HIP_TRY(hipMemcpy(counted.data(), lane.ws.scan_count, 8 * counted.size(), hipMemcpyDeviceToHost));
    uint64_t compared = 0;
    for (uint64_t c : counted) compared += c;
    float ms[5] = {0, 0, 0, 0, 0};
    if (lane.staged)
        for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&ms[i], lane.ev[i], lane.ev[i + 1]);
    double scan_sum = 0.0;
    const uint32_t have = ring_pairs < kRing ? ring_pairs : kRing;
    for (uint32_t i = 0; i < have; ++i) {
        float t = 0;
        (void)hipEventElapsedTime(&t, ix->ring[2 * i], ix->ring[2 * i + 1]);
        scan_sum += t;
    }
    ix->stats = issl_stats{};
    ix->stats.n_guides = lane.last_n;
    ix->stats.ms_bin = ms[0];
    ix->stats.ms_scan_events = have ? scan_sum / have : ms[1]; // mean over the batches since the last finish
    ix->stats.ms_scan = span_count ? span_sum / span_count * 1e-5 : 0.0;
    ix->stats.ms_verify = ms[2];
    ix->stats.ms_group = ms[3];
    ix->stats.ms_replay = ms[4];
    ix->stats.ms_total = ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
    ix->stats.raw_records = static_cast<uint64_t>(max_chunks) * (kChunkRecs - 1);
    ix->stats.candidates = compared;
    ix->stats.planned_comparisons = lane.last_max_dist < 0 ? 0 : pl.candidates;
    ix->stats.reference_comparisons = pl.reference_candidates;
    ix->stats.pruned = lane.last_prune ? pl.fine : 0;
    ix->stats.hits = total_hits;
    ix->stats.scan_tiles = pl.tiles;
    ix->stats.n_batches = batches;
    if (lane.ws.stamps) { // scan_stamps knob: dump the wave stamps of the last scan (4 u64 per wave)
        std::vector<unsigned long long> st(kStampsWords);
        HIP_TRY(hipMemcpy(st.data(), lane.ws.stamps, 8ull * kStampsWords, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(ix->tuning.stamps_path.c_str(), "wb")) {
            std::fwrite(st.data(), 8, st.size(), f);
            std::fclose(f);
        }
    }
    return ISSL_OK;
}

// Synchronous batch on the caller's stream.
int score_core(issl_index *ix, const uint64_t *d_guides, size_t n, int max_dist, double threshold, int method,
               double *d_mit, double *d_cfd, hipStream_t stream, bool dump, issl_profile *d_profile)
{
    int rc = finish_batches(ix, stream); // anything enqueued asynchronously before
    if (rc) return rc;
    ix->stats = issl_stats{};
    ix->stats.n_guides = n;
    if (n == 0) return ISSL_OK;
    for (int attempt = 0;; ++attempt) {
        rc = enqueue_batch(ix, ix->lane, stream, d_guides, n, max_dist, threshold, method, d_mit, d_cfd, dump, true, 1, d_profile);
        if (rc) return rc;
        rc = finish_batches(ix, stream);
        if (rc == ISSL_OK) {
            ix->stats.scan_launches = attempt + 1;
            return ISSL_OK;
        }
        if (rc != ISSL_E_RETRY) return rc;
        if (attempt >= 6) {
            set_error("internal error: raw record buffer kept overflowing");
            return ISSL_E_DEVICE;
        }
    }
}

// A batch of guides in host memory, in pieces (issl_score, the off-target report): run_piece(at, cnt) puts guides[at, at + cnt)
// through score_core on the lane's workspace, which is sized for them when it is called; the handle's statistics are
// the pieces' totals afterwards.
template <class RunPiece>
static int for_each_piece(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, RunPiece &&run_piece)
{
    HIP_TRY(hipSetDevice(idx->device));
    // Crackling hands over pages of up to 5 M guides (config.ini:112); larger batches go through in pieces of at most
    // 2^22 guides.  The guides are in host memory here, so the comparison count is five table look-ups per guide
    // away (SURVEY 8d cross-check).  Uniform data leaves one raw record per ~26 k comparisons (16 positions, <= 4
    // mismatches); the record buffers (32 B per slot with the sorted keys and score terms) are sized for twice
    // that up front, which saves the first large batch on an index its grow-and-rerun round, and a piece ends
    // early when its estimate would not fit a quarter of the free HBM.  Denser data still grows the buffers.
    // (the pruned scan places every guide in up to 65 groups: pieces of at most 2^20 guides while it may be chosen)
    const uint32_t piece_mode = prune_mode_for(idx->view, idx->tuning, 1, max_dist);
    size_t piece = piece_mode ? size_t(prune_max_guides(piece_mode, idx->view.n_slices)) : size_t(1) << 22;
    // ... and of no more guides than get hit slots (kSlotBytesMax: 512 k): a batch beyond that sends every hit through the
    // grouping pass -- 4 ms per million guides on an even index, where two batches of half a million pay nothing for it
    // (kernels 23.3 -> 21.6 ms) --, in pieces of equal size (a page of 1 M guides: 2 x 500 k, not 512 k + 488 k).
    if (idx->tuning.hit_slots) piece = std::min(piece, kSlotBytesMax / (size_t(kSlotHits) * sizeof(SlotRec)));
    {
        const size_t n_pieces = (n + piece - 1) / piece;
        piece = std::min(piece, (((n + n_pieces - 1) / n_pieces) + 7) & ~size_t(7));
    }
    // Every piece is cut where its estimated records would outgrow the record buffers this handle may have: five table
    // look-ups per guide.  What is skipped on a handle whose buffers already cover a piece is only the question how much
    // memory is free (hipMemGetInfo: asked lazily, once per call, when a piece's estimate first exceeds the buffers in
    // hand) and the call that grows them.  (Small pages: the default buffers do.)
    const bool estimate = !idx->tuning.raw_chunks && n >= (size_t(1) << 15);
    const double records_per_comparison = 8e-5;
    double budget_slots = -1.0; // records the buffers may grow to: the larger of what they hold and a quarter of the free HBM (<= 32 GiB)
    const uint64_t per = idx->geo.buckets_per_slice();
    if (estimate && !idx->worst_per_guide) // the most a guide can be compared with: the longest bucket of every slice
        for (uint64_t sl = 0; sl < idx->geo.n_slices; ++sl)
            idx->worst_per_guide += *std::max_element(idx->bucket_sizes.begin() + sl * per, idx->bucket_sizes.begin() + (sl + 1) * per);
    const size_t wave_chunks = size_t(scan_waves(idx->tuning)) * 10; // every scan wave's own first chunk and the unused tail of its last reservation of up to 16
    issl_stats total{};
    for (size_t at = 0; at < n;) {
        uint64_t cand = 0;
        size_t cnt = 0;
        const size_t most = std::min(piece, n - at);
        const size_t cap_chunks = idx->lane.ws.cap_chunks;
        const double have_slots = static_cast<double>(cap_chunks > wave_chunks ? cap_chunks - wave_chunks : 0) * (kChunkRecs - 1);
        // (an index of even buckets on a handle that has grown its buffers: the bound alone says the piece fits)
        const bool covered = static_cast<double>(most) * static_cast<double>(idx->worst_per_guide) * records_per_comparison <= have_slots ||
                             (most <= idx->proven_guides && cap_chunks >= idx->proven_chunks && idx->proven_chunks > 0 && max_dist <= idx->proven_dist);
        if (!estimate || covered) cnt = most;
        while (estimate && !covered && at + cnt < n && cnt < piece) {
            uint64_t c = 0;
            for (uint64_t sl = 0; sl < idx->geo.n_slices; ++sl)
                c += idx->bucket_sizes[sl * per + ((guides[at + cnt] >> (idx->geo.slice_width * sl)) & (per - 1))];
            const double want = static_cast<double>(cand + c) * records_per_comparison;
            if (want > have_slots) { // beyond the buffers in hand: may they grow that far?
                if (budget_slots < 0.0) {
                    size_t free_b = 0, total_b = 0;
                    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
                    budget_slots = std::max(have_slots, static_cast<double>(std::min<size_t>(free_b / 4, size_t(32) << 30)) / 32.0);
                }
                if (cnt > 0 && want > budget_slots) break;
            }
            cand += c;
            ++cnt;
        }
        Workspace &ws = idx->lane.ws;
        int rc = finish_batches(idx, nullptr); // asynchronous batches may still use the staging buffers
        if (rc) return rc;
        rc = ensure_workspace(idx, cnt, idx->lane);
        if (rc) return rc;
        if (estimate && !covered) {
            double slots = static_cast<double>(cand) * records_per_comparison;
            if (budget_slots >= 0.0) slots = std::min(slots, budget_slots);
            // (a buffer that has to grow grows by a quarter at least: the pieces of a page have estimates a few per cent apart, and
            // every step up is a free and an allocation of gigabytes -- the record buffer and the four arrays sized by it)
            size_t want_chunks = static_cast<size_t>(slots / (kChunkRecs - 1)) + wave_chunks;
            if (want_chunks > ws.cap_chunks && ws.cap_chunks > 0) {
                const size_t roomy = ws.cap_chunks + ws.cap_chunks / 4;
                const size_t most_chunks = budget_slots >= 0.0 ? static_cast<size_t>(budget_slots / (kChunkRecs - 1)) + wave_chunks : roomy;
                want_chunks = std::max(want_chunks, std::min(roomy, std::max(most_chunks, want_chunks)));
            }
            rc = ensure_raw_capacity(ws, want_chunks);
            if (rc) return rc;
        }
        rc = run_piece(at, cnt);
        if (rc) return rc;
        const issl_stats &s = idx->stats;
        // (a piece that went through at once: the next ones within its size and distance need no estimate; denser guides than
        // these still take the grow-and-rerun round)
        if (s.scan_launches == 1 && (max_dist > idx->proven_dist || (max_dist == idx->proven_dist && cnt > idx->proven_guides))) {
            idx->proven_dist = max_dist;
            idx->proven_guides = cnt;
            idx->proven_chunks = ws.cap_chunks;
        }
        total.n_guides += s.n_guides; total.candidates += s.candidates; total.hits += s.hits;
        total.planned_comparisons += s.planned_comparisons; total.reference_comparisons += s.reference_comparisons;
        total.pruned = std::max(total.pruned, s.pruned);
        total.scan_tiles += s.scan_tiles; total.ms_bin += s.ms_bin; total.ms_scan += s.ms_scan;
        total.ms_scan_events += s.ms_scan_events;
        total.ms_verify += s.ms_verify; total.ms_group += s.ms_group; total.ms_replay += s.ms_replay;
        total.ms_total += s.ms_total; total.scan_launches += s.scan_launches;
        total.raw_records = std::max(total.raw_records, s.raw_records); total.n_batches += s.n_batches;
        at += cnt;
    }
    idx->stats = total;
    return ISSL_OK;
}

// issl_score: a batch of guides in host memory, in pieces.
int score_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
               double *mit, double *cfd)
{
    return for_each_piece(idx, guides, n, max_dist, [&](size_t at, size_t cnt) -> int {
        Workspace &ws = idx->lane.ws;
        int rc;
        if (ensure_stage(ws, 24 * cnt)) { // guides in, scores out through pinned memory: one DMA each, one synchronisation
            uint64_t *sg = static_cast<uint64_t *>(ws.h_stage);
            double *sm = reinterpret_cast<double *>(sg + cnt), *sc = sm + cnt;
            std::memcpy(sg, guides + at, 8 * cnt);
            HIP_TRY(hipMemcpyAsync(ws.d_guides, sg, 8 * cnt, hipMemcpyHostToDevice, nullptr));
            rc = score_core(idx, ws.d_guides, cnt, max_dist, threshold, method, ws.d_mit, ws.d_cfd, nullptr, false);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(sm, ws.d_mit, 8 * cnt, hipMemcpyDeviceToHost, nullptr));
            HIP_TRY(hipMemcpyAsync(sc, ws.d_cfd, 8 * cnt, hipMemcpyDeviceToHost, nullptr));
            HIP_TRY(hipStreamSynchronize(nullptr));
            std::memcpy(mit + at, sm, 8 * cnt);
            std::memcpy(cfd + at, sc, 8 * cnt);
        } else {
            HIP_TRY(hipMemcpy(ws.d_guides, guides + at, 8 * cnt, hipMemcpyHostToDevice));
            rc = score_core(idx, ws.d_guides, cnt, max_dist, threshold, method, ws.d_mit, ws.d_cfd, nullptr, false);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(mit + at, ws.d_mit, 8 * cnt, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cfd + at, ws.d_cfd, 8 * cnt, hipMemcpyDeviceToHost));
        }
        return ISSL_OK;
    });
}

// issl_dump_hits: every hit of at most 2^22 guides, in guide order.
int dump_hits(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold, int method,
              issl_hit *hits, size_t cap, size_t *n_hits)
{
    HIP_TRY(hipSetDevice(idx->device));
    int rc = finish_batches(idx, nullptr);
    if (rc) return rc;
    Workspace &ws = idx->lane.ws;
    rc = ensure_workspace(idx, n, idx->lane);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(ws.d_guides, guides, 8 * n, hipMemcpyHostToDevice));
    rc = score_core(idx, ws.d_guides, n, max_dist, threshold, method, ws.d_mit, ws.d_cfd, nullptr, true);
    if (rc) return rc;
    std::vector<uint32_t> goff(n + 1), kept(n);
    HIP_TRY(hipMemcpy(goff.data(), ws.goff, 4 * (n + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(kept.data(), ws.d_kept, 4 * n, hipMemcpyDeviceToHost));
    std::vector<issl_hit> all(goff[n]);
    if (goff[n]) HIP_TRY(hipMemcpy(all.data(), ws.d_hitrec, sizeof(issl_hit) * goff[n], hipMemcpyDeviceToHost));
    size_t total = 0;
    for (size_t g = 0; g < n; ++g) {
        for (uint32_t k = 0; k < kept[g]; ++k) {
            if (total < cap) hits[total] = all[goff[g] + k];
            ++total;
        }
    }
    *n_hits = total;
    return ISSL_OK;
}

// ---- off-target report ------------------------------------------------------------------------
// (CallBuffer, issl_index.hpp: a device buffer of the call -- the piece's profiles, the piece's records)

// issl_offtarget_profile_device: the scoring pipeline with the profile kernels in the replay's place.  Neither score is
// asked of k_verify (ISSL_METHOD_UNKNOWN): the distance and the count are all the profile reads.
int profile_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, issl_profile *d_out, hipStream_t stream)
{
    return score_core(idx, d_guides, n, max_dist, 0.0, ISSL_METHOD_UNKNOWN, nullptr, nullptr, stream, false, d_out);
}

int profile_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, issl_profile *out)
{
    CallBuffer prof;
    return for_each_piece(idx, guides, n, max_dist, [&](size_t at, size_t cnt) -> int {
        Workspace &ws = idx->lane.ws;
        int rc = prof.reserve(sizeof(issl_profile) * cnt);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(ws.d_guides, guides + at, 8 * cnt, hipMemcpyHostToDevice));
        rc = profile_device(idx, ws.d_guides, cnt, max_dist, static_cast<issl_profile *>(prof.p), nullptr);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(out + at, prof.p, sizeof(issl_profile) * cnt, hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

// One batch of the record list: every hit grouped and expanded in scoring order by the replay (as issl_dump_hits has
// them; threshold 0: maximum_sum = +inf, no exit), offsets from the grouping pass's prefix, then -- when the caller has
// room for them -- the records.  Leaves the batch's number of records in *n_records; synchronises `stream`.
static int offtargets_batch(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, uint64_t base, size_t guide_base,
                            uint64_t *d_offsets, issl_offtarget *d_recs, size_t room, uint32_t *n_records, hipStream_t stream)
{
    Workspace &ws = idx->lane.ws;
    int rc = score_core(idx, d_guides, n, max_dist, 0.0, ISSL_METHOD_AND, ws.d_mit, ws.d_cfd, stream, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(n_records, ws.goff + n, 4, hipMemcpyDeviceToHost, stream));
    if (d_offsets) launch_report_offsets(ws, static_cast<uint32_t>(n), base, d_offsets, stream);
    HIP_TRY(hipStreamSynchronize(stream));
    if (d_recs && *n_records <= room) {
        launch_report_emit(idx->view, ws, d_guides, *n_records, static_cast<uint32_t>(guide_base), d_recs, stream);
        HIP_TRY(hipStreamSynchronize(stream));
    }
    HIP_TRY(hipGetLastError());
    return ISSL_OK;
}

int offtargets_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, uint64_t *d_offsets,
                      issl_offtarget *d_recs, size_t cap, size_t *n_total, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(idx->device));
    *n_total = 0;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ISSL_OK;
    }
    int rc = finish_batches(idx, stream);
    if (rc) return rc;
    rc = ensure_workspace(idx, std::min(n, kMaxBatch), idx->lane); // (the replay's score outputs: the workspace's; a batch too large is refused by enqueue_batch)
    if (rc) return rc;
    uint32_t records = 0;
    rc = offtargets_batch(idx, d_guides, n, max_dist, 0, 0, d_offsets, d_recs, cap, &records, stream);
    if (rc) return rc;
    *n_total = records;
    return ISSL_OK;
}

// issl_offtargets.  The records reach the caller's array only when all of them fit, and that is known once every piece
// has been counted: a batch of several pieces is counted first (the scoring pipeline, no score asked for: k_verify's
// per-guide counts are the answer) and listed in a second pass.  Below 2^15 guides for_each_piece never cuts, and the
// one piece is listed at once.
int offtargets_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, uint64_t *offsets, issl_offtarget *recs,
                    size_t cap, size_t *n_total)
{
    HIP_TRY(hipSetDevice(idx->device));
    offsets[0] = 0;
    *n_total = 0;
    if (n == 0) return ISSL_OK;
    const bool one_piece = n < (size_t(1) << 15);
    uint64_t run = 0;
    if (!recs || !one_piece) {
        std::vector<uint32_t> counts;
        int rc = for_each_piece(idx, guides, n, max_dist, [&](size_t at, size_t cnt) -> int {
            Workspace &ws = idx->lane.ws;
            HIP_TRY(hipMemcpy(ws.d_guides, guides + at, 8 * cnt, hipMemcpyHostToDevice));
            int prc = score_core(idx, ws.d_guides, cnt, max_dist, 0.0, ISSL_METHOD_UNKNOWN, ws.d_mit, ws.d_cfd, nullptr, false);
            if (prc) return prc;
            counts.resize(cnt);
            HIP_TRY(hipMemcpy(counts.data(), ws.gcount, 4 * cnt, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; ++i) { run += counts[i]; offsets[at + i + 1] = run; }
            return ISSL_OK;
        });
        if (rc) return rc;
        *n_total = run;
        if (!recs || run > cap) return ISSL_OK;
    }
    CallBuffer out;
    std::vector<uint32_t> goff;
    run = 0;
    bool fits = true;
    int rc = for_each_piece(idx, guides, n, max_dist, [&](size_t at, size_t cnt) -> int {
        Workspace &ws = idx->lane.ws;
        HIP_TRY(hipMemcpy(ws.d_guides, guides + at, 8 * cnt, hipMemcpyHostToDevice));
        uint32_t records = 0;
        int prc = offtargets_batch(idx, ws.d_guides, cnt, max_dist, 0, 0, nullptr, nullptr, 0, &records, nullptr);
        if (prc) return prc;
        goff.resize(cnt + 1);
        HIP_TRY(hipMemcpy(goff.data(), ws.goff, 4 * (cnt + 1), hipMemcpyDeviceToHost));
        for (size_t i = 1; i <= cnt; ++i) offsets[at + i] = run + goff[i];
        if (run + records > cap) fits = false; // (one piece, not counted before: nothing is written)
        if (fits && records) {
            if ((prc = out.reserve(sizeof(issl_offtarget) * size_t(records)))) return prc;
            launch_report_emit(idx->view, ws, ws.d_guides, records, static_cast<uint32_t>(at), static_cast<issl_offtarget *>(out.p), nullptr);
            HIP_TRY(hipMemcpy(recs + run, out.p, sizeof(issl_offtarget) * size_t(records), hipMemcpyDeviceToHost));
        }
        run += records;
        return ISSL_OK;
    });
    if (rc) return rc;
    *n_total = run;
    return ISSL_OK;
}

// ---- off-target records left on the device (issl_offtarget_landings*, issl_landing.hip) ----------------------------
// One batch: offtargets_batch, then the records into `buf`.  Everything is enqueued on `stream`; the records are there
// for what is enqueued behind them.
static int records_batch(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, size_t guide_base, CallBuffer &buf,
                         RecordBatch &out, hipStream_t stream)
{
    Workspace &ws = idx->lane.ws;
    uint32_t records = 0;
    int rc = offtargets_batch(idx, d_guides, n, max_dist, 0, 0, nullptr, nullptr, 0, &records, stream);
    if (rc) return rc;
    if (records) {
        if ((rc = buf.reserve(sizeof(issl_offtarget) * size_t(records)))) return rc;
        launch_report_emit(idx->view, ws, d_guides, records, static_cast<uint32_t>(guide_base), static_cast<issl_offtarget *>(buf.p), stream);
        HIP_TRY(hipGetLastError());
    }
    out = RecordBatch{d_guides, n, guide_base, static_cast<const issl_offtarget *>(buf.p), records, ws.goff};
    return ISSL_OK;
}

int records_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, CallBuffer &buf, RecordBatch &out, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(idx->device));
    int rc = finish_batches(idx, stream);
    if (rc) return rc;
    rc = ensure_workspace(idx, std::min(n, kMaxBatch), idx->lane);
    if (rc) return rc;
    return records_batch(idx, d_guides, n, max_dist, 0, buf, out, stream);
}

int records_host(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, CallBuffer &buf,
                 const std::function<int(const RecordBatch &)> &use)
{
    return for_each_piece(idx, guides, n, max_dist, [&](size_t at, size_t cnt) -> int {
        Workspace &ws = idx->lane.ws;
        HIP_TRY(hipMemcpy(ws.d_guides, guides + at, 8 * cnt, hipMemcpyHostToDevice));
        RecordBatch batch;
        if (int rc = records_batch(idx, ws.d_guides, cnt, max_dist, at, buf, batch, nullptr)) return rc;
        return use(batch);
    });
}

// issl_score_device_async: one batch enqueued on a lane's internal stream.
int score_async(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, double threshold, int method,
                double *d_mit, double *d_cfd, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(idx->device));
    // lanes option = 2: consecutive batches use different workspaces and streams, so that the short, latency-bound
    // kernels behind one batch's scan run in the wave slots the next batch's scan leaves free: +9-11 % guides/s at 100 k
    // guides x 300 M sites; every kernel then shares the chip and takes longer, which is why it is not the default
    Lane &lane = (idx->tuning.lanes >= 2 && (idx->n_async++ & 1u)) ? idx->lane2 : idx->lane;
    int rc = ensure_workspace(idx, n, lane); // creates the internal stream on first use
    if (rc) return rc;
    if (stream) { // inputs are produced on the caller's stream: the batch starts after what is enqueued there now
        HIP_TRY(hipEventRecord(lane.ev[0], stream));
        HIP_TRY(hipStreamWaitEvent(lane.stream, lane.ev[0], 0));
    }
    return enqueue_batch(idx, lane, lane.stream, d_guides, n, max_dist, threshold, method, d_mit, d_cfd, false,
                         idx->tuning.stage_timing, idx->tuning.lanes);
}

// issl_score_wait: `stream` waits for every batch enqueued so far.
int wait_batches(issl_index *idx, hipStream_t stream)
{
    if (idx->device >= 0) HIP_TRY(hipSetDevice(idx->device));
    for (Lane *lp : {&idx->lane, &idx->lane2})
        if (lp->ready && lp->pending) {
            if (!lp->done_recorded) { // the end of the lane's last batch, recorded now: everything enqueued on its stream so far
                HIP_TRY(hipEventRecord(lp->done, lp->last_tail));
                lp->done_recorded = true;
            }
            HIP_TRY(hipStreamWaitEvent(stream, lp->done, 0));
        }
    return ISSL_OK;
}

} // namespace issl
