// k_verify: the exact test of the scan's raw records, keys and MIT / CFD terms of the hits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "issl_kernels.hpp"

namespace issl {

// Exact check of the raw records, IN PLACE: one thread per record, one chunk per 128-thread workgroup.
// A record that survives becomes a hit: key guide<<37 | slice<<32 | site id (list-order layouts: position in the
// bucket's list), rank inside its guide from the per-guide counter, MIT / CFD terms.  With hit slots the first
// ws.slot_hits hits of a guide are written to its slots; what lies beyond overwrites the record with its key for the
// grouping pass; every other slot of the chunk becomes kDeadKey.
__global__ __launch_bounds__(kChunkRecs, 8) void k_verify(ImageView v, Workspace ws, const uint64_t *__restrict__ guides,
                                                       uint32_t n, ScoreParams p)
{
    short_kernel_priority();
    const int max_dist = p.max_dist;
    const bool calc_mit = p.method == ISSL_METHOD_MIT || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const bool calc_cfd = p.method == ISSL_METHOD_CFD || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const uint32_t prune_mode = ws.plan->fine; // what the scan of this batch worked through
    uint32_t n_chunks = ws.counters->raw_chunks;
    if (blockIdx.x == 0 && threadIdx.x == 0) { // what the host needs to know after any number of batches
        if (ws.counters->raw_overflow) atomicOr(&ws.sticky[0], 1u);
        atomicMax(&ws.sticky[1], n_chunks);
        if (ws.plan->error) atomicOr(&ws.sticky[2], ws.plan->error);
    }
    if (n_chunks > ws.cap_chunks) n_chunks = static_cast<uint32_t>(ws.cap_chunks);
    const uint64_t low = (1ull << v.slice_width) - 1ull;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        // The passes behind the scan are chains of dependent loads at full occupancy: what they cost is the number of
        // links.  Header and record of the chunk are asked for together (a chunk always has its 128 slots), then the
        // stream record and the guide's signature (bucket-level plan: the guide slot's two words) together, then -- nothing
        // more before the exact test.
        uint64_t *recs = ws.raw + static_cast<uint64_t>(chunk) * kChunkRecs;
        const uint32_t t = threadIdx.x + 1u;
        const uint64_t rec_any = recs[t < kChunkRecs ? t : 0u];
        const uint32_t used = ws.raw_used[chunk];
        const bool in_use = t < used && t < kChunkRecs; // every lane stays: the counting below is done by the wave
        const uint64_t rec = in_use ? rec_any : 0ull;
        uint64_t key = kDeadKey;
        double mit_term = 0.0, cfd_term = 0.0; // of a record that survives: computed here, one thread per hit, so that the
                                               // replay (one wave per guide, a chain of dependent steps) only adds them up
        uint64_t hit_gsig = 0, hit_ot = 0;     // ... from these
        uint32_t hit_occ = 0;
        const uint32_t offset = static_cast<uint32_t>(rec) & (kTileCands - 1u);
        const uint32_t tile = static_cast<uint32_t>(rec >> 11) & 0x3FFFFFFu;
        const uint32_t gslot = static_cast<uint32_t>(rec >> 37); // pruned scan: the slot's id, not its number
        // sorted layouts: what the stream holds at the record's place, asked for before anything else is known about it
        const bool by_id = v.srec || v.sid; // the scoring order is (slice, site id): ImageHeader
        StreamRec sr_early{};
        if (in_use && v.srec) sr_early = v.srec[static_cast<uint64_t>(tile) * kTileCands + offset];
        else if (in_use && v.sid) sr_early.id = v.sid[static_cast<uint64_t>(tile) * kTileCands + offset];
        // Whose record it is.  Pruned scan: the record says so itself (slot_id: guide and slice; the bucket follows from the
        // slice and the guide's signature, which is asked for beside the stream record, not behind it).  Bucket-level plan:
        // the guide slot knows its guide and its bucket -- no search for the tile's.
        uint32_t guide = kNoGuide, bucket = 0, slice = 0;
        uint64_t gsig = 0;
        if (in_use) {
            if (prune_mode) {
                if (gslot != kPadSlotId) slot_id_unpack(gslot, slice, guide);
                if (guide >= n || slice >= v.n_slices) guide = kNoGuide; // (a padding slot, or no slot of this batch at all)
                else {
                    gsig = guides[guide];
                    bucket = (slice << v.slice_width) + (static_cast<uint32_t>(gsig >> (v.slice_width * slice)) & static_cast<uint32_t>(low));
                }
            } else {
                guide = ws.gidx[gslot];
                bucket = ws.gbucket[gslot];
                slice = bucket >> v.slice_width;
            }
        }
        if (guide != kNoGuide) {
            // Is the candidate the item's?  The scan notes only candidates of the item's own window (`keep`: not the zero
            // padding behind a bucket, not the neighbouring group that shares the tile), so on the sorted layouts, which need
            // nothing else from the bucket tables, the question is not asked again.  The list-order layouts find their list
            // entry through the bucket's start and check on the way.
            uint64_t start = 0, pos = 0;
            bool mine = true;
            if (!by_id) {
                start = v.bucket_start[bucket];
                pos = static_cast<uint64_t>(tile - v.tile_first[bucket]) * kTileCands + offset; // in the stream
                mine = pos < v.bucket_start[bucket + 1] - start;
            }
            if (mine) {
                if (!prune_mode) gsig = guides[guide];
                // sorted layouts: signature, site id (and a 24-bit copy of the count) come in one stream-order record, or --
                // compact -- the id alone, with the signature behind it in the site table
                StreamRec sr = sr_early;
                if (v.sid) sr.sig = v.sites[sr.id]; // (the site table of a sorted layout: signature | 24-bit count << 40, like a stream record)
                const uint64_t ot = by_id    ? sr.sig & kSigMask
                                    : v.esig ? v.esig[start + pos]
                                    : v.occ8 ? candidate_signature(v, bucket, tile, offset) // cold sections in host memory
                                             : v.sites[v.entries[start + pos] & 0xFFFFFFFFull];
                if (__builtin_popcountll(mismatch_mask(gsig, ot)) <= max_dist) { // exact, full signatures (:376-382)
                    // First-matching-slice rule (equivalent of the seen bitmap, isslScoreOfftargets.cpp:385-390,463):
                    // the site was already met iff an earlier slice of the XOR is all zero.
                    const uint64_t x = gsig ^ ot;
                    if (!prune_mode) {
                        bool earlier = false;
                        for (uint32_t j = 0; j < slice; ++j)
                            if (((x >> (v.slice_width * j)) & low) == 0) earlier = true;
                        if (!earlier) {
                            // list-order layouts: the key carries the position in the bucket's list, which is the stream
                            // position; sorted layouts: the site id (lists ascend by id, so the order is the same)
                            const uint64_t lp = by_id ? sr.id : pos;
                            key = (static_cast<uint64_t>(guide) << kKeyGuideShift) | (static_cast<uint64_t>(slice) << kKeySliceShift) | lp;
                        }
                    } else {
                        // Pruned scan: the guide meets this site once in every exactly matching slice whose successor
                        // slice has at most `tol` mismatches (k_fine_count); the smallest such slice reports it, under
                        // the slice the reference would meet it in first.
                        const uint32_t tol = prune_mode - 1u; // 0, 1, 2 mismatches allowed in the successor slice
                        const uint64_t mm = mismatch_mask(gsig, ot);
                        uint32_t first = slice, reporter = slice;
                        for (uint32_t j = slice; j-- > 0;) {
                            if (((x >> (v.slice_width * j)) & low) != 0) continue;
                            first = j;
                            if (static_cast<uint32_t>(__builtin_popcount(succ_byte(mm, j, v.slice_width))) <= tol) reporter = j; // (the successor unit's flags)
                        }
                        if (reporter == slice)
                            key = (static_cast<uint64_t>(guide) << kKeyGuideShift) | (static_cast<uint64_t>(first) << kKeySliceShift) | sr.id;
                    }
                    if (key != kDeadKey) { // the hit will be scored: what its terms are made of (:348)
                        uint32_t occ;
                        if (by_id) {
                            occ = static_cast<uint32_t>(sr.sig >> 40);
                            if (occ == kOccSaturated) occ = v.site_occ[sr.id];
                        } else if (v.occ8) {
                            occ = v.occ8[start + pos];
                            if (occ == 255u) occ = static_cast<uint32_t>(v.entries[start + pos] >> 32); // (host memory)
                        } else {
                            occ = static_cast<uint32_t>(v.entries[start + pos] >> 32);
                        }
                        hit_gsig = gsig; hit_ot = ot; hit_occ = occ;
                    }
                }
            }
        }
        // Count the hit for its guide.  The count doubles as the hit's place in the guide's segment, so that the grouping
        // pass scatters without a second atomic (ws.rank, by raw-record slot).  The hits of a guide in one unit lie side by
        // side in the chunk (the scan wave notes them guide by guide): every RUN of neighbouring lanes with the same guide
        // takes one atomic, issued by its first lane -- no loop, every run of the wave in the same instruction.  (The
        // atomics are half of this kernel's time on a skewed index: profiles/r03_ablation_verify.log.)
        const bool live = key != kDeadKey;
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t prev_guide = static_cast<uint32_t>(__shfl_up(static_cast<int>(live ? guide : kNoGuide), 1, 64));
        const bool continues = live && lane != 0u && prev_guide == guide;    // (a dead lane never equals a live one: kNoGuide)
        const uint64_t starts = __ballot(!continues);                        // first lanes of runs, and the dead lanes
        uint32_t rank = 0;
        if (starts == ~0ull) { // (uniform over the wave) no runs, the usual case on an even index: everybody for itself
            if (live) rank = atomicAdd(&ws.gcount[guide], 1u);
        } else {
            const uint64_t upto = (lane == 63u ? 0ull : (~0ull << (lane + 1u))); // the lanes above this one
            const uint32_t head = 63u - static_cast<uint32_t>(__builtin_clzll(starts & ~upto)); // lane 0 always starts: never empty
            const uint64_t later = starts & upto;
            const uint32_t next = later ? static_cast<uint32_t>(__builtin_ctzll(later)) : 64u;
            uint32_t base = 0;
            if (live && !continues) base = atomicAdd(&ws.gcount[guide], next - lane); // the run is [lane, next)
            rank = static_cast<uint32_t>(__shfl(static_cast<int>(base), static_cast<int>(head), 64)) + (lane - head);
        }
        if (live && rank == kReplayLds) atomicAdd(&ws.counters->overflowed, 1u); // the guide's first hit beyond what k_replay takes
        if (live && rank < ws.slot_hits) {
            // hit slots (Workspace): the hit goes to its final place at once and takes no part in the grouping pass
            int dist;
            score_terms(v, hit_gsig, hit_ot, hit_occ, calc_mit, calc_cfd, mit_term, cfd_term, dist);
            const uint64_t at = static_cast<uint64_t>(guide) * ws.slot_hits + rank;
            SlotRec r;
            r.mit = mit_term; r.cfd = cfd_term; r.key = key;
            r.pad = slot_pad(hit_occ, static_cast<uint32_t>(dist)); // (read by k_profile alone)
            ws.slots[at] = r;
            key = kDeadKey;
        } else if (live) {
            const uint64_t slot = static_cast<uint64_t>(chunk) * (kChunkRecs - 1u) + (t - 1u); // < cap_chunks * 127 <= cap_hits
            ws.rank[slot] = rank;
            // The terms (:392-460) -- unless the guide already has more hits than the replays that read them take
            // (k_replay, k_replay_mid): the many-hit replay works out the terms of the hits it walks by itself, and on
            // skewed data most hits belong to such guides and lie behind their early exit.
            if (rank < kMidHits) {
                int dist;
                score_terms(v, hit_gsig, hit_ot, hit_occ, calc_mit, calc_cfd, mit_term, cfd_term, dist);
                reinterpret_cast<double2 *>(ws.pay)[slot] = make_double2(mit_term, cfd_term);
            }
        }
        if (!in_use) continue;
        // (a lean batch has no grouping pass to read the keys back -- every hit went to its guide's slots, or the batch is run
        // again in full: 8 bytes per record that need not be written)
        if (!ws.lean_tail) recs[t] = key;
    }
}

void launch_verify(const ImageView &v, const Workspace &ws, const uint64_t *d_guides, uint32_t n, const ScoreParams &p, void *stream)
{
    if (p.max_dist < 0) return;
    // (the kernel strides over the chunks the scan used: a small batch's few thousand need no 16 384 workgroups to start and leave)
    const uint32_t grid = n < 256u ? std::max<uint32_t>(2048u, 64u * n) : kTailGrid;
    hipLaunchKernelGGL(k_verify, dim3(std::min(grid, kTailGrid)), dim3(kChunkRecs), 0, static_cast<hipStream_t>(stream), v, ws, d_guides, n, p);
}

} // namespace issl
