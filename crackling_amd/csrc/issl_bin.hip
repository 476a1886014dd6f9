// Both sides of the scan word: the image's scan stream, packed once at upload (k_pack_scan_stream), and the guides of a
// batch, binned by index bucket and, for the pruned scan, by (bucket, successor byte), with the scan's items and cost ranges.
// (The pack kernel is here and not beside the other upload kernels in issl_build.hip because it shares image_word with the
// guide scatter: the compiler specialises an inline helper for the callers its unit has, and only in this unit does the
// kernel come out as it always has.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "issl_kernels.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// upload: build the scan stream from sites + bucket entries
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_pack_scan_stream(ImageView v, uint32_t *__restrict__ scan_out,
                                                          uint64_t *__restrict__ esig_out,
                                                          uint8_t *__restrict__ occ8_out,
                                                          uint32_t *__restrict__ error_flag, uint32_t *__restrict__ seen,
                                                          uint32_t tile_begin, uint32_t tile_end)
{
    for (uint32_t t = tile_begin + blockIdx.x; t < tile_end; t += gridDim.x) {
        // bucket of tile t: last b with tile_first[b] <= t (uniform binary search)
        uint32_t lo = 0, hi = v.n_buckets;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (v.tile_first[mid] <= t) lo = mid; else hi = mid;
        }
        const uint32_t b = lo;
        const uint32_t slice = b >> v.slice_width;
        const uint64_t start = v.bucket_start[b];
        const uint64_t len = v.bucket_start[b + 1] - start;
        const uint64_t tile_pos = static_cast<uint64_t>(t - v.tile_first[b]) * kTileCands;
        // 64 consecutive candidates per wave and step: lane j computes the scan word of candidate j, then the
        // wave transposes the 64 x 32 bit matrix with ballots: plane r of the two 32-candidate groups is
        // the low / high half of ballot(bit r).  Lane r (< 32) keeps plane r and stores it.
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t wave = threadIdx.x >> 6;
        uint32_t *tile_out = scan_out + static_cast<uint64_t>(t) * kTileCands;
        for (uint32_t k0 = wave * 64u; k0 < kTileCands; k0 += 256u) {
            const uint64_t pos = tile_pos + k0 + lane;
            uint32_t w = 0;
            if (pos < len && (v.srec || v.sid)) {
                // sorted layouts: the stream holds the candidates v.srec / v.sid list (built and checked by launch_sort_slice)
                const uint64_t at = static_cast<uint64_t>(t) * kTileCands + k0 + lane; // the maps are indexed like the stream
                w = image_word(v.srec ? v.srec[at].sig & kSigMask : v.sites[v.sid[at]] & kSigMask, slice, v.slice_width, true);
            } else if (pos < len) {
                const uint64_t e = v.entries[start + pos];
                const uint64_t id = e & 0xFFFFFFFFull;
                if (id < v.n_sites) {
                    const uint64_t sig = v.sites[id] & kSigMask;
                    // Every slice must list every site once, in the bucket its signature selects: the scan compares the
                    // 16 positions outside the slice and the first-matching-slice rule stands in for the reference's
                    // seen-bitmap (:385-390) on exactly that premise.  `seen`: one bit per (slice, site).
                    if (((sig >> (v.slice_width * slice)) & ((1ull << v.slice_width) - 1ull)) != (b & ((1u << v.slice_width) - 1u)))
                        atomicOr(error_flag, 4u);
                    if (seen) {
                        const uint64_t bit = static_cast<uint64_t>(slice) * v.n_sites + id;
                        if (atomicOr(&seen[bit >> 5], 1u << (bit & 31u)) & (1u << (bit & 31u))) atomicOr(error_flag, 4u);
                    }
                    w = scan_word(sig, slice, v.slice_width);
                    if (esig_out) esig_out[start + pos] = sig;
                    if (occ8_out) occ8_out[start + pos] = static_cast<uint8_t>((e >> 32) < 255ull ? (e >> 32) : 255ull);
                } else {
                    atomicOr(error_flag, 1u);
                }
            }
            uint32_t mine_lo = 0, mine_hi = 0;
            for (uint32_t r = 0; r < 32; ++r) {
                const uint64_t m = __ballot((w >> r) & 1u);
                if (lane == r) { mine_lo = static_cast<uint32_t>(m); mine_hi = static_cast<uint32_t>(m >> 32); }
            }
            if (lane < 32) {
                const uint32_t group = k0 >> 5; // lane index (in the scan kernel) that owns candidates k0..k0+31
                tile_out[plane_word(lane, group)] = mine_lo;
                tile_out[plane_word(lane, group + 1u)] = mine_hi;
            }
        }
    }
}

// Tiles [tile_begin, tile_end) only: the upload of an image whose cold sections stay in host memory packs one slice
// at a time from temporary device copies (v.entries then points at the slice's list minus the slice's offset).
void launch_pack_scan_range(const ImageView &v, uint32_t *scan_out, uint64_t *esig_out, uint8_t *occ8_out,
                            uint32_t *error_flag, uint32_t *seen, uint32_t tile_begin, uint32_t tile_end, void *stream)
{
    if (tile_end <= tile_begin) return;
    const uint32_t n = tile_end - tile_begin;
    const uint32_t grid = n < 65536u ? n : 65536u;
    hipLaunchKernelGGL(k_pack_scan_stream, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                       scan_out, esig_out, occ8_out, error_flag, seen, tile_begin, tile_end);
}

void launch_pack_scan_stream(const ImageView &v, uint32_t *scan_out, uint64_t *esig_out, uint8_t *occ8_out,
                             uint32_t *error_flag, uint32_t *seen, void *stream)
{
    launch_pack_scan_range(v, scan_out, esig_out, occ8_out, error_flag, seen, 0u, v.n_tiles, stream);
}

// ------------------------------------------------------------------------------------------------
// guide binning
// ------------------------------------------------------------------------------------------------

constexpr uint32_t kMaxBuckets = 2048;

// Histogram of the guides' slice keys, and -- in the same launch -- the reset of everything a scoring call
// accumulates into (nothing here depends on it; the kernels that do come later on the stream).  ng and gfill are
// not reset here: k_plan leaves them zeroed for the next batch.
__global__ __launch_bounds__(256) void k_guide_hist(Workspace ws, const uint64_t *__restrict__ guides, uint32_t n,
                                                    uint32_t slice_width, uint32_t n_slices, uint32_t n_buckets,
                                                    uint32_t n_slots, uint32_t n_scan_waves)
{
    short_kernel_priority();
    __shared__ uint32_t hist[kMaxBuckets];
    for (uint32_t b = threadIdx.x; b < n_buckets; b += 256) hist[b] = 0;
    __syncthreads();
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < n) {
        const uint64_t sig = guides[g];
        const uint32_t low = (1u << slice_width) - 1u;
        for (uint32_t s = 0; s < n_slices; ++s) {
            const uint32_t key = static_cast<uint32_t>(sig >> (slice_width * s)) & low;
            atomicAdd(&hist[(s << slice_width) + key], 1u);
        }
    }
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t k = g; k < n_slots; k += stride) { ws.gidx[k] = kNoGuide; ws.gword[k] = kPadGuideWord; }
    for (uint32_t k = g; k <= n; k += stride) ws.gcount[k] = 0;
    // chunk fill counts: a chunk nobody writes must read as empty; chunks [0, n_scan_waves) belong to the scan waves.  (The
    // counts have an array of their own: cleared in one sweep, where a header word inside every 1 KiB chunk cost a cache
    // line per chunk -- 0.2 ms on a skewed index, whose raw buffer has grown -- and out of the way of k_replay_big, which
    // uses the raw buffer as scratch.)
    for (uint32_t k = g; k <= ws.cap_chunks; k += stride) ws.raw_used[k] = 0;
    if (g == 0) {
        Counters c{};
        c.raw_chunks = n_scan_waves;
        *ws.counters = c;
        ws.scan_span[2u * ws.span_slot] = ~0ull;
        ws.scan_span[2u * ws.span_slot + 1u] = 0ull;
    }
    __syncthreads();
    if (blockIdx.x * 256 < n)
        for (uint32_t b = threadIdx.x; b < n_buckets; b += 256)
            if (hist[b]) atomicAdd(&ws.ng[b], hist[b]);
}

// Start of cost range r of n_ranges (r == n_ranges: the end marker).
template <bool COOP = false>
__device__ __forceinline__ RangeStart range_start_of(const ScanItem *__restrict__ items, uint32_t n_items, uint64_t total,
                                                     uint32_t n_ranges, uint32_t r)
{
    RangeStart out;
    out.item = n_items;
    out.tile = 0;
    out.goff = 0;
    out.pad = 0;
    if (r < n_ranges) {
        // no 128-bit intermediate: costs < 2^50 and range counts <= 2^15
        const uint64_t lo = total / n_ranges * r + (total % n_ranges) * r / n_ranges;
        uint32_t a = 0, z = n_items; // last item with cost0 <= lo
        if (COOP) {
            // the whole wave looks for ONE range's start: 64 probes per round trip instead of one (a list of a million items: four
            // dependent loads instead of twenty -- the chain was most of k_fine_ranges' 7 - 12 us)
            const uint32_t lane = threadIdx.x & 63u;
            while (z - a > 1) {
                const uint32_t step = (z - a + 63u) / 64u;
                const uint64_t pos = static_cast<uint64_t>(a) + static_cast<uint64_t>(lane + 1u) * step;
                const bool le = pos < z && items[pos].cost0 <= lo;
                const uint32_t k = static_cast<uint32_t>(__popcll(__ballot(le))); // (costs ascend: the lanes that say yes are the first k)
                const uint64_t na = static_cast<uint64_t>(a) + static_cast<uint64_t>(k) * step, nz = na + step;
                a = static_cast<uint32_t>(na);
                if (nz < z) z = static_cast<uint32_t>(nz);
            }
        } else
        while (z - a > 1) {
            const uint32_t mid = (a + z) >> 1;
            if (items[mid].cost0 <= lo) a = mid; else z = mid;
        }
        // A unit of an item costs kTileFixedCost (fetching it) + shape / 8 per guide (kGuideCost for a full unit).  A
        // boundary may fall between two groups of 8 guides INSIDE a unit: then two waves share that unit (both fetch
        // it), which makes the ranges equal to within 8 guides instead of within one unit.
        const ScanItem it = items[a];
        const uint32_t len = it.g1 - it.g0;
        const uint32_t per_guide = it.shape >> 3;
        const uint64_t tile_cost = static_cast<uint64_t>(len) * per_guide + kTileFixedCost;
        const uint64_t rel = lo - it.cost0;
        uint64_t k = rel / tile_cost;
        const uint64_t rem = rel % tile_cost;
        uint32_t goff = 0;
        if (rem > kTileFixedCost) { // (inside the fetch part the unit starts the range: positions stay monotone in r)
            goff = ((static_cast<uint32_t>(rem - kTileFixedCost) + per_guide - 1u) / per_guide + kGuideGroup - 1u) & ~(kGuideGroup - 1u);
            if (goff >= len) { goff = 0; ++k; }
        }
        if (k >= it.n_tiles) { out.item = a + 1; out.tile = 0; out.goff = 0; }
        else { out.item = a; out.tile = static_cast<uint32_t>(k); out.goff = goff; }
    }
    return out;
}

// Scan workgroups that get a range of the plan: all of the launch's for a plan of any size, fewer for a small one -- a workgroup
// with less than a few units per wave is no faster, and every scan wave owns a record chunk that k_verify then has to visit
// (a 64-guide batch of 12 k units: 1024 workgroups = 16 384 nearly empty chunks were 25 us of its 130).  The record chunks
// [0, 16 x ranges) are the scan waves' own; what is handed out later comes behind them (Counters::raw_chunks).
__device__ __forceinline__ uint32_t ranges_for(uint64_t units, uint32_t scan_blocks)
{
    const uint64_t want = units / 64u + 1u; // ~4 units per wave
    const uint32_t floor_ = scan_blocks < 64u ? scan_blocks : 64u;
    return want >= scan_blocks ? scan_blocks : want < floor_ ? floor_ : static_cast<uint32_t>(want);
}

// One block: lay out the bucket-sorted guide arrays and the list of scan items.
__global__ __launch_bounds__(256) void k_plan(ImageView v, uint32_t *__restrict__ ng, uint32_t *__restrict__ gfill,
                                              uint32_t *__restrict__ gstart, ScanItem *__restrict__ items,
                                              uint32_t cap_items, PlanInfo *__restrict__ plan, uint32_t item_guides,
                                              uint32_t scan_blocks, Counters *__restrict__ counters)
{
    short_kernel_priority();
    __shared__ uint64_t lds[256];
    const uint32_t nb = v.n_buckets;
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = threadIdx.x * per;
    const uint32_t b1 = (b0 + per < nb) ? b0 + per : nb;

    uint64_t slots = 0, n_it = 0, cost = 0, cand = 0, wtiles = 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t g = ng[b];
        const uint32_t nt = v.tile_first[b + 1] - v.tile_first[b];
        slots += (g + kGuideGroup - 1u) / kGuideGroup * kGuideGroup;
        if (g && nt) {
            const uint32_t k = (g + item_guides - 1u) / item_guides;
            n_it += k;
            cost += static_cast<uint64_t>(nt) * (static_cast<uint64_t>(g) * kGuideCost + static_cast<uint64_t>(k) * kTileFixedCost);
            cand += (v.bucket_start[b + 1] - v.bucket_start[b]) * g;
            wtiles += static_cast<uint64_t>(nt) * k;
        }
    }
    uint64_t tot_slots, tot_items, tot_cost, tot_cand, tot_tiles;
    uint64_t slot_at = block_exclusive_scan(slots, lds, &tot_slots);
    uint64_t item_at = block_exclusive_scan(n_it, lds, &tot_items);
    uint64_t cost_at = block_exclusive_scan(cost, lds, &tot_cost);
    (void)block_exclusive_scan(cand, lds, &tot_cand);
    uint64_t tile_at = block_exclusive_scan(wtiles, lds, &tot_tiles);

    const bool overflow = tot_items > cap_items;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t g = ng[b];
        const uint32_t nt = v.tile_first[b + 1] - v.tile_first[b];
        gstart[b] = static_cast<uint32_t>(slot_at);
        if (g && nt && !overflow) {
            const uint64_t blen = v.bucket_start[b + 1] - v.bucket_start[b];
            for (uint32_t done = 0; done < g; done += item_guides) {
                const uint32_t len = (g - done < item_guides) ? g - done : item_guides;
                ScanItem it;
                it.bucket = b;
                it.g0 = static_cast<uint32_t>(slot_at) + done;
                it.g1 = it.g0 + len;
                it.n_tiles = nt;
                it.cost0 = cost_at;
                it.tile0 = static_cast<uint32_t>(tile_at);
                it.last_cands = static_cast<uint32_t>(blen - static_cast<uint64_t>(nt - 1u) * kTileCands);
                it.group_abs = v.tile_first[b] * 64u;
                it.window = it.last_cands << 16;
                it.shape = 32; it.gmid = 0;
                items[item_at++] = it;
                cost_at += static_cast<uint64_t>(nt) * (len * kGuideCost + kTileFixedCost);
                tile_at += nt;
            }
        }
        slot_at += (g + kGuideGroup - 1u) / kGuideGroup * kGuideGroup;
        ng[b] = 0;    // for the next batch's histogram
        gfill[b] = 0; // for this batch's scatter
    }
    if (threadIdx.x == 255) {
        gstart[nb] = static_cast<uint32_t>(tot_slots);
        if (!overflow) {
            ScanItem end;
            end.bucket = 0; end.g0 = 0; end.g1 = 0; end.n_tiles = 0; end.cost0 = tot_cost;
            end.tile0 = static_cast<uint32_t>(tot_tiles); end.last_cands = 0; end.group_abs = 0; end.window = 0;
            end.shape = 32; end.gmid = 0;
            items[tot_items] = end;
        }
        plan->n_items = overflow ? 0u : static_cast<uint32_t>(tot_items);
        plan->total_cost = overflow ? 0ull : tot_cost;
        plan->candidates = tot_cand;
        plan->reference_candidates = tot_cand;
        plan->fine = 0;
        plan->scan_tail = 0;
        plan->tiles = tot_tiles;
        // one equal-cost range per scan workgroup; inside a workgroup the waves share the tiles dynamically
        plan->n_ranges = (overflow || tot_tiles == 0) ? 0u : ranges_for(tot_tiles, scan_blocks);
        counters->raw_chunks = (plan->n_ranges ? plan->n_ranges : 1u) * 16u; // (k_guide_hist has reset the counters; k_fine_plan may choose again)
        plan->error = overflow ? 2u : 0u;
    }
}

// Scatter every guide into its bucket's range of (gword, gidx, gsig), once per slice.  (gsig: the guide's signature once
// more, in bucket order -- 8 bytes per pair, so that the two kernels of the pruned plan that walk a bucket's guides read it
// beside the index instead of behind it: guides[gidx[k]] was a chain of two round trips in each of them.)
__global__ __launch_bounds__(256) void k_guide_scatter(const uint64_t *__restrict__ guides, uint32_t n,
                                                       uint32_t slice_width, uint32_t n_slices, uint32_t sorted_layout,
                                                       uint32_t n_buckets, const uint32_t *__restrict__ gstart,
                                                       uint32_t *__restrict__ gfill, uint32_t *__restrict__ gword,
                                                       uint32_t *__restrict__ gidx, uint32_t *__restrict__ gbucket,
                                                       uint64_t *__restrict__ gsig,
                                                       uint32_t guide_blocks, const PlanInfo *__restrict__ plan,
                                                       const ScanItem *__restrict__ items,
                                                       RangeStart *__restrict__ starts)
{
    short_kernel_priority();
    if (blockIdx.x >= guide_blocks) {
        // the workgroups behind the guides resolve the cost ranges of the scan (independent of the scatter; one launch
        // less).  First tile of every range: range r owns the tiles whose start cost lies in [lo(r), lo(r+1)); done
        // once here so that the scan waves neither divide nor search.
        const uint32_t n_ranges = plan->n_ranges;
        const uint32_t r = (blockIdx.x - guide_blocks) * 256 + threadIdx.x;
        if (r <= n_ranges && n_ranges != 0) starts[r] = range_start_of(items, plan->n_items, plan->total_cost, n_ranges, r);
        return;
    }
    __shared__ uint32_t hist[kMaxBuckets];
    __shared__ uint32_t base[kMaxBuckets];
    for (uint32_t b = threadIdx.x; b < n_buckets; b += 256) hist[b] = 0;
    __syncthreads();
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t low = (1u << slice_width) - 1u;
    uint64_t sig = 0;
    uint32_t rank[kMaxSlices];
    if (g < n) {
        sig = guides[g];
#pragma unroll
        for (uint32_t s = 0; s < kMaxSlices; ++s) {
            if (s < n_slices) {
                const uint32_t key = static_cast<uint32_t>(sig >> (slice_width * s)) & low;
                rank[s] = atomicAdd(&hist[(s << slice_width) + key], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_buckets; b += 256)
        base[b] = hist[b] ? atomicAdd(&gfill[b], hist[b]) : 0u;
    __syncthreads();
    if (g < n) {
#pragma unroll
        for (uint32_t s = 0; s < kMaxSlices; ++s) {
            if (s < n_slices) {
                const uint32_t key = static_cast<uint32_t>(sig >> (slice_width * s)) & low;
                const uint32_t b = (s << slice_width) + key;
                const uint32_t slot = gstart[b] + base[b] + rank[s];
                gword[slot] = image_word(sig, s, slice_width, sorted_layout != 0u);
                gidx[slot] = g;
                gbucket[slot] = b;
                gsig[slot] = sig;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// pruned scan: guides grouped by (bucket, successor byte)
// ------------------------------------------------------------------------------------------------
// A site within max_dist <= 4 mismatches of a guide matches it exactly in some of the five slices (set E), and for at
// least one slice i of E the NEXT slice (i + 1 mod 5) has at most one mismatch: otherwise every slice of E is followed by
// a slice with >= 2 mismatches, these followers are distinct and lie outside E, the other slices outside E have >= 1
// each, and 2|E| + (5 - 2|E|) = 5 > 4 mismatches.  (For max_dist <= 2 the next slice is even exact for some i of E;
// both facts are checked by enumeration in tests/test_oracle_golden.py.)  With every bucket's candidates ordered by
// the byte of the successor slice, a guide therefore needs, in each of its five buckets, only the 13 groups whose
// successor byte is within one mismatch of its own (1 group for max_dist <= 2) instead of all 256 -- the reference
// scans the whole bucket, isslScoreOfftargets.cpp:344, and finds the same sites.  k_verify re-attributes a hit to the
// first exactly matching slice and its position there (pos_of), which is what the reference's order is made of.

// Units of one successor-byte group: its candidates [s0, s1) of the bucket's stream are covered from the group's first
// lane group (32 candidates) on by n_full full units of 2048 candidates and, for the `rest` behind them, one last unit of
// the smallest shape that holds it: 8, 16 or 32 candidates per lane (512 / 1024 / 2048 per unit).  In a short unit every
// plane register holds the lane's candidates 4 / 2 times over and one pass of the distance test serves 4 / 2 guides:
// the same comparisons per instruction as a full unit, a quarter / half of the idle lanes.
struct GroupUnits {
    uint32_t s0a, n_full, rest, shape, units;
};
__device__ __forceinline__ GroupUnits group_units(uint32_t s0, uint32_t s1, uint32_t tail_shapes)
{
    GroupUnits u;
    u.s0a = s0 & ~31u;
    const uint32_t span = s1 - u.s0a;
    u.n_full = span / kTileCands;
    u.rest = span - u.n_full * kTileCands;
    u.shape = (!tail_shapes || u.rest > 1024u) ? 32u : u.rest > 512u ? 16u : 8u;
    u.units = u.n_full + (u.rest ? 1u : 0u);
    return u;
}
// cost of the group's units against `len` guides (one chunk of at most item_guides of them)
__device__ __forceinline__ uint64_t group_cost(const GroupUnits &u, uint32_t len)
{
    return static_cast<uint64_t>(u.n_full) * (static_cast<uint64_t>(len) * kGuideCost + kTileFixedCost) +
           (u.rest ? static_cast<uint64_t>(len) * (u.shape >> 3) + kTileFixedCost : 0ull);
}

// The successor bytes a guide with successor byte `gj` visits: way 0 = gj itself, ways 1..12 = one position changed.
__device__ __forceinline__ uint32_t fine_way(uint32_t gj, uint32_t way)
{
    if (way == 0) return gj;
    if (way < kFineWays) {
        const uint32_t q = (way - 1u) / 3u, d = (way - 1u) % 3u + 1u;
        return gj ^ (d << (2u * q));
    }
    // ways 13..66 (max_dist 5): two of the four positions changed -- pair (a, b) of 6, bases (d1, d2) of 9
    const uint32_t w2 = way - kFineWays, pair = w2 / 9u, d1 = (w2 % 9u) / 3u + 1u, d2 = w2 % 3u + 1u;
    const uint32_t a = pair < 3u ? 0u : pair < 5u ? 1u : 2u;
    const uint32_t b = pair < 3u ? pair + 1u : pair < 5u ? pair - 1u : 3u;
    return gj ^ (d1 << (2u * a)) ^ (d2 << (2u * b));
}
// mismatches in the successor slice of a guide placed by `way`: 0, 1 or 2 -- the guide's class (fine_word)
__device__ __forceinline__ uint32_t fine_class(uint32_t way) { return way == 0u ? 0u : way < kFineWays ? 1u : 2u; }

__host__ __device__ __forceinline__ uint32_t fine_word(uint32_t word, uint32_t slice, uint32_t slice_width = 8u)
{
    const uint32_t lo = word & 0xFFFFu, hi = word >> 16;
    uint32_t lo12 = 0, hi12 = 0;
    for (uint32_t j = 0; j < 3u; ++j) {
        const uint32_t q = fine_order(slice, j, slice_width);
        lo12 |= ((lo >> (4u * q)) & 0xFu) << (4u * j);
        hi12 |= ((hi >> (4u * q)) & 0xFu) << (4u * j);
    }
    return lo12 | (hi12 << 12);
}

// Per bucket: guides per successor byte, and what the bucket's groups add to the plan.
template <uint32_t WAYS>
__global__ __launch_bounds__(256) void k_fine_count(ImageView v, const uint64_t *__restrict__ gsig,
                                                    const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ gfill,
                                                    uint32_t *__restrict__ fcount,
                                                    uint32_t *__restrict__ fcount0,
                                                    FineSum *__restrict__ fsum, uint32_t item_guides, uint32_t tail_shapes)
{
    constexpr uint32_t ways = WAYS; // compiled in: the 13 (or 67) LDS atomics of a guide are in flight together
    short_kernel_priority();
    __shared__ uint32_t cnt[256], cnt0[256];
    __shared__ uint64_t lds[256];
    const uint32_t b = blockIdx.x, slice = b >> v.slice_width;
    cnt[threadIdx.x] = 0;
    cnt0[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t g0 = gstart[b], n = gfill[b];
    for (uint32_t i = threadIdx.x; i < n; i += 256) { // one guide per thread and step: its load once, its ways from registers
        const uint32_t gj = succ_byte(gsig[g0 + i], slice, v.slice_width);
        atomicAdd(&cnt0[gj], 1u); // class 0: the guide's successor byte is the group's own (fine_class)
#pragma unroll
        for (uint32_t way = 0; way < ways; ++way) atomicAdd(&cnt[fine_way(gj, way)], 1u);
    }
    __syncthreads();
    const uint32_t w = threadIdx.x, c = cnt[w];
    const uint32_t *ss = v.sub_start + static_cast<uint64_t>(b) * 257u;
    const uint32_t s0 = ss[w], s1 = ss[w + 1];
    fcount[static_cast<uint64_t>(b) * 256u + w] = (s1 > s0) ? c : 0u; // a group without candidates takes no guides
    fcount0[static_cast<uint64_t>(b) * 256u + w] = (s1 > s0) ? cnt0[w] : 0u;
    uint64_t cost = 0, cand = 0, slots = 0, items = 0, units = 0;
    if (c && s1 > s0) {
        const GroupUnits gu = group_units(s0, s1, tail_shapes);
        const uint32_t kk = (c + item_guides - 1u) / item_guides;
        slots = (c + kGuideGroup - 1u) / kGuideGroup * kGuideGroup;
        units = static_cast<uint64_t>(gu.units) * kk;
        items = units; // one item per unit and chunk of guides: the scan finds the item of a unit without a search
        for (uint32_t done = 0; done < c; done += item_guides) cost += group_cost(gu, c - done < item_guides ? c - done : item_guides);
        cand = static_cast<uint64_t>(s1 - s0) * c;
    }
    uint64_t t_cost, t_cand, t_slots, t_items, t_units, t_places;
    (void)block_exclusive_scan(cost, lds, &t_cost);
    (void)block_exclusive_scan(cand, lds, &t_cand);
    (void)block_exclusive_scan(slots, lds, &t_slots);
    (void)block_exclusive_scan(items, lds, &t_items);
    (void)block_exclusive_scan(units, lds, &t_units);
    (void)block_exclusive_scan((c && s1 > s0) ? c : 0u, lds, &t_places);
    if (threadIdx.x == 0) {
        FineSum f;
        f.cost = t_cost; f.cand = t_cand; f.slots = static_cast<uint32_t>(t_slots); f.items = static_cast<uint32_t>(t_items);
        f.units = static_cast<uint32_t>(t_units); f.places = static_cast<uint32_t>(t_places);
        fsum[b] = f;
    }
}

// One block: exclusive prefix of the per-bucket totals (in place) and the plan of the pruned scan.
__global__ __launch_bounds__(256) void k_fine_plan(FineSum *__restrict__ fsum, uint32_t nb, ScanItem *__restrict__ fitems,
                                                   uint32_t cap_items, uint32_t cap_slots, PlanInfo *__restrict__ plan,
                                                   uint32_t scan_blocks, uint32_t prune_mode, uint32_t always,
                                                   uint32_t *__restrict__ sticky, Counters *__restrict__ counters)
{
    short_kernel_priority();
    __shared__ uint64_t lds[256];
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = threadIdx.x * per, b1 = (b0 + per < nb) ? b0 + per : nb;
    uint64_t cost = 0, cand = 0, slots = 0, items = 0, units = 0, places = 0;
    for (uint32_t b = b0; b < b1; ++b) {
        cost += fsum[b].cost; cand += fsum[b].cand; slots += fsum[b].slots; items += fsum[b].items; units += fsum[b].units;
        places += fsum[b].places;
    }
    uint64_t t_cost, t_cand, t_slots, t_items, t_units, t_places;
    (void)block_exclusive_scan(places, lds, &t_places);
    uint64_t cost_at = block_exclusive_scan(cost, lds, &t_cost);
    (void)block_exclusive_scan(cand, lds, &t_cand);
    uint64_t slot_at = block_exclusive_scan(slots, lds, &t_slots);
    uint64_t item_at = block_exclusive_scan(items, lds, &t_items);
    uint64_t unit_at = block_exclusive_scan(units, lds, &t_units);
    for (uint32_t b = b0; b < b1; ++b) {
        const FineSum f = fsum[b];
        FineSum at;
        at.cost = cost_at; at.cand = 0; at.slots = static_cast<uint32_t>(slot_at); at.items = static_cast<uint32_t>(item_at);
        at.units = static_cast<uint32_t>(unit_at); at.places = 0;
        fsum[b] = at;
        cost_at += f.cost; slot_at += f.slots; item_at += f.items; unit_at += f.units;
    }
    if (threadIdx.x == 255) {
        // Which plan is faster?  Comparing and fetching overlap: time ~ max((guide, tile) pairs, kFetchPairs x tile
        // fetches).  Few guides per successor-byte group make the pruned scan fetch-bound (every group reads its own
        // tiles, a bucket-level item reads a tile once for up to 512 guides); costs are pairs + kTileFixedCost x fetches.
        // (all in cost units: kGuideCost per pair of a guide with a full unit)
        const uint64_t fetch_cost = static_cast<uint64_t>(kFetchPairs) * kGuideCost;
        const uint64_t full_fetch = plan->tiles, full_pairs = plan->total_cost - kTileFixedCost * full_fetch;
        const uint64_t fine_pairs = t_cost - kTileFixedCost * t_units;
        const uint64_t est_full = full_pairs > fetch_cost * full_fetch ? full_pairs : fetch_cost * full_fetch;
        // (+ one comparison per place of a guide in a group: binning every guide 65 times is not free either)
        const uint64_t est_fine = (fine_pairs > fetch_cost * t_units ? fine_pairs : fetch_cost * t_units) + t_places * kGuideCost;
        const bool fits = t_items <= cap_items && t_slots <= cap_slots; // (the slots cover every guide in 13 groups)
        if (t_items > cap_items) // the host enlarges the item list for the next batches; this one scans whole buckets
            atomicMax(&sticky[3], static_cast<uint32_t>(t_items < 0xFFFFFFFFull ? t_items : 0xFFFFFFFFull));
        if (fits && plan->error == 0 && (always || est_fine < est_full)) {
            ScanItem end;
            end.bucket = 0; end.g0 = 0; end.g1 = 0; end.n_tiles = 0; end.cost0 = t_cost;
            end.tile0 = static_cast<uint32_t>(t_units); end.last_cands = 0; end.group_abs = 0; end.window = 0;
            end.shape = 32; end.gmid = 0;
            fitems[t_items] = end;
            plan->n_items = static_cast<uint32_t>(t_items);
            plan->total_cost = t_cost;
            plan->candidates = t_cand; // reference_candidates stays what the bucket-level plan counted
            plan->tiles = t_units;
            plan->n_ranges = t_units == 0 ? 0u : ranges_for(t_units, scan_blocks);
            counters->raw_chunks = (plan->n_ranges ? plan->n_ranges : 1u) * 16u;
            plan->fine = prune_mode;
            plan->fine_slots = static_cast<uint32_t>(t_slots);
            plan->scan_tail = t_cand >= kScanTailCands * 16ull * plan->n_ranges ? 1u : 0u; // (16 waves per range)
        }
    }
}

// Per bucket: the items of its successor-byte groups and the guides of every group in its slots -- two halves that need
// nothing from each other but the slot prefix of the bucket's groups, which each makes for itself from fcount: workgroups
// [0, nb) write the bucket's items, workgroups [nb, 2 nb) place its guides.  (One workgroup per bucket doing one after the
// other was a serial chain of dependent loads, the guides waiting for the last item.)  THREADS threads each, 512 or 256: with
// 512 the ~391 guides of a bucket of a 100 k batch are placed in one trip and its ~770 items staged in two; a batch with
// fewer guides per bucket than 256 takes the smaller workgroup (half the waves to launch for the same work).

// What an item needs to know of its group: worked out once by the group's thread, read from LDS by the items' threads
// (which found their group by a search, and had two dependent global loads and group_units behind that).
struct alignas(16) FineGroup {
    uint64_t cost0, chunk_cost; // cost in front of the group's first item; of a full chunk of item_guides guides
    uint32_t s0, s1, n_full, units;
    uint32_t shape, c, slot, slot0; // c guides in the slots from `slot` on, the class-0 ones from `slot0` on
};
template <uint32_t THREADS> struct FineItemLds {
    uint64_t scan[THREADS / 64u];
    uint32_t item0_of[257];
    FineGroup group[256];
    alignas(16) ScanItem stage[THREADS];
};
template <uint32_t THREADS> struct FineGuideLds {
    uint64_t scan[THREADS / 64u];
    uint32_t slot_of[256], slot0_of[256], cursor[256], cursor0[256], has_cands[256];
};
static_assert(sizeof(FineItemLds<512u>) <= 40u * 1024u, "four workgroups of k_fine_scatter per CU");

// (block_exclusive_scan serves the first 256 threads of a larger block too: the other waves add nothing and ignore what they get)
template <uint32_t THREADS>
__device__ __forceinline__ void fine_scatter_items(const ImageView &v, uint32_t b, const uint32_t *__restrict__ fcount,
                                                   const uint32_t *__restrict__ fcount0, const FineSum *__restrict__ fbase,
                                                   ScanItem *__restrict__ fitems, uint32_t item_guides, uint32_t tail_shapes,
                                                   FineItemLds<THREADS> &l)
{
    const uint32_t w = threadIdx.x;
    const FineSum base = fbase[b];
    const uint64_t blen = v.bucket_start[b + 1] - v.bucket_start[b];
    const uint32_t tile_first_b = v.tile_first[b];
    uint32_t c = 0, c1 = 0, s0 = 0, s1 = 0;
    if (w < 256u) {
        c = fcount[static_cast<uint64_t>(b) * 256u + w];
        c1 = c - fcount0[static_cast<uint64_t>(b) * 256u + w]; // class 1 first, class 0 behind it (fine_class)
        const uint32_t *ss = v.sub_start + static_cast<uint64_t>(b) * 257u;
        s0 = ss[w];
        s1 = ss[w + 1];
    }
    uint64_t cost = 0, slots = 0, items = 0;
    GroupUnits gu{};
    if (c) { // (fcount is zero where the group has no candidates)
        gu = group_units(s0, s1, tail_shapes);
        const uint32_t kk = (c + item_guides - 1u) / item_guides;
        slots = (c + kGuideGroup - 1u) / kGuideGroup * kGuideGroup;
        items = static_cast<uint64_t>(gu.units) * kk; // one item per unit and chunk of guides
        for (uint32_t done = 0; done < c; done += item_guides) cost += group_cost(gu, c - done < item_guides ? c - done : item_guides);
    }
    const uint64_t cost_at = base.cost + block_exclusive_scan(cost, l.scan, nullptr);
    const uint32_t slot_at = base.slots + static_cast<uint32_t>(block_exclusive_scan(slots, l.scan, nullptr));
    const uint32_t item_at = static_cast<uint32_t>(block_exclusive_scan(items, l.scan, nullptr)); // (inside the bucket)
    if (w < 256u) {
        l.item0_of[w] = item_at;
        if (w == 255u) l.item0_of[256] = item_at + static_cast<uint32_t>(items);
        FineGroup g;
        g.cost0 = cost_at; g.chunk_cost = group_cost(gu, item_guides);
        g.s0 = s0; g.s1 = s1; g.n_full = gu.n_full; g.units = gu.units;
        g.shape = gu.shape; g.c = c; g.slot = slot_at; g.slot0 = slot_at + c1;
        l.group[w] = g;
    }
    __syncthreads();
    // The bucket's items -- one per unit and chunk of guides, ~770 of 48 bytes -- are written by the whole workgroup, item i by
    // thread i % THREADS into a staging row in LDS and from there in 16-byte pieces that consecutive lanes put side by side:
    // every group's thread writing its own three items one after the other touched each 64-byte line of the list three times
    // from different lanes (four times the requests of the bytes moved).
    const uint32_t total = l.item0_of[256];
    for (uint32_t i0 = 0; i0 < total; i0 += THREADS) {
        const uint32_t i = i0 + w;
        if (i < total) {
            uint32_t lo = 0, hi = 256; // the group of item i: the last one whose first item is <= i (groups without items share a start)
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (l.item0_of[mid] <= i) lo = mid; else hi = mid;
            }
            const uint32_t gw = lo;
            const FineGroup g = l.group[gw];
            const uint32_t s0a = g.s0 & ~31u; // (group_units)
            const uint32_t j = i - l.item0_of[gw];
            const uint32_t chunk = j / g.units, t = j - chunk * g.units; // single-unit items: chunk after chunk, unit after unit
            const uint32_t done = chunk * item_guides;
            const uint32_t len = (g.c - done < item_guides) ? g.c - done : item_guides;
            const bool full = t < g.n_full;
            const uint32_t shape = full ? 32u : g.shape, cap = 64u * shape; // candidates the unit covers
            const uint32_t wstart = s0a + t * kTileCands;                  // position in the bucket (a lane group)
            const uint64_t after = blen - wstart;                          // candidates of the bucket from there on
            ScanItem it;
            it.bucket = (b << 8) | gw;
            it.g0 = g.slot + done; // item_guides is a multiple of 8
            it.g1 = it.g0 + len;
            it.n_tiles = 1;
            // the chunks in front of this one are full ones; the units in front of this one inside its chunk are full units
            it.cost0 = g.cost0 + static_cast<uint64_t>(chunk) * g.chunk_cost +
                       static_cast<uint64_t>(t) * (static_cast<uint64_t>(len) * kGuideCost + kTileFixedCost);
            it.tile0 = base.items + i;
            it.last_cands = after < cap ? static_cast<uint32_t>(after) : cap;
            it.group_abs = tile_first_b * 64u + (wstart >> 5);
            it.window = (t == 0 ? g.s0 - s0a : 0u) | ((g.s1 - wstart < cap ? g.s1 - wstart : cap) << 16);
            it.shape = shape; it.gmid = g.slot0;
            l.stage[w] = it;
        }
        __syncthreads();
        const uint32_t n_here = total - i0 < THREADS ? total - i0 : THREADS;
        const uint4 *src4 = reinterpret_cast<const uint4 *>(l.stage);
        uint4 *dst4 = reinterpret_cast<uint4 *>(fitems + base.items + i0);
        for (uint32_t q = w; q < n_here * 3u; q += THREADS) dst4[q] = src4[q];
        __syncthreads();
    }
}

template <uint32_t WAYS, uint32_t THREADS>
__device__ __forceinline__ void fine_scatter_guides(const ImageView &v, uint32_t b, const uint32_t *__restrict__ gstart,
                                                    const uint32_t *__restrict__ gfill, const uint32_t *__restrict__ gword,
                                                    const uint32_t *__restrict__ gidx, const uint64_t *__restrict__ gsig,
                                                    const uint32_t *__restrict__ fcount, const uint32_t *__restrict__ fcount0,
                                                    const FineSum *__restrict__ fbase, FineSlot *__restrict__ fword,
                                                    FineGuideLds<THREADS> &l)
{
    constexpr uint32_t ways = WAYS;
    const uint32_t w = threadIdx.x, slice = b >> v.slice_width;
    const uint32_t g0 = gstart[b], n = gfill[b];
    const uint32_t base_slots = fbase[b].slots;
    uint32_t c = 0, c1 = 0;
    if (w < 256u) {
        c = fcount[static_cast<uint64_t>(b) * 256u + w];
        c1 = c - fcount0[static_cast<uint64_t>(b) * 256u + w]; // class 1 first, class 0 behind it (fine_class)
    }
    // One guide per thread and step: its index, scan word and signature, side by side in bucket order, are on their way
    // while the prefix is made; its 13 (or 1) places come from registers and LDS.
    uint32_t i = w, guide = 0, word = 0;
    uint64_t sig = 0;
    if (i < n) { guide = gidx[g0 + i]; word = gword[g0 + i]; sig = gsig[g0 + i]; }
    const uint32_t slots = (c + kGuideGroup - 1u) / kGuideGroup * kGuideGroup;
    const uint32_t slot_at = base_slots + static_cast<uint32_t>(block_exclusive_scan(slots, l.scan, nullptr));
    if (w < 256u) {
        l.slot_of[w] = slot_at;
        l.slot0_of[w] = slot_at + c1;
        l.cursor[w] = 0;
        l.cursor0[w] = 0;
        // fcount is zero where the group has no candidates -- and nowhere else among the groups a guide of this bucket
        // visits: k_fine_count counted these very guides there
        l.has_cands[w] = c ? 1u : 0u;
        for (uint32_t k2 = c; k2 < slots; ++k2) fword[slot_at + k2] = FineSlot{kPadGuideWord, kPadSlotId}; // padding slots behind the group's guides
    }
    __syncthreads();
    while (i < n) {
        const uint32_t gj = succ_byte(sig, slice, v.slice_width);
        const uint32_t word12 = fine_word(word, slice, v.slice_width), id = slot_id(slice, guide);
#pragma unroll
        for (uint32_t way = 0; way < ways; ++way) {
            const uint32_t ww = fine_way(gj, way);
            if (!l.has_cands[ww]) continue; // no candidates there: the group has no slots
            const uint32_t slot = way ? l.slot_of[ww] + atomicAdd(&l.cursor[ww], 1u) : l.slot0_of[ww] + atomicAdd(&l.cursor0[ww], 1u);
            fword[slot] = FineSlot{word12 | (fine_class(way) << 24), id}; // one 8-byte store per placement
        }
        i += THREADS;
        if (i < n) { guide = gidx[g0 + i]; word = gword[g0 + i]; sig = gsig[g0 + i]; }
    }
}

template <uint32_t WAYS, uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void k_fine_scatter(ImageView v, const uint32_t *__restrict__ gstart,
                                                          const uint32_t *__restrict__ gfill, const uint32_t *__restrict__ gword,
                                                          const uint32_t *__restrict__ gidx, const uint64_t *__restrict__ gsig,
                                                          const uint32_t *__restrict__ fcount, const uint32_t *__restrict__ fcount0,
                                                          const FineSum *__restrict__ fbase, const PlanInfo *__restrict__ plan,
                                                          FineSlot *__restrict__ fword,
                                                          ScanItem *__restrict__ fitems, uint32_t item_guides, uint32_t tail_shapes)
{
    short_kernel_priority();
    if (!plan->fine) return; // the bucket-level plan stays
    __shared__ union { FineItemLds<THREADS> items; FineGuideLds<THREADS> guides; } lds;
    const uint32_t nb = v.n_buckets;
    if (blockIdx.x < nb) fine_scatter_items(v, blockIdx.x, fcount, fcount0, fbase, fitems, item_guides, tail_shapes, lds.items);
    else fine_scatter_guides<WAYS, THREADS>(v, blockIdx.x - nb, gstart, gfill, gword, gidx, gsig, fcount, fcount0, fbase, fword, lds.guides);
}

// Cost ranges of the pruned scan (the bucket-level ones are resolved by k_guide_scatter's last workgroups).
__global__ __launch_bounds__(256) void k_fine_ranges(const PlanInfo *__restrict__ plan, const ScanItem *__restrict__ fitems,
                                                     RangeStart *__restrict__ starts)
{
    short_kernel_priority();
    if (!plan->fine) return;
    const uint32_t n_ranges = plan->n_ranges;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); // one wave per range start
    if (r <= n_ranges && n_ranges != 0) {
        const RangeStart st = range_start_of<true>(fitems, plan->n_items, plan->total_cost, n_ranges, r);
        if ((threadIdx.x & 63u) == 0u) starts[r] = st;
    }
}

// ---- a small batch: the whole binning in ONE launch -------------------------------------------------------------------
// Seven dependent launches bin a batch (histogram, plan, scatter, group counts, group plan, group scatter, ranges); for a
// page of a few dozen guides they are 48 us of a 110 us step, and nearly all of that is launch boundaries and the chains of
// dependent loads behind each.  A batch of up to kSmallPairs (guide, slice) pairs (102 guides of five slices) is planned here
// without any grouping: EVERY (guide, slice, way) placement becomes a group of its own -- eight slots, the guide in the
// first --, so there is nothing to count, sort or scatter: one thread per (guide, slice) pair looks its 13 (or 1) groups up, a
// prefix sum over the pairs lays out slots, items and costs.  One workgroup PER WAY: each of them makes the whole prefix
// (loads that hit the L2) and writes the slots and items of its own way -- the stores of 4160 placements from one CU alone
// took 40 us.  Two guides that would have shared a group fetch its units twice; at this size that is nothing.  Same slots /
// items / plan as k_fine_* leave behind (k_fine_ranges follows); the bucket-level plan is not made (the host takes this path
// only where the pruned plan wins anyway: small_bin_ok).
constexpr uint32_t kSmallPairs = 512;

__device__ inline uint64_t block512_exclusive_scan(uint64_t v, uint64_t *lds /*[8]*/, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t incl = wave_inclusive_scan_u64(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t w = 0; w < kSmallPairs / 64u; ++w) {
        const uint64_t x = lds[w];
        if (w < wave) before += x;
        all += x;
    }
    if (total) *total = all;
    __syncthreads();
    return before + incl - v;
}

template <uint32_t WAYS>
__global__ __launch_bounds__(kSmallPairs) void k_bin_small(ImageView v, Workspace ws, const uint64_t *__restrict__ guides, uint32_t n,
                                                           uint32_t prune_mode, uint32_t tail_shapes, uint32_t scan_blocks,
                                                           uint32_t sorted_layout)
{
    short_kernel_priority();
    __shared__ uint64_t lds[kSmallPairs / 64u];
    const uint32_t t = threadIdx.x, my_way = blockIdx.x; // gridDim.x == WAYS
    // what k_guide_hist resets (shared out among the workgroups)
    for (uint32_t k = my_way * kSmallPairs + t; k <= n; k += WAYS * kSmallPairs) ws.gcount[k] = 0;
    for (uint32_t k = my_way * kSmallPairs + t; k <= ws.cap_chunks; k += WAYS * kSmallPairs) ws.raw_used[k] = 0;
    if (t == 0 && my_way == 0) {
        ws.scan_span[2u * ws.span_slot] = ~0ull;
        ws.scan_span[2u * ws.span_slot + 1u] = 0ull;
    }
    const uint32_t pairs = n * v.n_slices;
    const uint32_t low = (1u << v.slice_width) - 1u;
    const bool mine = t < pairs;
    const uint32_t g = mine ? t / v.n_slices : 0u, sl = mine ? t - g * v.n_slices : 0u;
    // the pair's bucket, its 13 (1) groups and what they add; pairs in thread order, ways in order = the order of slots and items
    uint64_t sig = 0, blen = 0, units = 0, cost = 0, cand = 0, ref = 0, valid = 0;
    uint64_t cost_before = 0;               // ... of the pair's ways in front of this workgroup's
    uint32_t units_before = 0, valid_before = 0;
    uint32_t b = 0, gj = 0, tf = 0, my_s0 = 0, my_s1 = 0;
    if (mine) {
        sig = guides[g];
        b = (sl << v.slice_width) + (static_cast<uint32_t>(sig >> (v.slice_width * sl)) & low);
        gj = succ_byte(sig, sl, v.slice_width);
        const uint32_t *ss = v.sub_start + static_cast<uint64_t>(b) * 257u;
        uint32_t s0[WAYS], s1[WAYS];
#pragma unroll
        for (uint32_t way = 0; way < WAYS; ++way) { // (all in flight together)
            const uint32_t ww = fine_way(gj, way);
            s0[way] = ss[ww];
            s1[way] = ss[ww + 1];
        }
        blen = v.bucket_start[b + 1] - v.bucket_start[b];
        tf = v.tile_first[b];
        ref = blen;
#pragma unroll
        for (uint32_t way = 0; way < WAYS; ++way) {
            if (way == my_way) { my_s0 = s0[way]; my_s1 = s1[way]; units_before = static_cast<uint32_t>(units); cost_before = cost; valid_before = static_cast<uint32_t>(valid); }
            if (s1[way] > s0[way]) {
                const GroupUnits gu = group_units(s0[way], s1[way], tail_shapes);
                units += gu.units;
                cost += group_cost(gu, 1u);
                cand += s1[way] - s0[way];
                ++valid;
            }
        }
    }
    uint64_t t_units, t_cost, t_cand, t_ref, t_valid;
    uint32_t item_at = static_cast<uint32_t>(block512_exclusive_scan(units, lds, &t_units)) + units_before;
    uint64_t cost_at = block512_exclusive_scan(cost, lds, &t_cost) + cost_before;
    (void)block512_exclusive_scan(cand, lds, &t_cand);
    (void)block512_exclusive_scan(ref, lds, &t_ref);
    const uint32_t slot_at = (static_cast<uint32_t>(block512_exclusive_scan(valid, lds, &t_valid)) + valid_before) * kGuideGroup;
    const uint64_t t_slots = t_valid * kGuideGroup;
    const bool overflow = t_units > ws.cap_fitems || t_slots > ws.cap_fslots;
    // slots and items of this workgroup's way of every pair
    if (mine && !overflow && my_s1 > my_s0) {
        const uint32_t way = my_way, s0 = my_s0, s1 = my_s1;
        const uint32_t word12 = fine_word(image_word(sig, sl, v.slice_width, sorted_layout != 0u), sl, v.slice_width);
        const uint32_t ww = fine_way(gj, way);
        const uint32_t c1 = way ? 1u : 0u; // a group's class-1 guides come first, its class-0 guides from gmid on: here ONE guide
        uint4 *fw = reinterpret_cast<uint4 *>(ws.fword + slot_at); // (slot_at is a multiple of 8: 64-byte aligned)
        fw[0] = make_uint4(word12 | (fine_class(way) << 24), slot_id(sl, g), kPadGuideWord, kPadSlotId);
#pragma unroll
        for (uint32_t k2 = 1; k2 < kGuideGroup / 2u; ++k2) fw[k2] = make_uint4(kPadGuideWord, kPadSlotId, kPadGuideWord, kPadSlotId);
        const GroupUnits gu = group_units(s0, s1, tail_shapes);
        for (uint32_t u = 0; u < gu.units; ++u) { // as k_fine_scatter lays a group's units out, for one guide
            const bool full = u < gu.n_full;
            const uint32_t shape = full ? 32u : gu.shape, cap = 64u * shape;
            const uint32_t wstart = gu.s0a + u * kTileCands;
            const uint64_t after = blen - wstart;
            ScanItem it;
            it.bucket = (b << 8) | ww;
            it.g0 = slot_at;
            it.g1 = slot_at + 1u;
            it.n_tiles = 1;
            it.cost0 = cost_at;
            it.tile0 = item_at;
            it.last_cands = after < cap ? static_cast<uint32_t>(after) : cap;
            it.group_abs = tf * 64u + (wstart >> 5);
            it.window = (u == 0 ? s0 - gu.s0a : 0u) | ((s1 - wstart < cap ? s1 - wstart : cap) << 16);
            it.shape = shape; it.gmid = slot_at + c1;
            ws.fitems[item_at++] = it;
            cost_at += static_cast<uint64_t>(shape >> 3) + kTileFixedCost;
        }
    }
    if (t == 0 && my_way == 0) {
        const uint32_t n_items = overflow ? 0u : static_cast<uint32_t>(t_units);
        ScanItem end;
        end.bucket = 0; end.g0 = 0; end.g1 = 0; end.n_tiles = 0; end.cost0 = overflow ? 0ull : t_cost;
        end.tile0 = n_items; end.last_cands = 0; end.group_abs = 0; end.window = 0; end.shape = 32; end.gmid = 0;
        ws.fitems[n_items] = end;
        PlanInfo pl{};
        pl.n_items = n_items;
        pl.error = 0;
        pl.n_ranges = n_items == 0 ? 0u : ranges_for(t_units, scan_blocks);
        pl.fine = prune_mode;
        pl.total_cost = overflow ? 0ull : t_cost;
        pl.candidates = overflow ? 0ull : t_cand;
        pl.reference_candidates = t_ref;
        pl.tiles = n_items;
        pl.fine_slots = overflow ? 0u : static_cast<uint32_t>(t_slots);
        *ws.plan = pl;
        Counters c{};
        c.raw_chunks = (pl.n_ranges ? pl.n_ranges : 1u) * 16u;
        *ws.counters = c;
        if (overflow) { // room for the next try (finish_batches enlarges the item list), and this batch once more
            atomicMax(&ws.sticky[3], static_cast<uint32_t>(t_units < 0xFFFFFFFFull ? t_units : 0xFFFFFFFFull));
            atomicOr(&ws.sticky[0], 2u);
        }
    }
}

// The one-launch binning where it is safe and pays: a sorted image (the pruned plan exists), at most kSmallPairs
// (guide, slice) pairs, 13 ways or 1 (max_dist <= 4), and an index on which the pruned plan beats the bucket-level one for a lone
// guide anyway -- its buckets hold more units than the 13 groups a guide visits (k_fine_plan's estimate, taken for the mean
// bucket) -- or a caller who asked for the pruned plan always (prune = 1).
static bool small_bin_ok(const ImageView &v, const Workspace &ws, const Tuning &tn, uint32_t n, uint32_t prune_mode)
{
    if (!tn.small_bin || (prune_mode != 1u && prune_mode != 2u) || !ws.fitems || !v.sub_start) return false;
    if (n == 0 || static_cast<uint64_t>(n) * v.n_slices > kSmallPairs) return false;
    const uint64_t buckets_per_slice = 1ull << v.slice_width;
    return tn.prune == 1 || v.n_sites / buckets_per_slice >= 16ull * kTileCands;
}

uint32_t prune_mode_for(const ImageView &v, const Tuning &tn, uint32_t n_guides, int max_dist)
{
    const bool geometry = v.n_slices * v.slice_width == 40u && (v.slice_width == 8 || v.slice_width == 4 || v.slice_width == 2); // succ_byte
    if ((!v.srec && !v.sid) || tn.prune == 0 || max_dist < 0 || max_dist > 5 || !geometry) return 0;
    if (n_guides > prune_max_guides(max_dist == 5 ? 3u : 2u, v.n_slices)) return 0;
    // max_dist 5: a hit the reference can find matches some slice exactly (:330-344 walks the buckets of the guide's own
    // slice values), and then some exact slice is followed by one with at most TWO mismatches (the cycle lemma of the
    // comment above with 3 |E| + (5 - 2 |E|) > 5): 67 of a bucket's 256 groups instead of all of them.
    return max_dist <= 2 ? 1u : max_dist <= 4 ? 2u : 3u;
}

void launch_bin_guides(const ImageView &v, const Workspace &ws, const Tuning &tn, const uint64_t *d_guides, uint32_t n,
                       uint32_t prune_mode, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t nb = v.n_buckets;
    if (small_bin_ok(v, ws, tn, n, prune_mode)) { // two launches instead of seven
        const uint32_t sorted = (v.srec || v.sid) ? 1u : 0u;
        if (fine_ways_of(prune_mode) == 1u)
            hipLaunchKernelGGL(k_bin_small<1u>, dim3(1), dim3(kSmallPairs), 0, stream, v, ws, d_guides, n, prune_mode,
                               static_cast<uint32_t>(tn.tail_shapes), tn.scan_blocks, sorted);
        else
            hipLaunchKernelGGL(k_bin_small<kFineWays>, dim3(kFineWays), dim3(kSmallPairs), 0, stream, v, ws, d_guides, n, prune_mode,
                               static_cast<uint32_t>(tn.tail_shapes), tn.scan_blocks, sorted);
        hipLaunchKernelGGL(k_fine_ranges, dim3((tn.scan_blocks + 1u + 3u) / 4u), dim3(256), 0, stream, ws.plan, ws.fitems, ws.range_start);
        return;
    }
    // slots in use: 8-padded guides per bucket, at most n * slices + 8 * buckets
    const uint32_t n_slots = static_cast<uint32_t>(
        std::min<size_t>(ws.cap_gslots, static_cast<size_t>(n) * v.n_slices + static_cast<size_t>(kGuideGroup) * nb));
    // three launches: histogram (+ resets), plan, scatter (+ ranges)
    const uint32_t blocks = (n + 255u) / 256u;
    const uint32_t reset_blocks = std::min<uint32_t>(1024u, (std::max(n_slots, nb) + 255u) / 256u);
    hipLaunchKernelGGL(k_guide_hist, dim3(std::max(blocks, reset_blocks)), dim3(256), 0, stream, ws, d_guides, n,
                       v.slice_width, v.n_slices, nb, n_slots, tn.scan_blocks * 16u);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(256), 0, stream, v, ws.ng, ws.gfill, ws.gstart, ws.items,
                       static_cast<uint32_t>(ws.cap_items), ws.plan, tn.item_guides, tn.scan_blocks, ws.counters);
    const uint32_t range_blocks = (tn.scan_blocks + 1u + 255u) / 256u;
    hipLaunchKernelGGL(k_guide_scatter, dim3(blocks + range_blocks), dim3(256), 0, stream, d_guides, n, v.slice_width,
                       v.n_slices, (v.srec || v.sid) ? 1u : 0u, nb, ws.gstart, ws.gfill, ws.gword, ws.gidx, ws.gbucket, ws.gsig, blocks, ws.plan, ws.items,
                       ws.range_start);
    if (prune_mode) { // regroup by (bucket, successor byte); k_fine_plan decides which of the two plans the scan follows
        const uint32_t ways = fine_ways_of(prune_mode);
        // (max_dist 5: three classes of guides in a pass -- the class plane of the short units has weight one only)
        const uint32_t tail_shapes = prune_mode == 3 ? 0u : static_cast<uint32_t>(tn.tail_shapes);
        auto launch_fine = [&](auto ways_tag) {
            constexpr uint32_t W = decltype(ways_tag)::value;
            hipLaunchKernelGGL(k_fine_count<W>, dim3(nb), dim3(256), 0, stream, v, ws.gsig, ws.gstart, ws.gfill, ws.fcount,
                               ws.fcount0, ws.fsum, tn.item_guides, tail_shapes);
            hipLaunchKernelGGL(k_fine_plan, dim3(1), dim3(256), 0, stream, ws.fsum, nb, ws.fitems,
                               static_cast<uint32_t>(ws.cap_fitems), static_cast<uint32_t>(ws.cap_fslots), ws.plan, tn.scan_blocks,
                               prune_mode, tn.prune == 1 ? 1u : 0u, ws.sticky, ws.counters);
            // (the workgroup size from the mean bucket: 391 guides at 100 k guides of five slices over 1280 buckets)
            if (static_cast<uint64_t>(n) * v.n_slices > 256ull * nb)
                hipLaunchKernelGGL((k_fine_scatter<W, 512u>), dim3(2u * nb), dim3(512), 0, stream, v, ws.gstart, ws.gfill, ws.gword, ws.gidx, ws.gsig,
                                   ws.fcount, ws.fcount0, ws.fsum, ws.plan, ws.fword, ws.fitems, tn.item_guides, tail_shapes);
            else
                hipLaunchKernelGGL((k_fine_scatter<W, 256u>), dim3(2u * nb), dim3(256), 0, stream, v, ws.gstart, ws.gfill, ws.gword, ws.gidx, ws.gsig,
                                   ws.fcount, ws.fcount0, ws.fsum, ws.plan, ws.fword, ws.fitems, tn.item_guides, tail_shapes);
        };
        if (ways == 1u) launch_fine(std::integral_constant<uint32_t, 1u>{});
        else if (ways == kFineWays) launch_fine(std::integral_constant<uint32_t, kFineWays>{});
        else launch_fine(std::integral_constant<uint32_t, kFineWays2>{});
        hipLaunchKernelGGL(k_fine_ranges, dim3((tn.scan_blocks + 1u + 3u) / 4u), dim3(256), 0, stream, ws.plan, ws.fitems, ws.range_start);
    }
}

} // namespace issl
