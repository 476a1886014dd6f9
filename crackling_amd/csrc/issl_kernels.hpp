// Device code that more than one pipeline stage uses: the scan word and tile layout, candidate_signature, the block
// scans, the sizes the scoring tail's stages agree on, and the MIT / CFD terms of a hit.  Included by the .hip files
// only; every one of them is a translation unit of its own (no relocatable device code), so everything here is inline.
#pragma once
#include <hip/hip_runtime.h>

#include "issl_device.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// bit helpers
// ------------------------------------------------------------------------------------------------

// The short kernels around the scan raise their wave priority: when they share the GPU with a scan (two lanes),
// they are latency-bound and few, and should not queue behind the scan's older waves.
__device__ __forceinline__ void short_kernel_priority() { __builtin_amdgcn_s_setprio(3); }

// Even bits of a 32-bit word gathered into the low 16 bits.
__host__ __device__ inline uint32_t gather_even16(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// Scan word of a 20 bp signature for slice `s` (8-bit slices): drop the slice's own byte (it is
// equal for every candidate and guide of the bucket), then split the remaining 16 positions into
// low-bit plane (bits 0..15) and high-bit plane (bits 16..31).  Two words differ at position p
// iff bit p of (x | x>>16) is set, x = a ^ b.
// Narrower slices (width 4 / 2: the reference scorer takes any width, :261-270,330-341) leave 18 / 19 other positions:
// the scan word keeps the first 16 of them, so the scan's count is a lower bound of the distance there -- it notes a
// superset of the hits and k_verify's exact test on the whole signatures decides, as it does anyway.
__host__ __device__ inline uint32_t scan_word(uint64_t sig, uint32_t s, uint32_t width = 8u)
{
    const uint32_t sh = width * s;
    const uint64_t low = sig & ((1ull << sh) - 1ull);
    const uint64_t high = (sig >> (sh + width)) << sh;
    const uint32_t rem = static_cast<uint32_t>(low | high);
    return gather_even16(rem) | (gather_even16(rem >> 1) << 16);
}

// Narrow slices on a SORTED layout (round 4; ten 4-bit or twenty 2-bit slices): the word's first quad holds the four
// positions of the successor unit (the next two / four slices: one byte, the same for every candidate of a successor-byte
// group, so the pruned scan leaves that quad in memory as it does with 8-bit slices), then the previous slice's two / one
// (fine_dup), then the ten / eleven positions that follow the successor unit; the last two / three before the previous slice
// are left out -- the count is a lower bound, k_verify decides.
__host__ __device__ inline uint32_t scan_word_sorted_narrow(uint64_t sig, uint32_t s, uint32_t width)
{
    const uint32_t sh = (width * (s + 1u)) % 40u;
    const uint64_t x = sig & kSigMask;
    const uint64_t a = (sh ? (x >> sh) | (x << (40u - sh)) : x) & kSigMask; // slices s + 1, s + 2, ... , s - 1, s from bit 0 on
    const uint64_t prev = (a >> (40u - 2u * width)) & ((1ull << width) - 1ull);
    const uint64_t mid = (a >> 8) & ((1ull << (24u - width)) - 1ull);
    const uint32_t rem = static_cast<uint32_t>((a & 0xFFull) | (prev << 8) | (mid << (8u + width)));
    return gather_even16(rem) | (gather_even16(rem >> 1) << 16);
}
// The word of a signature in slice s as the image's stream holds it (guides are packed the same way).
__host__ __device__ inline uint32_t image_word(uint64_t sig, uint32_t s, uint32_t width, bool sorted_layout)
{
    return (sorted_layout && width < 8u) ? scan_word_sorted_narrow(sig, s, width) : scan_word(sig, s, width);
}

// Mismatch flags of two packed signatures, one flag at bit 2p (isslScoreOfftargets.cpp:376-379).
__host__ __device__ inline uint64_t mismatch_mask(uint64_t a, uint64_t b)
{
    const uint64_t x = a ^ b;
    return ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | (x & 0x5555555555555555ull);
}

// Bit-sliced tile layout.  A tile holds 2048 candidates = 64 groups of 32.  Group G is owned by lane G of
// the scanning wave and consists of 32 PLANES: plane r < 16 holds, for its 32 candidates (bit j =
// candidate at tile offset 32 G + j), the low bit of the 2-bit code at position r of the scan word;
// plane 16 + r the high bit.  The word of (plane r, group G) sits at index ((r / 4) * 64 + G) * 4 + r % 4,
// so the scanning wave fetches its 32 planes with 8 coalesced 16-byte loads per lane.
constexpr int kPlanes = 32; // planes per lane = VGPRs holding the lane's 32 candidates

__host__ __device__ inline uint32_t plane_word(uint32_t r, uint32_t group)
{
    return ((r >> 2) * 64u + group) * 4u + (r & 3u);
}

// The packed signature of the candidate at offset `offset` of scan tile `tile` of bucket `bucket`, rebuilt from the
// scan stream: bit (offset % 32) of the 32 plane words of its group gives the 16 remaining positions (inverse of
// scan_word), the bucket number gives the slice's own byte.  8 loads of 16 B -- HBM, where the site table may be in
// host memory.
__device__ inline uint64_t candidate_signature(const ImageView &v, uint32_t bucket, uint32_t tile, uint32_t offset)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(v.scan + static_cast<uint64_t>(tile) * kTileCands);
    const uint32_t group = offset >> 5, bit = offset & 31u;
    uint32_t w = 0; // plane r of the candidate at bit r: bits 0..15 = low code bits of the 16 positions, 16..31 = high bits
#pragma unroll
    for (uint32_t q = 0; q < kPlanes / 4; ++q) {
        const uint4 t4 = src[q * 64u + group];
        w |= ((t4.x >> bit) & 1u) << (4 * q) | ((t4.y >> bit) & 1u) << (4 * q + 1) | ((t4.z >> bit) & 1u) << (4 * q + 2) |
             ((t4.w >> bit) & 1u) << (4 * q + 3);
    }
    uint64_t rem = 0; // 16 positions x 2 bits: low bit of position p at bit 2p, high bit at 2p + 1
#pragma unroll
    for (uint32_t p = 0; p < 16; ++p)
        rem |= static_cast<uint64_t>(((w >> p) & 1u) | (((w >> (16 + p)) & 1u) << 1)) << (2 * p);
    const uint32_t slice = bucket >> v.slice_width;
    const uint32_t sh = v.slice_width * slice;
    const uint64_t key = bucket & ((1u << v.slice_width) - 1u);
    return (rem & ((1ull << sh) - 1ull)) | (key << sh) | ((rem >> sh) << (sh + v.slice_width));
}

// Exclusive scan of one uint64 per thread over a 256-thread block: shuffles inside the four waves, one LDS
// exchange across them (two barriers instead of the seventeen of a Hillis-Steele scan through LDS).
__device__ inline uint64_t wave_inclusive_scan_u64(uint64_t x)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up(static_cast<uint32_t>(x), d, 64);
        const uint32_t hi = __shfl_up(static_cast<uint32_t>(x >> 32), d, 64);
        if (lane >= d) x += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return x;
}

__device__ inline uint64_t block_exclusive_scan(uint64_t v, uint64_t *lds /*[256], 4 used*/, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t incl = wave_inclusive_scan_u64(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t w = 0; w < 4; ++w) {
        const uint64_t s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    if (total) *total = all;
    __syncthreads();
    return before + incl - v;
}

// The pruned scan compares 12 positions, not 16.  An item of its plan is ONE (bucket, successor byte) group: inside the
// item's window every candidate carries the same four bases in the successor slice, and how far a guide is from them is
// known when the guide is placed -- 0 mismatches in its own group (way 0, "class 0"), 1 in the twelve others (ways 1..12,
// "class 1").  The scan therefore leaves the successor slice's planes in memory (two of the eight 16-byte loads per lane,
// scan_word: positions 4 s' .. 4 s' + 3 of the 16, s' = fine_quad(slice)) and counts the other 12 positions against
// max_dist - class; the reference's test :376-382 on the full signatures is k_verify's.  Guide word of the pruned plan:
// bits 0..11 the low code bits of the 12 positions (fine_order), bits 12..23 the high ones, bits 24..25 the class.
// A group's slots hold its class-1 guides first (from a multiple of 8 on), its class-0 guides behind them from
// ScanItem::gmid on: full units run the two classes as two loops with their own compiled tests, short units take the
// class bit as a thirteenth plane.
__host__ __device__ __forceinline__ constexpr uint32_t fine_quad(uint32_t slice) { return slice < 4u ? slice : 0u; }
// The order of the 12 positions (three quads of the scan word's four): the quad of the PREVIOUS slice (slice - 1) first --
// its four mismatch planes tell, for nothing, whether the slice before the bucket's own matches the guide exactly too, and
// a candidate for which it does is reported from that slice's bucket already (fine_dup) -- then the other two, ascending.
// Slice 0 has no previous slice: its quads in ascending order.  (Quad q of slice s's scan word holds slice q < s ? q : q + 1.)
// Narrow slices (scan_word_sorted_narrow): the successor unit is quad 0 for every slice, the previous slice opens quad 1: quads 1, 2, 3.
__host__ __device__ __forceinline__ constexpr uint32_t fine_order(uint32_t slice, uint32_t j, uint32_t slice_width = 8u)
{
    if (slice_width != 8u) return j + 1u;
    const uint32_t sq = fine_quad(slice);
    if (slice == 0u) return j + 1u;                                // quads 1, 2, 3
    const uint32_t prev = slice - 1u;                              // slice - 1 sits in quad slice - 1 (it is below the own slice)
    if (j == 0u) return prev;
    uint32_t q = 0, seen = 0;                                      // the j-th of the quads that are neither sq nor prev
    for (; q < 4u; ++q) {
        if (q == sq || q == prev) continue;
        if (++seen == j) break;
    }
    return q;
}

// Workgroups of the two passes over the raw chunks (one chunk per workgroup and step): enough of them that the
// ~16 k first chunks of the scan waves are all in flight at once -- the passes are chains of dependent loads.
constexpr uint32_t kTailGrid = 16384;
constexpr uint32_t kReplayLds = 512;  // guides with up to this many hits: one wave each (k_replay)
static_assert(kReplayLds <= 512, "k_replay sorts (key, 9-bit index) pairs");
constexpr uint32_t kMidHits = 2048;   // ... up to this many: one 256-thread workgroup each (k_replay_mid), terms from k_verify;
                                      // beyond: k_replay_big (1024 threads, slice by slice, terms worked out as it walks)

constexpr uint32_t kScanChunk = 2048; // elements per block in the device-wide prefix sum
constexpr uint32_t kBigLds = 7680;    // hits per slice k_replay_big sorts in LDS (2 x 30 KiB); longer slices are sorted in HBM

// What a guide's hits take in the grouped arrays: nothing when they all sit in its hit slots (Workspace::slot_hits).
// (with slots of any width every guide of the many-hit replays keeps a segment for ALL its hits: k_replay_big copies the keys in
// the slots in front of the rest, and k_replay_mid may hand a guide on to it)
__device__ __forceinline__ uint32_t grouped_hits(uint32_t count, uint32_t slot_hits)
{
    return count <= (slot_hits ? kSlotHits : 0u) ? 0u : count;
}

// CFD penalty tables (cfdPenalties.h:1-346) live in the code object's constant segment.
// (inline variables: every unit that scores carries its own copy on the device, the host links one shadow.  `static` would
// let the compiler fold the entries it can see into the code.)
#define ISSL_CFD_QUAL inline __constant__
#include "cfd_tables.inc"

// precalculatedScores[mask] with operator[] semantics: a missing mask contributes 0.0 (:394).
// Reference-built tables hold masks with flags on even bits below bit 40 only; for those the image carries a
// dense 2^20-entry table indexed by the 20 flags (one load instead of a 13-step search).
// (View: ImageView, or the one in k_scan's kernel arguments -- VerifyCtx, KernargCtx.)
template <class View>
__device__ inline double mit_lookup(const View &v, uint64_t mask)
{
    if (v.mit_dense) {
        if (mask >> 40) return 0.0;
        const uint32_t idx = gather_even16(static_cast<uint32_t>(mask)) |
                             (gather_even16(static_cast<uint32_t>(mask >> 32)) << 16);
        return v.mit_dense[idx];
    }
    uint32_t lo = 0, hi = v.n_scores;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t m = v.score_mask[mid];
        if (m == mask) return v.score_val[mid];
        if (m < mask) lo = mid + 1; else hi = mid;
    }
    return 0.0;
}

// MIT and CFD terms of one scored off-target (isslScoreOfftargets.cpp:392-460) from the two signatures and the
// occurrence count.  The CFD product multiplies the penalties of the mismatching positions in position order, as the
// reference's loop over all 20 positions does (:399-460); the walk over the set flags visits the same positions.
template <class View>
__device__ inline void score_terms(const View &v, uint64_t gsig, uint64_t ot, uint32_t occ, bool calc_mit, bool calc_cfd,
                                   double &mit_term, double &cfd_term, int &dist_out)
{
    mit_term = 0.0;
    cfd_term = 0.0;
    const uint64_t mm = mismatch_mask(gsig, ot);
    const int dist = __builtin_popcountll(mm);
    dist_out = dist;
    if (calc_mit && dist > 0) mit_term = mit_lookup(v, mm) * static_cast<double>(occ); // :394
    if (calc_cfd) {                                                                    // :399-460
        double cfd;
        if (dist == 0) {
            cfd = 1.0;
        } else {
            cfd = issl_cfd_pam[10];
            for (uint64_t left = mm; left != 0ull; left &= left - 1ull) { // the mismatching positions, ascending (<= max_dist)
                const uint32_t q = static_cast<uint32_t>(__builtin_ctzll(left)) >> 1;
                const uint32_t gb = static_cast<uint32_t>(gsig >> (2 * q)) & 3u;
                const uint32_t ob = static_cast<uint32_t>(ot >> (2 * q)) & 3u;
                cfd *= issl_cfd_pos[(q << 4) | (gb << 2) | (ob ^ 3u)];
            }
        }
        cfd_term = cfd * static_cast<double>(occ);
    }
}

// MIT and CFD terms of one scored off-target (isslScoreOfftargets.cpp:392-460) and its record.
struct HitTerms {
    double mit, cfd;
    issl_hit rec;
};

__device__ inline HitTerms hit_terms(const ImageView &v, uint64_t gsig, uint32_t g, uint64_t key, bool calc_mit,
                                     bool calc_cfd, bool want_id)
{
    HitTerms t;
    t.mit = 0.0;
    t.cfd = 0.0;
    const uint64_t low = (1ull << v.slice_width) - 1ull;
    const uint32_t slice = static_cast<uint32_t>(key >> kKeySliceShift) & kKeySliceMask;
    uint32_t pos = static_cast<uint32_t>(key);
    const uint32_t bucket = (slice << v.slice_width) + static_cast<uint32_t>((gsig >> (v.slice_width * slice)) & low);
    const uint64_t at = v.bucket_start[bucket] + pos;
    uint32_t id = 0, occ;
    uint64_t ot;
    if (v.srec || v.sid) {
        // sorted layouts: the key's low word is the site id; issl_dump_hits also wants the position in the bucket's list
        // (:344): the lists ascend by id, so a binary search finds it (in host memory when the lists live there)
        id = pos;
        const uint64_t site = v.sites[id]; // signature | min(count, kOccSaturated) << 40 (k_tag_sites)
        ot = site & kSigMask;
        occ = static_cast<uint32_t>(site >> 40);
        if (occ == kOccSaturated) occ = v.site_occ[id];
        pos = 0;
        if (want_id && v.entries) {
            const uint64_t *list = v.entries + v.bucket_start[bucket];
            uint64_t lo = 0, hi = v.bucket_start[bucket + 1] - v.bucket_start[bucket];
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (static_cast<uint32_t>(list[mid]) < id) lo = mid + 1; else hi = mid;
            }
            pos = static_cast<uint32_t>(lo);
        } else if (want_id) {
            // An image without slice lists (ImageHeader::lists_absent): the position in the bucket's list is the number of
            // the bucket's sites with a smaller id.  The stream holds the bucket's ids, ascending inside each of its 256
            // successor-byte groups: one binary search per group.
            const uint32_t *ss = v.sub_start + static_cast<uint64_t>(bucket) * 257u;
            const uint64_t first = static_cast<uint64_t>(v.tile_first[bucket]) * kTileCands;
            for (uint32_t w = 0; w < 256u; ++w) {
                uint32_t lo = ss[w], hi = ss[w + 1];
                const uint32_t s0 = lo;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    const uint32_t there = v.srec ? v.srec[first + mid].id : v.sid[first + mid];
                    if (there < id) lo = mid + 1; else hi = mid;
                }
                pos += lo - s0;
            }
        }
    } else if (v.occ8) {
        // cold sections in host memory: signature from the scan planes, occurrences from the byte copy in HBM; the list
        // entry itself (PCIe) only for counts that do not fit a byte and for the site id of issl_dump_hits
        ot = candidate_signature(v, bucket, v.tile_first[bucket] + (pos >> 11), pos & (kTileCands - 1u));
        occ = v.occ8[at];
        if (occ == 255u || want_id) {
            const uint64_t e = v.entries[at];
            id = static_cast<uint32_t>(e);
            occ = static_cast<uint32_t>(e >> 32);
        }
    } else {
        const uint64_t e = v.entries[at];
        id = static_cast<uint32_t>(e);
        occ = static_cast<uint32_t>(e >> 32);
        ot = v.esig ? v.esig[at] : v.sites[id]; // independent of `e` when the in-list copy exists
    }
    int dist;
    score_terms(v, gsig, ot, occ, calc_mit, calc_cfd, t.mit, t.cfd, dist);
    t.rec.guide = g; t.rec.slice = slice; t.rec.pos = pos; t.rec.id = id;
    t.rec.dist = static_cast<uint32_t>(dist); t.rec.occ = occ;
    return t;
}

// ------------------------------------------------------------------------------------------------
// the exact test of one raw record (k_verify, and k_scan's tail: a scan wave verifies the chunks of records it has
// filled itself, between two of its units)
// ------------------------------------------------------------------------------------------------
// One copy of the rules, in two steps so that a caller with several records per lane asks for all their loads before it
// waits for any: verify_fetch -- the record's fields, the stream record and the guide's signature asked for together --
// and verify_finish -- the exact test on the whole signatures, the first-matching-slice / reporter rule, the run-wise
// count per guide, the terms, the hit slot or rank and terms by raw slot, the key written back unless the tail is lean.
// SORTED_PRUNED: the caller knows that the batch ran the pruned plan on a sorted layout (k_scan's tail runs nowhere
// else); the bucket tables and the list-order layouts then drop out of the code.  Every lane of the wave calls both steps
// (verify_finish counts by wave); a lane without a record passes in_use = false.
struct VerifyRec {
    StreamRec sr;      // sorted layouts: what the stream holds at the record's place
    uint64_t gsig;     // pruned plan: the guide's signature
    uint32_t guide, bucket, slice, tile, offset;
};

// Ctx: VerifyCtx; k_scan's tail reads its own through the kernel-argument segment (KernargCtx: scalar loads made where the
// tail runs -- loads of a by-value argument are made ahead of the scan's loop and held in registers through the passes).
typedef const __attribute__((address_space(4))) VerifyCtx KernargCtx;
template <bool SORTED_PRUNED, class Ctx>
__device__ __forceinline__ VerifyRec verify_fetch(const Ctx &c, uint32_t prune_mode, uint64_t rec, bool in_use)
{
    const auto &v = c.v;
    VerifyRec r;
    r.sr = StreamRec{};
    r.gsig = 0;
    r.guide = kNoGuide; r.bucket = 0; r.slice = 0;
    r.offset = static_cast<uint32_t>(rec) & (kTileCands - 1u);
    r.tile = static_cast<uint32_t>(rec >> 11) & 0x3FFFFFFu;
    const uint32_t gslot = static_cast<uint32_t>(rec >> 37); // pruned scan: the slot's id, not its number
    // sorted layouts: what the stream holds at the record's place, asked for before anything else is known about it
    if (in_use && v.srec) r.sr = v.srec[static_cast<uint64_t>(r.tile) * kTileCands + r.offset];
    else if (in_use && v.sid) r.sr.id = v.sid[static_cast<uint64_t>(r.tile) * kTileCands + r.offset];
    // Whose record it is.  Pruned scan: the record says so itself (slot_id: guide and slice; the bucket follows from the
    // slice and the guide's signature, which is asked for beside the stream record, not behind it).  Bucket-level plan:
    // the guide slot knows its guide and its bucket -- no search for the tile's.
    if (in_use) {
        if (SORTED_PRUNED || prune_mode) {
            const uint64_t low = (1ull << v.slice_width) - 1ull;
            if (gslot != kPadSlotId) slot_id_unpack(gslot, r.slice, r.guide);
            if (r.guide >= c.n || r.slice >= v.n_slices) r.guide = kNoGuide; // (a padding slot, or no slot of this batch at all)
            else {
                r.gsig = c.guides[r.guide];
                r.bucket = (r.slice << v.slice_width) + (static_cast<uint32_t>(r.gsig >> (v.slice_width * r.slice)) & static_cast<uint32_t>(low));
            }
        } else if constexpr (!SORTED_PRUNED) {
            r.guide = c.gidx[gslot];
            r.bucket = c.gbucket[gslot];
            r.slice = r.bucket >> v.slice_width;
        }
    }
    return r;
}

// `chunk`, `t`: the record's chunk and its slot there (1 .. kChunkRecs - 1 when in_use); lane: of the wave.
// SLOT = false: the record has no raw slot -- k_scan's tail on a buffer of its wave's LDS, a lean batch only: rank, terms
// and key by raw slot are what the grouping pass reads, and a lean batch has none (a hit beyond its guide's slots is
// counted in `overflowed`, and the batch runs again in full).
template <bool SORTED_PRUNED, bool SLOT = true, class Ctx>
__device__ __forceinline__ void verify_finish(const Ctx &c, uint32_t prune_mode, const VerifyRec &r, bool in_use,
                                              uint32_t chunk, uint32_t t, uint32_t lane)
{
    const auto &v = c.v;
    const int max_dist = c.max_dist;
    const bool calc_mit = c.calc_mit != 0u, calc_cfd = c.calc_cfd != 0u;
    const uint64_t low = (1ull << v.slice_width) - 1ull;
    const uint32_t guide = r.guide, bucket = r.bucket, slice = r.slice, tile = r.tile, offset = r.offset;
    uint64_t gsig = r.gsig;
    uint64_t key = kDeadKey;
    double mit_term = 0.0, cfd_term = 0.0; // of a record that survives: computed here, one thread per hit, so that the
                                           // replay (one wave per guide, a chain of dependent steps) only adds them up
    uint64_t hit_gsig = 0, hit_ot = 0;     // ... from these
    uint32_t hit_occ = 0;
    const bool by_id = SORTED_PRUNED || v.srec || v.sid; // the scoring order is (slice, site id): ImageHeader
    if (guide != kNoGuide) {
        // Is the candidate the item's?  The scan notes only candidates of the item's own window (`keep`: not the zero
        // padding behind a bucket, not the neighbouring group that shares the tile), so on the sorted layouts, which need
        // nothing else from the bucket tables, the question is not asked again.  The list-order layouts find their list
        // entry through the bucket's start and check on the way.
        uint64_t start = 0, pos = 0;
        bool mine = true;
        if constexpr (!SORTED_PRUNED) if (!by_id) {
            start = v.bucket_start[bucket];
            pos = static_cast<uint64_t>(tile - v.tile_first[bucket]) * kTileCands + offset; // in the stream
            mine = pos < v.bucket_start[bucket + 1] - start;
        }
        if (mine) {
            if (!(SORTED_PRUNED || prune_mode)) gsig = c.guides[guide];
            // sorted layouts: signature, site id (and a 24-bit copy of the count) come in one stream-order record, or --
            // compact -- the id alone, with the signature behind it in the site table
            StreamRec sr = r.sr;
            if (v.sid) sr.sig = v.sites[sr.id]; // (the site table of a sorted layout: signature | 24-bit count << 40, like a stream record)
            uint64_t ot = sr.sig & kSigMask;
            if constexpr (!SORTED_PRUNED)
                if (!by_id) ot = v.esig   ? v.esig[start + pos]
                                 : v.occ8 ? candidate_signature(v, bucket, tile, offset) // cold sections in host memory
                                          : v.sites[v.entries[start + pos] & 0xFFFFFFFFull];
            if (__builtin_popcountll(mismatch_mask(gsig, ot)) <= max_dist) { // exact, full signatures (:376-382)
                // First-matching-slice rule (equivalent of the seen bitmap, isslScoreOfftargets.cpp:385-390,463):
                // the site was already met iff an earlier slice of the XOR is all zero.
                const uint64_t x = gsig ^ ot;
                if (!(SORTED_PRUNED || prune_mode)) {
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
                    uint32_t occ = 0;
                    if (by_id) {
                        occ = static_cast<uint32_t>(sr.sig >> 40);
                        if (occ == kOccSaturated) occ = v.site_occ[sr.id];
                    } else if constexpr (!SORTED_PRUNED) {
                        if (v.occ8) {
                            occ = v.occ8[start + pos];
                            if (occ == 255u) occ = static_cast<uint32_t>(v.entries[start + pos] >> 32); // (host memory)
                        } else {
                            occ = static_cast<uint32_t>(v.entries[start + pos] >> 32);
                        }
                    }
                    hit_gsig = gsig; hit_ot = ot; hit_occ = occ;
                }
            }
        }
    }
    // Count the hit for its guide.  The count doubles as the hit's place in the guide's segment, so that the grouping
    // pass scatters without a second atomic (rank, by raw-record slot).  The hits of a guide in one unit lie side by
    // side in the chunk (the scan wave notes them guide by guide): every RUN of neighbouring lanes with the same guide
    // takes one atomic, issued by its first lane -- no loop, every run of the wave in the same instruction.  (The
    // atomics are half of k_verify's time on a skewed index: profiles/r03_ablation_verify.log.)
    const bool live = key != kDeadKey;
    const uint32_t prev_guide = static_cast<uint32_t>(__shfl_up(static_cast<int>(live ? guide : kNoGuide), 1, 64));
    const bool continues = live && lane != 0u && prev_guide == guide;    // (a dead lane never equals a live one: kNoGuide)
    const uint64_t starts = __ballot(!continues);                        // first lanes of runs, and the dead lanes
    uint32_t rank = 0;
    if (starts == ~0ull) { // (uniform over the wave) no runs, the usual case on an even index: everybody for itself
        if (live) rank = atomicAdd(&c.gcount[guide], 1u);
    } else {
        const uint64_t upto = (lane == 63u ? 0ull : (~0ull << (lane + 1u))); // the lanes above this one
        const uint32_t head = 63u - static_cast<uint32_t>(__builtin_clzll(starts & ~upto)); // lane 0 always starts: never empty
        const uint64_t later = starts & upto;
        const uint32_t next = later ? static_cast<uint32_t>(__builtin_ctzll(later)) : 64u;
        uint32_t base = 0;
        if (live && !continues) base = atomicAdd(&c.gcount[guide], next - lane); // the run is [lane, next)
        rank = static_cast<uint32_t>(__shfl(static_cast<int>(base), static_cast<int>(head), 64)) + (lane - head);
    }
    if (live && rank == kReplayLds) atomicAdd(&c.counters->overflowed, 1u); // the guide's first hit beyond what k_replay takes
    if (live && rank < c.slot_hits) {
        // hit slots (Workspace): the hit goes to its final place at once and takes no part in the grouping pass
        int dist;
        score_terms(v, hit_gsig, hit_ot, hit_occ, calc_mit, calc_cfd, mit_term, cfd_term, dist);
        const uint64_t at = static_cast<uint64_t>(guide) * c.slot_hits + rank;
        SlotRec s;
        s.mit = mit_term; s.cfd = cfd_term; s.key = key;
        s.pad = slot_pad(hit_occ, static_cast<uint32_t>(dist)); // (read by k_profile alone)
        c.slots[at] = s;
        key = kDeadKey;
    } else if (SLOT && live) {
        const uint64_t slot = static_cast<uint64_t>(chunk) * (kChunkRecs - 1u) + (t - 1u); // < cap_chunks * 127 <= cap_hits
        c.rank[slot] = rank;
        // The terms (:392-460) -- unless the guide already has more hits than the replays that read them take
        // (k_replay, k_replay_mid): the many-hit replay works out the terms of the hits it walks by itself, and on
        // skewed data most hits belong to such guides and lie behind their early exit.
        if (rank < kMidHits) {
            int dist;
            score_terms(v, hit_gsig, hit_ot, hit_occ, calc_mit, calc_cfd, mit_term, cfd_term, dist);
            reinterpret_cast<double2 *>(c.pay)[slot] = make_double2(mit_term, cfd_term);
        }
    }
    // (a lean batch has no grouping pass to read the keys back -- every hit went to its guide's slots, or the batch is run
    // again in full: 8 bytes per record that need not be written)
    if (SLOT && in_use && !c.lean_tail) c.raw[static_cast<uint64_t>(chunk) * kChunkRecs + t] = key;
}

// Both steps at once: one record per lane (k_verify).
template <bool SORTED_PRUNED, bool SLOT = true, class Ctx>
__device__ __forceinline__ void verify_record(const Ctx &c, uint32_t prune_mode, uint64_t rec, bool in_use, uint32_t chunk,
                                              uint32_t t, uint32_t lane)
{
    const VerifyRec r = verify_fetch<SORTED_PRUNED>(c, prune_mode, rec, in_use);
    verify_finish<SORTED_PRUNED, SLOT>(c, prune_mode, r, in_use, chunk, t, lane);
}

} // namespace issl
