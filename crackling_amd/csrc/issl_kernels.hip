// HIP kernels of the ISSL off-target scorer for gfx950 (MI355X).  Wave = 64 lanes.
//
// Pipeline for one batch of guides (reference: src/ISSL/isslScoreOfftargets.cpp:307-511):
//   bin_*      group the guides of the batch by (slice, slice value) = by index bucket; on a sorted image
//              once more by (bucket, byte of the successor slice) for the pruned scan                 (A3)
//   scan       bucket tiles (pruned: the units of the successor-byte groups that can hold a hit) against
//              the guides placed there: XOR, fold, popcount, bit-sliced; candidates within max_dist are
//              NOTED as 8-byte records (guide slot, tile, offset)                                     (A4-A6)
//   verify     every record: exact test on the whole signatures, first-matching-slice rule (replaces
//              the seen-bitmap, A7), key (guide, slice, site id or list position), MIT / CFD terms;
//              the first 512 hits of a guide go straight to its hit slots (Workspace)                 (A7-A9)
//              -- by the scan wave that noted the record, between two of its units (scan_tail: pruned
//              plan, sorted layout), else by k_verify
//   group_*    counting sort by guide of the keys and terms that lie beyond their guide's slots
//              (nothing on an index where no guide has more than 512 hits)
//   replay     per guide: its hits in key order = the reference's scan order, terms added sequentially
//              with the reference's early exit                                                        (A10-A11)
//
// The scan is the ALU-critical kernel.  It streams 4 B per candidate (the signature with the bucket's own
// slice removed, stored bit-sliced: 32 candidates per 32-bit plane) and keeps a tile of 2048 candidates in
// registers while the guide words of the item arrive through scalar loads, so one HBM read of a tile serves
// every guide of the batch that is placed there.
//
// This file holds the scan alone and keeps its path: bench.py stamps its profiles with this file's hash.  The other stages:
// issl_bin.hip (upload packing and guide binning), issl_verify.hip, issl_group.hip, issl_replay.hip, issl_report.hip; what
// they share is in issl_kernels.hpp.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "issl_kernels.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// scan
// ------------------------------------------------------------------------------------------------

struct alignas(4 * kGuideGroup) GuideGroup {
    uint32_t w[kGuideGroup];
};


// ---- raw records ------------------------------------------------------------------------------
// A candidate that the scan finds within max_dist of a guide is only NOTED by the scan kernel, as an
// 8-byte record (guide slot, tile, offset in tile), with plain stores into a chunk of the raw buffer
// that the wave owns -- no dependent load, no returning atomic on the hot path (one hit per ~50k
// comparisons is frequent enough that a latency chain per hit would dominate the kernel).
// Every record is then checked exactly, the first-matching-slice rule applied and the survivors turned
// into keys (verify_record, issl_kernels.hpp) -- off the hot path: by the wave itself between two units
// (scan_tail), by k_verify where no tail runs.  Chunk = kChunkRecs slots of 8 bytes, slot 0 unused; raw_used[chunk] = slots in use (slot 0 included).
__device__ __forceinline__ uint64_t raw_record(uint32_t gslot, uint32_t tile, uint32_t offset)
{
    return (static_cast<uint64_t>(gslot) << 37) | (static_cast<uint64_t>(tile) << 11) | offset;
}

struct RawWriter {
    uint64_t *chunk;   // current chunk of this wave (wave-uniform)
    uint32_t fill;     // used slots of the current chunk, header included
    uint32_t left;     // further chunks of the wave's current reservation (they follow the current one)
    uint32_t reserve;  // chunks the next reservation takes: 1, 2, 4 ... 16 -- a wave in a hit-dense bucket fills a chunk
                       // every few guides, and every reservation is a returning atomic that the wave waits for with all
                       // its record stores; a wave with few hits never reserves a chunk it does not use
    uint32_t tail;     // the wave's verify tail (scan_tail).  kTailOn: one follows; kTailPending: a chunk has been retired since
                       // it last ran; kTailRangeDone: the wave's range has no unit left; kTailLast: the chunk the wave is
                       // writing when its range is done is the tail's too -- always where the tail is forced, else once
                       // the wave has retired a chunk.  (A wave of a small batch notes a few records; verifying them
                       // is a chain of six dependent accesses behind its last unit, with nothing on the CU to hide it:
                       // 64 guides 0.058 -> 0.076 ms, 10 k guides x 50 M sites 0.29 -> 0.42 ms per step with every wave's
                       // last chunk taken.  k_verify does those chunks at full occupancy, as before.)
    uint32_t lbuf;     // the tail build on the pruned plan notes into LDS (wave_recs): byte address there of the buffer being filled
                       // (`fill` counts ITS slots); the other buffer is lbuf ^ kRecBufBytes.  Everything else the buffers need is
                       // looked at when one is full and lives in LDS (slot 0 of a waiting buffer, wave_bufs): the scalar registers
                       // are all taken, and one more carried through the passes is one more spilt to a vector register's lanes
    uint32_t budget;   // chunks' worth of records the wave may still take on for its tail: a buffer drained from LDS costs one, a
                       // listed reservation its chunks -- in all the chunks of a full list (wave_runs), whichever way the records go
};
constexpr uint32_t kTailOn = 4u, kTailPending = 1u, kTailRangeDone = 2u, kTailLast = 8u;
// ... of the LDS buffers: kTailLds: the other buffer is full and the tail's; kTailHave: `chunk` is a chunk nothing has been
// copied to yet; kTailLean: a full buffer may wait in LDS for the tail (a lean batch: nothing wants its records' raw slots)
constexpr uint32_t kTailLds = 16u, kTailHave = 32u, kTailLean = 64u;
constexpr uint32_t kListChunks = 64u; // chunks of a full list: 1 + 1 + 2 + 4 + 8 + 16 + 16 + 16
static_assert(kScanVerifyRuns == 8u, "kListChunks: the chunks of run_chunks(0 .. kScanVerifyRuns - 1)");
// The wave's list in LDS for its verify tail: [0] = runs listed, then the first chunk of each -- run 0 is the wave's own
// chunk, run k >= 1 its k-th reservation, min(1 << (k - 1), 16) chunks.  A list that is full stays as it is: what the wave
// reserves from then on is k_verify's.  Behind the list: the tail's cursor (run, chunk of the run) and its count of
// records.  (Found from the thread's number where it is wanted, all cold places: a pointer carried through the scan's
// loop is a register the passes do not have.)
constexpr uint32_t kRunCursor = 1u + kScanVerifyRuns, kRunWords = kRunCursor + 3u;
__device__ __forceinline__ uint32_t *wave_runs()
{
    __shared__ uint32_t runs[16][kRunWords];
    return runs[threadIdx.x >> 6];
}
__device__ __forceinline__ uint32_t run_chunks(uint32_t k) { return k == 0u ? 1u : k > 4u ? 16u : 1u << (k - 1u); }
// ... and, in the build for lean batches, two words for the wave's record buffers in LDS (wave_recs).  kBufDrained:
// buffers the tail has drained from LDS; kBufTop: one past the last chunk the wave has given a fill count (k_verify stops at
// the launch's largest).  Looked at when a buffer is full or drained, by lane 0.
constexpr uint32_t kBufDrained = 0u, kBufTop = 1u;
__device__ __forceinline__ uint32_t *wave_bufs()
{
    __shared__ uint32_t bufs[16][2];
    return bufs[threadIdx.x >> 6];
}
// The wave's two record buffers in LDS (the tail build on the pruned plan): kChunkRecs slots each, slot 0 unused as in a
// chunk, so a buffer is one round of the tail, two records per lane; slot 0 of a buffer that waits for the tail holds its
// slots in use.  Addressed by 32-bit LDS byte addresses.
typedef __attribute__((address_space(3))) uint64_t LdsRec;
constexpr uint32_t kRecBufBytes = 8u * kChunkRecs;
__device__ __forceinline__ uint32_t wave_recs()
{
    __shared__ __attribute__((aligned(2 * kRecBufBytes))) uint64_t recs[16][2u * kChunkRecs];
    return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsRec *)recs[threadIdx.x >> 6])));
}
__device__ __forceinline__ LdsRec *lds_rec(uint32_t at) { return reinterpret_cast<LdsRec *>(static_cast<uintptr_t>(at)); }

__device__ __forceinline__ void raw_retire(const RawWriter &w, uint32_t lane, const uint64_t *raw, uint32_t *raw_used)
{
    if (lane == 0) raw_used[(w.chunk - raw) / kChunkRecs] = w.fill;
}

// LDS: the wave notes into LDS (note_candidates) and comes here for the chunk a buffer is copied to (lds_spill): `fill`
// and the tail's flags are that buffer's business, and a reservation is listed only within the wave's budget.
template <bool LDS = false>
__device__ __forceinline__ void raw_acquire(RawWriter &w, uint64_t *raw, uint32_t max_chunks, Counters *counters,
                                            uint32_t lane)
{
    if constexpr (!LDS) {
        w.fill = 1;
        if ((w.tail & kTailOn) != 0u) w.tail |= kTailPending | kTailLast;
    }
    if (w.left != 0u) { // the next chunk of the reservation: its header was cleared with all the others (k_guide_hist)
        w.chunk += kChunkRecs;
        w.left -= 1u;
        return;
    }
    const uint32_t take = w.reserve;
    uint32_t idx = 0;
    if (lane == 0) idx = atomicAdd(&counters->raw_chunks, take);
    idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx + take > max_chunks) { // buffer exhausted: write into the spare chunk, the host grows the buffer and re-runs
        idx = max_chunks;
        if (lane == 0) counters->raw_overflow = 1u;
        w.chunk = raw + static_cast<uint64_t>(idx) * kChunkRecs;
        return; // (left stays 0: every further chunk comes here again)
    }
    w.chunk = raw + static_cast<uint64_t>(idx) * kChunkRecs;
    w.left = take - 1u;
    if (take < 16u) w.reserve = take * 2u;
    if constexpr (LDS) {
        if ((w.tail & kTailOn) == 0u) return;
        if (w.budget < take) return;
        w.budget -= take; // (a list that is full has used the budget up: the reservations of a wave that drains nothing are 63 chunks)
    }
    if ((w.tail & kTailOn) != 0u && lane == 0) {
        uint32_t *runs = wave_runs();
        const uint32_t listed = runs[0];
        if (listed < kScanVerifyRuns) {
            runs[1u + listed] = idx;
            runs[0] = listed + 1u;
        }
    }
}

// A buffer of the wave's LDS records (`used` slots, slot 0 included) into the next chunk of the wave -- its own, then its
// reservations, as the records went before there were buffers -- with two 8-byte stores per lane, and the chunk's fill
// count.  From there the records go the way they always went: the read-back tail when the chunk is listed (`last`: also
// when it is the first the wave retires), else k_verify.
__device__ __forceinline__ void lds_spill(RawWriter &w, uint32_t buf, uint32_t used, bool last, uint32_t lane, uint64_t *raw,
                                          uint32_t *raw_used, uint32_t max_chunks, Counters *counters)
{
    if ((w.tail & kTailHave) == 0u) raw_acquire<true>(w, raw, max_chunks, counters, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t r0 = lds_rec(buf)[lane], r1 = lds_rec(buf)[64u + lane];
    if (lane != 0u && lane < used) w.chunk[lane] = r0;
    if (64u + lane < used) w.chunk[64u + lane] = r1;
    __builtin_amdgcn_wave_barrier();
    const uint32_t idx = static_cast<uint32_t>((w.chunk - raw) / kChunkRecs);
    if (lane == 0) {
        raw_used[idx] = used;
        if (idx + 1u > wave_bufs()[kBufTop]) wave_bufs()[kBufTop] = idx + 1u;
    }
    w.tail &= ~kTailHave;
    if ((w.tail & kTailOn) != 0u && (last || (w.tail & kTailLast) != 0u)) w.tail |= kTailPending | kTailLast;
}

// The buffer the wave is filling has no room for a pass's records.  A lean batch: it waits in LDS for the tail at the next
// unit boundary and the wave goes on in the other buffer -- unless that one still waits (both filled inside one unit: a
// hit-dense one), which then goes to a chunk first, or the wave's budget is used up.  Any other batch needs raw slots for its
// grouping pass: every full buffer goes to a chunk at once.
__device__ __forceinline__ void lds_buffer_full(RawWriter &w, uint32_t lane, uint64_t *raw, uint32_t *raw_used, uint32_t max_chunks,
                                                Counters *counters)
{
    const bool waits = (w.tail & kTailLds) != 0u; // the other buffer: to a chunk, and this one waits in its place (its share of the budget too)
    uint32_t used = w.fill;
    w.fill = 1;
    bool stays = waits;
    if (!waits && (w.tail & kTailLean) != 0u) {
        stays = w.budget != 0u;
        if (stays) w.budget -= 1u;
    }
    if (stays) {
        if (lane == 0) *lds_rec(w.lbuf) = used;
        w.lbuf ^= kRecBufBytes;
        w.tail |= kTailLds | kTailLast;
        if (!waits) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        used = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(*lds_rec(w.lbuf)));
    }
    // (either way the buffer that goes to a chunk is the one the wave fills next: the copy's loads stand ahead of the next stores)
    lds_spill(w, w.lbuf, used, true, lane, raw, raw_used, max_chunks, counters);
}

// ---- bit-sliced distance test -------------------------------------------------------------------
// 3:2 and 2:2 counters on bit planes; v_bitop3_b32 evaluates any 3-input boolean function in one op.
__device__ __forceinline__ void full_add(uint32_t a, uint32_t b, uint32_t c, uint32_t &sum, uint32_t &carry)
{
    sum = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);   // a ^ b ^ c
    carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); // majority(a, b, c)
}
__device__ __forceinline__ void half_add(uint32_t a, uint32_t b, uint32_t &sum, uint32_t &carry)
{
    sum = a ^ b;
    carry = a & b;
}

// For the lane's 32 candidates (planes c[]) and one guide scan word gw: the plane of candidates whose
// mismatch count over the 16 positions is <= THR (THR = 0..4 compiled in; THR < 0: runtime `thr`, any value).
// Position p mismatches iff low or high bit differs: (c[p] ^ G0p) | (c[16+p] ^ G1p) with the guide's bits
// broadcast to all-zero / all-one scalars (isslScoreOfftargets.cpp:376-380 in transposed form); the 16 mismatch
// planes are then counted with a carry-save adder tree.
// `keep`: the lane's candidates that belong to the item (the others are padding or a neighbouring group's); folded into
// the last operation of the count, which has an operand to spare for every compiled threshold but 1.
template <int THR>
__device__ __forceinline__ uint32_t count_near(const uint32_t (&m)[16], uint32_t thr, uint32_t keep);

template <int THR>
__device__ __forceinline__ uint32_t near_plane(const uint32_t (&c)[kPlanes], uint32_t gw, uint32_t thr, uint32_t keep)
{
    uint32_t m[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const uint32_t g0 = 0u - ((gw >> p) & 1u);
        const uint32_t g1 = 0u - ((gw >> (16 + p)) & 1u);
        m[p] = (c[p] ^ g0) | (c[16 + p] ^ g1);
    }
    return count_near<THR>(m, thr, keep);
}

// The same test in a SHORT unit: every plane register holds the lane's 16 / 8 candidates two / four times over, and
// mask word p (32 words in LDS, made by the wave itself: short_unit_masks) carries bit p of two / four guides' scan
// words, each spread over its field: one pass, two / four guides.  The masks arrive as wave-uniform VGPRs (every lane
// reads the same 16 bytes), four positions at a time so that they never occupy more than a handful of registers.
template <int THR>
__device__ __forceinline__ uint32_t near_plane_masks(const uint32_t (&c)[kPlanes], const uint4 *gm /*LDS, 8 x uint4*/,
                                                     uint32_t thr, uint32_t keep)
{
    uint32_t m[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 lo = gm[q], hi = gm[4 + q];
        asm volatile("" ::: "memory"); // (keeps the next loads behind these: at most two steps' masks are live)
        m[4 * q + 0] = (c[4 * q + 0] ^ lo.x) | (c[16 + 4 * q + 0] ^ hi.x);
        m[4 * q + 1] = (c[4 * q + 1] ^ lo.y) | (c[16 + 4 * q + 1] ^ hi.y);
        m[4 * q + 2] = (c[4 * q + 2] ^ lo.z) | (c[16 + 4 * q + 2] ^ hi.z);
        m[4 * q + 3] = (c[4 * q + 3] ^ lo.w) | (c[16 + 4 * q + 3] ^ hi.w);
    }
    return count_near<THR>(m, thr, keep);
}

// Masks of up to 8 passes of a short unit (guide slots g0 .. g0 + 8 * per - 1) into the wave's own 1 KiB of LDS: lane
// (pass i, quarter q) makes the four words 4q .. 4q + 3 of pass i: bit p of each of the pass's `per` guide words, spread
// over that guide's field of `shape` bits.  wide: shape 16, two guides per pass (their slots arrive as one 16-byte load);
// else shape 8, four guides (two 16-byte loads: g0 is a multiple of 8).  A slot's word uses bits 0..25, so the quarter that
// would make words 28 .. 31 stores the pass's slot ids there instead: the cold block reads the id of the guide a candidate
// came near from the wave's own LDS (kPassIds).
constexpr uint32_t kPassIds = 28; // word of a pass's 32 that holds the first of its ids
typedef uint32_t SlotPair __attribute__((ext_vector_type(4))); // two slots, word and id each, as one load (a uint4's four members are loaded one by one where only one lane in eight wants the ids)
__device__ __forceinline__ void short_unit_masks(const FineSlot *__restrict__ slots, uint32_t g0, bool wide,
                                                 uint32_t lane, uint4 *lds_masks)
{
    const uint32_t i = lane >> 3, q = lane & 7u;
    uint32_t m[4];
    if (wide) {
        const SlotPair gw = *reinterpret_cast<const SlotPair *>(slots + g0 + 2u * i);
        const uint32_t a = gw.x >> (4u * q), b = gw.z >> (4u * q);
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
            m[r] = ((0u - ((a >> r) & 1u)) & 0xFFFFu) | ((0u - ((b >> r) & 1u)) << 16);
        if (q == 7u) { m[0] = gw.y; m[1] = gw.w; }
    } else {
        const SlotPair *src = reinterpret_cast<const SlotPair *>(slots + g0 + 4u * i);
        const SlotPair ga = src[0], gb = src[1];
        const uint32_t t[4] = {ga.x >> (4u * q), ga.z >> (4u * q), gb.x >> (4u * q), gb.z >> (4u * q)};
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            // bit r of the four words into bits 0, 8, 16, 24; times 255 = each spread over its byte
            const uint32_t bits = ((t[0] >> r) & 1u) | (((t[1] >> r) & 1u) << 8) | (((t[2] >> r) & 1u) << 16) | (((t[3] >> r) & 1u) << 24);
            m[r] = bits * 255u;
        }
        if (q == 7u) { m[0] = ga.y; m[1] = ga.w; m[2] = gb.y; m[3] = gb.w; }
    }
    lds_masks[i * 8u + q] = make_uint4(m[0], m[1], m[2], m[3]);
}

// The planes of candidates whose mismatch planes m[0..15] count up to at most THR.
template <int THR>
__device__ __forceinline__ uint32_t count_near(const uint32_t (&m)[16], uint32_t thr, uint32_t keep)
{
    uint32_t s0, s1, s2, s3, s4, t, u, n0, n1, n2;
    uint32_t k2[8], k4[4], k8a, k8b;
    // weight 1: 16 planes
    full_add(m[0], m[1], m[2], s0, k2[0]);
    full_add(m[3], m[4], m[5], s1, k2[1]);
    full_add(m[6], m[7], m[8], s2, k2[2]);
    full_add(m[9], m[10], m[11], s3, k2[3]);
    full_add(m[12], m[13], m[14], s4, k2[4]);
    full_add(s0, s1, s2, t, k2[5]);
    full_add(s3, s4, m[15], u, k2[6]);
    half_add(t, u, n0, k2[7]);
    // weight 2: 8 planes
    uint32_t a2, b2, c2;
    full_add(k2[0], k2[1], k2[2], a2, k4[0]);
    full_add(k2[3], k2[4], k2[5], b2, k4[1]);
    full_add(k2[6], k2[7], a2, c2, k4[2]);
    half_add(b2, c2, n1, k4[3]);
    // weight 4: 4 planes k4[0..3], S4 = how many of them are set.  count = 4 S4 + 2 n1 + n0, so the compiled thresholds
    // need S4 only as "none", "at least one", "at least two" -- cheaper than adding the four planes up:
    //   count <= 3  <=>  S4 == 0;   count <= 4  <=>  S4 == 0 or (S4 == 1 and n1 == n0 == 0)
    // with o = k4[0] | k4[1] | k4[2] and p = majority(k4[0], k4[1], k4[2]):  S4 >= 1 = o | k4[3],
    // S4 >= 2 = p | (o & k4[3]), and  S4 >= 2 or (S4 >= 1 and w)  =  p | majority(o, k4[3], w).
    if (THR >= 0 && THR <= 4) {
        const uint32_t o = __builtin_amdgcn_bitop3_b32(k4[0], k4[1], k4[2], 0xFE); // a | b | c
        // (the last operation of each case is ~(a | b) & keep as one bitop3: table 0x02)
        if (THR == 0) return __builtin_amdgcn_bitop3_b32(o, __builtin_amdgcn_bitop3_b32(k4[3], n1, n0, 0xFE), keep, 0x02);
        if (THR == 1) return __builtin_amdgcn_bitop3_b32(o, k4[3], n1, 0x01) & keep;     // ~(a | b | c)
        if (THR == 2) return __builtin_amdgcn_bitop3_b32(o, __builtin_amdgcn_bitop3_b32(k4[3], n1, n0, 0xF8), keep, 0x02); // a | (b & c)
        if (THR == 3) return __builtin_amdgcn_bitop3_b32(o, k4[3], keep, 0x02);
        const uint32_t p = __builtin_amdgcn_bitop3_b32(k4[0], k4[1], k4[2], 0xE8);            // majority
        const uint32_t z = __builtin_amdgcn_bitop3_b32(o, k4[3], n1 | n0, 0xE8);
        return __builtin_amdgcn_bitop3_b32(p, z, keep, 0x02);
    }
    uint32_t a4;
    full_add(k4[0], k4[1], k4[2], a4, k8a);
    half_add(a4, k4[3], n2, k8b);
    // generic threshold: count = n0 + 2 n1 + 4 n2 + 8 n3 + 16 n4, compared MSB first with the uniform thr
    const uint32_t n[5] = {n0, n1, n2, k8a ^ k8b, k8a & k8b};
    uint32_t gt = 0u, eq = ~0u;
#pragma unroll
    for (int b = 4; b >= 0; --b) {
        if ((thr >> b) & 1u) {
            eq &= n[b];
        } else {
            gt |= eq & n[b];
            eq &= ~n[b];
        }
    }
    return keep & ~gt;
}

// ---- the pruned scan's test: 12 positions (fine_word) -------------------------------------------------------------
// The planes of candidates whose 12 mismatch planes m[] (+ the class plane f when EXTRA) count up to at most B
// (B = 0..4 compiled in; B < 0: runtime `thr`).  count = n0 + 2 n1 + 4 S4 with S4 the number of set planes among the
// three of weight 4 (k4[0], k4[1], a2 & b2), so the compiled budgets need the weight-2 sums a2, b2 only through a handful
// of three-input functions: 41 vector operations per pass for B = 3 (the class-1 guides of max_dist 4: twelve of
// thirteen), 46 for B = 4, against 62 for the 16-position test.
// `prev` (out): three planes whose OR is "some position of the previous slice mismatches" -- m[0..3] are that slice's
// (fine_order), and m[0] | m[1] | m[2] = sum | carry of the first adder.  Only the cold block looks at them (fine_dup).
struct PrevSlice {
    uint32_t a, b, c;
};
template <int B, bool EXTRA>
__device__ __forceinline__ uint32_t count_near12(const uint32_t (&m)[12], uint32_t f, uint32_t thr, uint32_t keep, PrevSlice &prev)
{
    uint32_t s0, s1, s2, s3, t, n0, a2, b2, k2[6], k40, k41;
    full_add(m[0], m[1], m[2], s0, k2[0]);
    prev.a = s0; prev.b = k2[0]; prev.c = m[3];
    full_add(m[3], m[4], m[5], s1, k2[1]);
    full_add(m[6], m[7], m[8], s2, k2[2]);
    full_add(m[9], m[10], m[11], s3, k2[3]);
    full_add(s0, s1, s2, t, k2[4]);
    if (EXTRA) full_add(t, s3, f, n0, k2[5]);
    else half_add(t, s3, n0, k2[5]);
    full_add(k2[0], k2[1], k2[2], a2, k40);
    full_add(k2[3], k2[4], k2[5], b2, k41);
    // bitop3 tables: bit (4a + 2b + c) of the constant is f(a, b, c)
    if (B >= 0 && B <= 3) {
        const uint32_t r1 = __builtin_amdgcn_bitop3_b32(k40, k41, keep, 0x02);              // ~(a | b) & c: no weight-4 plane among the first two
        if (B == 3) return __builtin_amdgcn_bitop3_b32(r1, a2, b2, 0x70);                   // a & ~(b & c): S4 == 0
        if (B == 1) return __builtin_amdgcn_bitop3_b32(r1, a2, b2, 0x10);                   // a & ~(b | c): S4 == 0 and n1 == 0
        if (B == 0) return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(r1, a2, b2, 0x10), n0, n0, 0x30); // ... and n0 == 0
        const uint32_t r2 = __builtin_amdgcn_bitop3_b32(r1, a2, b2, 0x70);
        return __builtin_amdgcn_bitop3_b32(r2, a2 ^ b2, n0, 0x70);                          // B == 2: S4 == 0 and not (n1 and n0)
    }
    const uint32_t k42 = a2 & b2;
    if (B == 4) { // count <= 4  <=>  not (S4 >= 2 or (S4 >= 1 and (n1 or n0)))
        const uint32_t w = __builtin_amdgcn_bitop3_b32(a2, b2, n0, 0xBE);                   // (a ^ b) | c
        const uint32_t p = __builtin_amdgcn_bitop3_b32(k40, k41, k42, 0xE8);                // majority
        const uint32_t o = __builtin_amdgcn_bitop3_b32(k40, k41, k42, 0xFE);                // a | b | c
        const uint32_t x = __builtin_amdgcn_bitop3_b32(o, w, keep, 0x2A);                   // ~(a & b) & c
        return __builtin_amdgcn_bitop3_b32(x, p, p, 0x30);                                  // a & ~b
    }
    // runtime budget: count = n0 + 2 n1 + 4 n2 + 8 n3 (<= 13), compared MSB first with the uniform thr (< 16)
    uint32_t n2, n3;
    full_add(k40, k41, k42, n2, n3);
    const uint32_t n[4] = {n0, a2 ^ b2, n2, n3};
    uint32_t gt = 0u, eq = ~0u;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
        if ((thr >> b) & 1u) {
            eq &= n[b];
        } else {
            gt |= eq & n[b];
            eq &= ~n[b];
        }
    }
    return keep & ~gt;
}

// Full unit of the pruned scan: the lane's 32 candidates (c[0..11] low, c[12..23] high code bits of the 12 positions)
// against one guide word of the pruned plan (fine_word), budget B.
template <int B>
__device__ __forceinline__ uint32_t near_plane12(const uint32_t (&c)[24], uint32_t gw, uint32_t thr, uint32_t keep, PrevSlice &prev)
{
    uint32_t m[12];
#pragma unroll
    for (int p = 0; p < 12; ++p) {
        const uint32_t g0 = 0u - ((gw >> p) & 1u);
        const uint32_t g1 = 0u - ((gw >> (12 + p)) & 1u);
        m[p] = (c[p] ^ g0) | (c[12 + p] ^ g1);
    }
    return count_near12<B, false>(m, 0u, thr, keep, prev);
}

// Short unit of the pruned scan: two / four guides per pass, the masks from the wave's LDS (short_unit_masks: word p of a
// pass = bit p of its guides' words, spread over their fields; word 24 = the class bits: a plane of weight one).
template <int B>
__device__ __forceinline__ uint32_t near_plane12_masks(const uint32_t (&c)[24], const uint4 *gm /*LDS, 8 x uint4*/,
                                                       uint32_t thr, uint32_t keep, PrevSlice &prev)
{
    uint32_t m[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint4 lo = gm[q], hi = gm[3 + q];
        asm volatile("" ::: "memory"); // (keeps the next loads behind these: at most two steps' masks are live)
        m[4 * q + 0] = (c[4 * q + 0] ^ lo.x) | (c[12 + 4 * q + 0] ^ hi.x);
        m[4 * q + 1] = (c[4 * q + 1] ^ lo.y) | (c[12 + 4 * q + 1] ^ hi.y);
        m[4 * q + 2] = (c[4 * q + 2] ^ lo.z) | (c[12 + 4 * q + 2] ^ hi.z);
        m[4 * q + 3] = (c[4 * q + 3] ^ lo.w) | (c[12 + 4 * q + 3] ^ hi.w);
    }
    const uint32_t f = reinterpret_cast<const uint32_t *>(gm)[24];
    return count_near12<B, true>(m, f, thr, keep, prev);
}

// Guide words that start at any slot (a class boundary is no multiple of 8): a scalar load needs its address dword-aligned only.
// A candidate that also matches the guide exactly in the slice BEFORE the bucket's own is met in that slice's bucket too --
// in the group of the guide's own successor byte, which every guide is placed in -- and the smaller slice reports it
// (k_verify's reporter rule): the record this unit would note is one k_verify reads 16 random bytes for and
// throws away.  58 % of the duplicate records of a hit at distance 4 are of this kind (enumerated in
// tests/test_oracle_golden.py); dropping them here costs two operations in the cold block.
__device__ __forceinline__ uint32_t fine_dup(uint32_t ok, const PrevSlice &prev, uint32_t dup_filter)
{
    const uint32_t prev_mismatch = __builtin_amdgcn_bitop3_b32(prev.a, prev.b, prev.c, 0xFE); // a | b | c
    return ok & (prev_mismatch | ~dup_filter);
}

struct alignas(4) GuideGroupAny {
    uint32_t w[kGuideGroup];
};
// ... of the pruned plan: eight slots, word and id side by side, in ONE 16-dword scalar load -- the id of a guide a
// candidate came near is in a scalar register when the cold block wants it.
struct alignas(8) FineSlotGroup {
    FineSlot s[kGuideGroup];
};

// fine_order as a table: the three plane quads of a slice's 12 positions in 2 bits each, the five 8-bit slices side by side
// (narrow slices: the same three quads for every slice).
constexpr uint32_t fine_order_code(uint32_t slice, uint32_t slice_width)
{
    return fine_order(slice, 0u, slice_width) | (fine_order(slice, 1u, slice_width) << 2) | (fine_order(slice, 2u, slice_width) << 4);
}
constexpr uint32_t kFineOrders = fine_order_code(0u, 8u) | (fine_order_code(1u, 8u) << 6) | (fine_order_code(2u, 8u) << 12) |
                                 (fine_order_code(3u, 8u) << 18) | (fine_order_code(4u, 8u) << 24);
constexpr uint32_t kFineOrderNarrow = fine_order_code(0u, 4u);
static_assert(fine_order_code(0u, 2u) == kFineOrderNarrow && fine_order_code(7u, 4u) == kFineOrderNarrow && (kFineOrders & 63u) == kFineOrderNarrow,
              "narrow slices: one order, that of slice 0 of the 8-bit ones");

// Cold block of the scan: the wave knows that SOME lane has a candidate within thr of a guide.  `ok` = this lane's
// plane of such candidates; bit q of it is candidate q % (1 << w_log) of the lane -- which sits at offset off0 + that of
// `tile` (the lane's own: a window of the pruned scan straddles two tiles) -- against the guide in slot gslot + (q >>
// w_log) (full units: w_log = 5, one guide per pass).  Pruned scan: a record carries the slot's id (slot_id), not its
// number: `gslot` is the pass's id in a full unit, and in a short one the ids of the pass's guides are pass_ids[q >> w_log]
// (the wave's LDS, short_unit_masks).
// What of a record is the lane's alone is made once per unit (RecLane): the two words of raw_record(0, tile, off0); a round
// ORs the candidate's number into the low word and the (wave-uniform) guide slot into the high one.  (The store keeps its
// 64-bit lane address: a scalar base + 8 * rank as a 32-bit offset, with the lane's remaining candidates cleared outside the
// branch, is five vector operations fewer per noting pass and a LONGER launch -- uniform index +-0, skewed one +2 %, same-box
// against this form, profiles/ab_scan_trim_bench.log.)
struct RecLane {
    uint32_t lo, hi;
};
__device__ __forceinline__ RecLane rec_lane(uint32_t tile, uint32_t off0)
{
    return {(tile << 11) | off0, tile >> 21};
}
// ... of the pruned scan's units, whose lanes may sit in two tiles: the lane's candidates start `cand` candidates behind
// lane group `group_abs` of the stream (tile * 64 + group), i.e. at tile << 11 | offset = 32 * group_abs + cand.
__device__ __forceinline__ RecLane rec_lane_at(uint32_t group_abs, uint32_t cand)
{
    const uint64_t at = (static_cast<uint64_t>(group_abs) << 5) + cand;
    return {static_cast<uint32_t>(at), static_cast<uint32_t>(at >> 32)};
}

template <bool LDS = false>
__device__ __forceinline__ void note_candidates(uint32_t ok, uint32_t gslot, const uint32_t *pass_ids, uint32_t w_log, const RecLane &rl,
                                                uint32_t lane, RawWriter &w, uint64_t *raw, uint32_t *raw_used,
                                                uint32_t max_chunks, Counters *counters)
{
    uint64_t who = __ballot(ok != 0u);
    if (who == 0ull) return;
    // One round per candidate of the lane that has most -- almost always ONE: the loop is laid out with its first round as the
    // straight path (a taken branch drains the wave's instruction buffer, and more than half of the passes come through
    // here: k_scan<4> -3 % same-box, profiles/r05_ab_scan_peel_lanes3.log).
    do {
        const uint32_t n = static_cast<uint32_t>(__builtin_popcountll(who));
        if (__builtin_expect(w.fill + n > kChunkRecs, 0)) {
            if constexpr (LDS) {
                lds_buffer_full(w, lane, raw, raw_used, max_chunks, counters);
            } else {
                raw_retire(w, lane, raw, raw_used);
                raw_acquire(w, raw, max_chunks, counters, lane);
            }
        }
        if (ok != 0u) {
            const uint32_t q = static_cast<uint32_t>(__builtin_ctz(ok));
            ok &= ok - 1u;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(who >> 32),
                                                            __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(who), 0u));
            // = raw_record(gslot + (q >> w_log), tile, off0 + (q & ((1u << w_log) - 1u))): off0 is a multiple of 1 << w_log
            const uint32_t slot = pass_ids ? pass_ids[q >> w_log] : gslot + (q >> w_log);
            const uint32_t lo = rl.lo | (q & ((1u << w_log) - 1u)), hi = rl.hi | (slot << 5);
            if constexpr (LDS) *lds_rec(w.lbuf + 8u * (w.fill + rank)) = (static_cast<uint64_t>(hi) << 32) | lo; // (a 32-bit LDS address)
            else w.chunk[w.fill + rank] = (static_cast<uint64_t>(hi) << 32) | lo;
        }
        w.fill += n;
        who = __ballot(ok != 0u);
    } while (__builtin_expect(who != 0ull, 0));
}

// The verify tail of a scan wave.  Between two units its planes and guide words are dead, and the SIMD's other waves go
// on comparing: there, and once more when its range has no unit left, it applies verify_record's rules (issl_kernels.hpp)
// to the records it noted itself, in the chunks only it owns and has retired (wave_runs), instead of leaving them to
// k_verify, which does nothing but wait for HBM while the vector ALUs idle.  (At the end of the range alone the tails of
// all waves fall into the same moment -- the ranges cost the same -- and the chip then does what k_verify does, for as
// long: measured, profiles/ab_scan_verify_bench.log.)  A whole chunk per round, two records per lane, both asked for at
// once; the chains behind them run one after the other (two VerifyRec at a time do not fit the scan's 64 registers
// without scratch).  The wave reads back what it stored: it waits for its stores, and the loads are device-scope ones,
// which cannot be served from a line the CU's L1 holds from before the store.  A chunk it has been through is marked in
// raw_used (kChunkVerified): k_verify leaves it alone.  The walk stops at the first chunk without a fill count: the one
// the wave is writing (raw_retire has not come to it), cleared by the binning like every header.  Only behind the pruned
// plan on a sorted layout (VerifyCtx::scan_verify, plan->fine): there a record needs nothing but itself, the stream and
// the batch's guides.
__device__ __forceinline__ void scan_tail(uint32_t prune_mode, uint32_t lane, const uint64_t *raw, const uint32_t *raw_used)
{
    // the verify context is k_scan's FIRST argument: it stands at the start of the kernel-argument segment, and is read from
    // there HERE (the address passes through an empty asm statement: nothing the tail needs is loaded ahead of the scan's loop).
    // Should the context ever stand elsewhere -- a parameter put in front of it, a code object that lays its arguments out
    // differently -- what is read here is not the context: its record buffer and fill counts are then not the kernel's own
    // `raw` and `raw_used`, and the tail leaves everything to k_verify (tests/test_scan_verify.py sees ws_scan_verified 0).
    uint64_t kernarg = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(kernarg));
    KernargCtx &vc = *(KernargCtx *)kernarg;
    if (vc.raw != raw || vc.raw_used != raw_used) return;
    uint32_t *runs = wave_runs();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the wave's record stores and its fill counts (raw_retire)
    asm volatile("" : "+v"(lane)); // (what the tail makes of the lane number is made here, not ahead of the scan's loop, where it would hold registers through the passes)
    const uint32_t listed = __builtin_amdgcn_readfirstlane(runs[0]);
    uint32_t k = __builtin_amdgcn_readfirstlane(runs[kRunCursor]), j = __builtin_amdgcn_readfirstlane(runs[kRunCursor + 1u]);
    uint32_t verified = 0;
    while (k < listed) {
        const uint32_t chunk = __builtin_amdgcn_readfirstlane(runs[1u + k]) + j;
        const uint32_t used = __builtin_amdgcn_readfirstlane(__hip_atomic_load(vc.raw_used + chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (used <= 1u) break;
        const uint64_t *recs = vc.raw + static_cast<uint64_t>(chunk) * kChunkRecs;
        const uint32_t t0 = lane + 1u, t1 = lane + 65u;
        const bool use0 = t0 < used, use1 = t1 < used && t1 < kChunkRecs;
        const uint64_t rec0 = use0 ? __hip_atomic_load(recs + t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        const uint64_t rec1 = use1 ? __hip_atomic_load(recs + t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        verify_record<true>(vc, prune_mode, rec0, use0, chunk, t0, lane);
        verify_record<true>(vc, prune_mode, rec1, use1, chunk, t1, lane);
        if (lane == 0) vc.raw_used[chunk] = used | kChunkVerified;
        verified += (used < kChunkRecs ? used : kChunkRecs) - 1u;
        if (++j == run_chunks(k)) { j = 0u; ++k; }
    }
    if (lane == 0) { runs[kRunCursor] = k; runs[kRunCursor + 1u] = j; runs[kRunCursor + 2u] += verified; }
}

// The same round on a buffer of the wave's own LDS (`used` slots, slot 0 included), on a lean batch: the records never
// left the wave, so there is no store to wait for, no fill count to read back and no mark to leave -- and no raw slot: on a
// lean batch nothing reads a record's rank, terms or key by its slot (verify_finish<.., false>; a guide beyond its hit
// slots makes the batch run again in full, k_replay).  The context was checked when the wave chose to keep buffers here
// (kTailLean, scan_range).
__device__ __forceinline__ void scan_tail_lds(uint32_t prune_mode, uint32_t lane, uint32_t buf)
{
    uint64_t kernarg = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(kernarg));
    KernargCtx &vc = *(KernargCtx *)kernarg;
    asm volatile("" : "+v"(lane));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the wave's own LDS stores (note_candidates), as in short_unit_masks
    __builtin_amdgcn_wave_barrier();
    const uint32_t used = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(*lds_rec(buf))); // (slot 0: lds_buffer_full)
    const uint32_t t0 = lane + 1u, t1 = lane + 65u;
    const bool use0 = t0 < used, use1 = t1 < used && t1 < kChunkRecs;
    const uint64_t rec0 = use0 ? lds_rec(buf)[t0] : 0ull;
    const uint64_t rec1 = use1 ? lds_rec(buf)[t1] : 0ull;
    __builtin_amdgcn_wave_barrier();
    verify_record<true, false>(vc, prune_mode, rec0, use0, 0u, t0, lane);
    verify_record<true, false>(vc, prune_mode, rec1, use1, 0u, t1, lane);
    if (lane == 0) { wave_runs()[kRunCursor + 2u] += used - 1u; wave_bufs()[kBufDrained] += 1u; }
}

// Scan kernel.  A workgroup of 16 waves (two per CU = 8 waves per SIMD) owns one equal-cost range of the work
// and its waves share the tiles of that range through a ticket counter in LDS: the hardware favours the older
// waves of a SIMD, so waves with equal static shares finish anywhere between 30 % and 100 % of the kernel time
// (measured with the scan_stamps knob) and the SIMDs run half empty for the second half; with the LDS tickets all
// waves of a workgroup stop within one tile of each other.  (A device-wide ticket counter would serialise at ~12 ns
// per ticket; an LDS atomic costs a few hundred cycles and no global traffic.)
// Per tile a wave keeps the 2048 candidates in registers (32 bit planes per lane) while the guide words of the
// item stream through scalar registers, 8 per scalar load.  (Two tiles per wave -- the scalar work of a guide shared by
// 4096 candidates, 4 waves per SIMD -- was measured in round 2: 15 % slower, profiles/r02_ab_scan_tiles_*.log; the
// scalar pipe is not what limits the loop, tools/ubench_issue.hip.)
// The streams the hot loop reads (scan planes, tile table, items, guide words, plan) are separate
// `const __restrict__` kernel arguments: they are never written by this kernel, which lets the compiler fetch the
// wave-uniform ones through the scalar cache.
// The work of one scan workgroup.  FINE: the plan of the pruned scan (single-tile items numbered like the units).  A
// function template instantiated once per plan inside k_scan, so that each copy reads its item list and guide words
// through the kernel's own `__restrict__` arguments (a pointer chosen at run time loses the scalar loads).
template <int THR, bool FINE, bool TAIL, bool LEAN>
__device__ __forceinline__ void scan_range(const uint32_t *__restrict__ scan_stream, const ScanItem *__restrict__ items,
                                           const PlanInfo *__restrict__ plan, const RangeStart *__restrict__ range_start,
                                           const std::conditional_t<FINE, FineSlot, uint32_t> *__restrict__ gword_stream, uint4 *wave_masks,
                                           uint64_t *raw, uint32_t *raw_used, uint32_t max_chunks,
                                           Counters *counters, uint32_t thr, unsigned long long *stamps,
                                           uint64_t *__restrict__ scan_count, uint32_t *next_unit_p, uint32_t *waves_done_p,
                                           unsigned long long *wg_compared_p, unsigned long long t_start,
                                           unsigned long long *span, uint32_t n_tiles, uint32_t slice_bits,
                                           const VerifyCtx &vc, uint32_t *tails_done_p)
{
    uint32_t &next_unit = *next_unit_p;
    uint32_t &waves_done = *waves_done_p;
    unsigned long long &wg_compared = *wg_compared_p;
    constexpr bool fine = FINE;
    uint32_t units_done = 0;
    unsigned long long plane_wait = 0ull; // stamps only: 100 MHz ticks this wave spent waiting for tile planes to arrive
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    // Raw records: the wave's first chunk is the one with its own number (no atomic); k_guide_hist cleared its header.
    RawWriter w;
    const bool no_own_chunk = wave_id >= max_chunks; // buffer smaller than the wave count: spare chunk + overflow flag
    w.chunk = raw + static_cast<uint64_t>(no_own_chunk ? max_chunks : wave_id) * kChunkRecs;
    w.fill = 1;
    w.left = 0;
    w.reserve = 1;
    // the verify tail (scan_tail): the pruned plan alone, and no wave that starts in the spare chunk
    // (the batch's plan says whether its waves fill chunks at all, PlanInfo::scan_tail; scan_verify 2 = the test setting: always)
    const bool tail_launch = TAIL && FINE && (vc.scan_verify > 1u || (vc.scan_verify != 0u && plan->scan_tail != 0u)); // (TAIL = false: the build without a tail, Workspace::scan_verify 0)
    const bool tail = tail_launch && !no_own_chunk;
    w.tail = tail ? kTailOn | (vc.scan_verify > 1u ? kTailLast : 0u) : 0u;
    if (tail && lane == 0) {
        uint32_t *runs = wave_runs();
        runs[0] = 1u; runs[1] = wave_id; runs[kRunCursor] = 0u; runs[kRunCursor + 1u] = 0u; runs[kRunCursor + 2u] = 0u;
    }
    w.lbuf = w.budget = 0u;
    constexpr bool lds = FINE && TAIL && LEAN; // the build for a lean batch on the pruned plan (launch_scan_thr)
    if constexpr (lds) {
        // the records are noted into LDS; the first buffer that goes to a chunk goes to the wave's own.  A lean batch whose tail is
        // armed keeps full buffers in LDS for it -- where the context in the kernel-argument segment is the kernel's own (scan_tail).
        w.lbuf = wave_recs();
        if (lane == 0) { wave_bufs()[kBufDrained] = 0u; wave_bufs()[kBufTop] = 0u; } // (the wave's own chunk is listed from the start)
        w.budget = kListChunks - 1u;
        w.tail |= kTailHave;
        KernargCtx &kc = *(KernargCtx *)__builtin_amdgcn_kernarg_segment_ptr();
        if (tail && vc.lean_tail != 0u && kc.raw == raw && kc.raw_used == raw_used) w.tail |= kTailLean;
    }
    bool own_chunk = false;
    unsigned long long compared = 0ull; // (real candidate, real guide) pairs this wave has compared; wave-uniform

    // Work of this workgroup: from `first` up to (not including) `last`; a position is (item, tile of the item,
    // guide offset inside the item in multiples of 8).  Units = tiles, numbered from the first one; the first and
    // the last tile may be shared with the neighbouring workgroups (guide offsets).
    const RangeStart first = range_start[blockIdx.x];
    const RangeStart last = range_start[blockIdx.x + 1];
    const uint32_t tile_begin = items[first.item].tile0 + first.tile;
    const uint32_t tile_last = items[last.item].tile0 + last.tile; // partly ours when last.goff > 0
    const uint32_t n_units = tile_last - tile_begin + (last.goff ? 1u : 0u);
    uint32_t it = first.item;
    ScanItem cur = items[it];

    const uint32_t order_step = slice_bits == 8u ? 6u : 0u; // pruned scan: bits per slice in kFineOrders
    while (true) {
        if constexpr (FINE && TAIL) {
            // between two units: the chunks retired since; behind the last one: also the chunk the wave was writing
            if constexpr (lds) {
                if ((w.tail & kTailLds) != 0u) { // a full buffer of the wave's LDS
                    scan_tail_lds(plan->fine, lane, w.lbuf ^ kRecBufBytes);
                    w.tail &= ~kTailLds;
                }
            }
            if ((w.tail & kTailPending) != 0u) {
                scan_tail(plan->fine, lane, raw, raw_used);
                w.tail &= ~kTailPending;
            }
        }
        if ((w.tail & kTailRangeDone) != 0u) break;
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(&next_unit, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= n_units) {
            if constexpr (lds) {
                // the part-filled buffer: the tail's under the gate of a wave's last chunk (kTailLast) on a lean batch, else into
                // the wave's next chunk -- its own, if no buffer went to one before -- for the read-back tail or k_verify
                if (own_chunk && w.fill > 1u) {
                    if ((w.tail & (kTailLean | kTailLast)) == (kTailLean | kTailLast) && w.budget != 0u) {
                        if (lane == 0) *lds_rec(w.lbuf) = w.fill;
                        w.lbuf ^= kRecBufBytes;
                        w.tail |= kTailLds;
                    } else {
                        lds_spill(w, w.lbuf, w.fill, false, lane, raw, raw_used, max_chunks, counters);
                    }
                    w.fill = 1u;
                }
                if (own_chunk && no_own_chunk && lane == 0) counters->raw_overflow = 1u;
                own_chunk = false; // (what follows asks whether a CHUNK is left for the read-back tail: lds_spill has said so)
            } else if (own_chunk) {
                raw_retire(w, lane, raw, raw_used);
                if (no_own_chunk && lane == 0) counters->raw_overflow = 1u;
            }
            // comparisons of the workgroup: summed in LDS, stored (not added: no reset needed) by its last wave
            if (lane == 0) {
                atomicAdd(&wg_compared, compared);
                if (atomicAdd(&waves_done, 1u) == (blockDim.x >> 6) - 1u) {
                    scan_count[blockIdx.x] = atomicAdd(&wg_compared, 0ull);
                    if (!tail_launch) atomicMax(span + 1, static_cast<unsigned long long>(__builtin_amdgcn_s_memrealtime())); // (no tails: the launch ends here)
                }
            }
            w.tail |= kTailRangeDone | ((own_chunk && (w.tail & kTailLast) != 0u) ? kTailPending : 0u);
            continue;
        }
        ++units_done;
        const uint32_t gt = tile_begin + u;            // tile number in item order
        if (fine) { it = gt; cur = items[gt]; }        // single-tile items: numbered like the units, no search
        else while (gt >= cur.tile0 + cur.n_tiles) cur = items[++it]; // tickets only grow: the cursor moves forward
        const uint32_t k = gt - cur.tile0;
        const uint32_t g_begin = cur.g0 + (u == 0 ? first.goff : 0u);
        const uint32_t g_end = (gt == tile_last) ? cur.g0 + last.goff : cur.g1;

        if constexpr (FINE) {
            // The planes the unit needs: 12 of the 16 positions (fine_word) -- the successor slice's four sit in plane quads
            // sq and 4 + sq of the tile and stay in memory.
            const uint32_t slice_of = cur.bucket >> (8u + slice_bits); // bucket << 8 | successor byte; slice = bucket >> slice width
            const uint32_t order = (kFineOrders >> (slice_of * order_step)) & 63u; // (narrow slices: step 0, all take slice 0's)
            const uint32_t dup_filter = slice_of != 0u ? ~0u : 0u; // (fine_dup: positions 0..3 are the previous slice's)
            // Where the lanes read.  The window starts in lane group g0 of tile t0 and may reach into the next tile: all
            // wave-uniform, so the planes come through three scalar bases (quad q and quad 4 + q lie 4096 bytes apart, an
            // immediate offset either side of the middle) and ONE 32-bit offset per lane.  (A window at the very end of
            // the stream would reach past it: those lanes read the last tile instead, and `keep` hides them.)
            const uint32_t t0 = cur.group_abs >> 6, g0 = cur.group_abs & 63u;
            const uint32_t next_tile = t0 + 1u < n_tiles ? 64u * 16u : 0u; // bit of a lane's 16 * (g0 + its lane group) that says "next tile"
            const char *planes = reinterpret_cast<const char *>(scan_stream) + static_cast<uint64_t>(t0) * (4u * kTileCands) + 4096u;
            const char *plane0 = planes + ((order & 3u) << 10), *plane1 = planes + (((order >> 2) & 3u) << 10), *plane2 = planes + ((order >> 4) << 10);
            const uint32_t lo = cur.window & 0xFFFFu, hi = cur.window >> 16; // lo < 32: a window starts in its first lane group
            compared += static_cast<unsigned long long>(cur.last_cands) * (g_end - g_begin);
            if (cur.shape != 32u) {
                // ---- a SHORT unit: the last 64 * shape candidates of a successor-byte group, 32 / shape guides per pass ----
                // Lane l takes candidates [l * shape, (l + 1) * shape) of the window, i.e. field l % per of lane group
                // first + l / per: the same 16-byte loads, then one byte permute per plane spreads the field over the
                // whole register.  shape is 16 or 8: everything that depends on it is a shift or a select.
                const bool wide = cur.shape == 16u;
                const uint32_t shape = wide ? 16u : 8u, w_log = wide ? 4u : 3u, per_log = wide ? 1u : 2u, per = wide ? 2u : 4u;
                const uint32_t at16 = (g0 + (lane >> per_log)) << 4, sub = lane & (per - 1u);
                const uint32_t off = (at16 & 0x3F0u) + ((at16 & next_tile) << 3);
                const uint32_t sel = (wide ? 0x01000100u : 0u) + sub * (wide ? 0x02020202u : 0x01010101u);
                uint32_t c[24];
                {
                    const uint4 a0 = *reinterpret_cast<const uint4 *>(plane0 - 4096 + off), a1 = *reinterpret_cast<const uint4 *>(plane1 - 4096 + off);
                    const uint4 a2 = *reinterpret_cast<const uint4 *>(plane2 - 4096 + off);
                    const uint4 b0 = *reinterpret_cast<const uint4 *>(plane0 + off), b1 = *reinterpret_cast<const uint4 *>(plane1 + off);
                    const uint4 b2 = *reinterpret_cast<const uint4 *>(plane2 + off);
                    const uint4 t6[6] = {a0, a1, a2, b0, b1, b2};
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        c[4 * q + 0] = __builtin_amdgcn_perm(0u, t6[q].x, sel); c[4 * q + 1] = __builtin_amdgcn_perm(0u, t6[q].y, sel);
                        c[4 * q + 2] = __builtin_amdgcn_perm(0u, t6[q].z, sel); c[4 * q + 3] = __builtin_amdgcn_perm(0u, t6[q].w, sel);
                    }
                }
                // the lane's candidates that are the item's: window offsets [lo, hi), the same for every guide field: bits
                // [from, to) of the field, both clamped to it
                const int mine0 = static_cast<int>(lane << w_log), width = static_cast<int>(shape);
                const int from = min(max(static_cast<int>(lo) - mine0, 0), width), to = min(max(static_cast<int>(hi) - mine0, 0), width);
                const uint32_t keep = ((1u << to) - (1u << from)) * (wide ? 0x00010001u : 0x01010101u);
                // (candidate q of the lane sits at window offset lane * shape + q: 32 * its lane group + shape * sub)
                const RecLane rl = rec_lane_at(cur.group_abs, lane << w_log);
                for (uint32_t gb = g_begin; gb < g_end; gb += 8u * per) { // 8 passes' masks at a time
                    __builtin_amdgcn_wave_barrier();
                    short_unit_masks(gword_stream, gb, wide, lane, wave_masks);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const uint32_t passes = (g_end - gb + per - 1u) >> per_log;
                    for (uint32_t i = 0; i < (passes < 8u ? passes : 8u); ++i) {
                        PrevSlice prev;
                        const uint32_t ok = near_plane12_masks<THR>(c, wave_masks + i * 8u, thr, keep, prev);
                        if (__ballot(ok != 0u) != 0ull) {
                            note_candidates<TAIL && LEAN>(fine_dup(ok, prev, dup_filter), 0u, reinterpret_cast<const uint32_t *>(wave_masks + i * 8u) + kPassIds, w_log, rl, lane, w, raw,
                                            raw_used, max_chunks, counters);
                            own_chunk = true;
                        }
                    }
                }
                continue;
            }
            // ---- a full unit: 2048 consecutive candidates of the bucket from lane group cur.group_abs on; lane l takes the
            // 32 of group (first + l).
            const uint32_t at16 = (g0 + lane) << 4;
            const uint32_t off = (at16 & 0x3F0u) + ((at16 & next_tile) << 3);
            uint32_t c[24];
            {
                const uint4 a0 = *reinterpret_cast<const uint4 *>(plane0 - 4096 + off), a1 = *reinterpret_cast<const uint4 *>(plane1 - 4096 + off);
                const uint4 a2 = *reinterpret_cast<const uint4 *>(plane2 - 4096 + off);
                const uint4 b0 = *reinterpret_cast<const uint4 *>(plane0 + off), b1 = *reinterpret_cast<const uint4 *>(plane1 + off);
                const uint4 b2 = *reinterpret_cast<const uint4 *>(plane2 + off);
                c[0] = a0.x; c[1] = a0.y; c[2] = a0.z; c[3] = a0.w; c[4] = a1.x; c[5] = a1.y; c[6] = a1.z; c[7] = a1.w;
                c[8] = a2.x; c[9] = a2.y; c[10] = a2.z; c[11] = a2.w;
                c[12] = b0.x; c[13] = b0.y; c[14] = b0.z; c[15] = b0.w; c[16] = b1.x; c[17] = b1.y; c[18] = b1.z; c[19] = b1.w;
                c[20] = b2.x; c[21] = b2.y; c[22] = b2.z; c[23] = b2.w;
            }
            // the lane's candidates that are the item's: offsets [lo, hi) of the unit.  lo touches lane 0 alone; of hi the lane
            // keeps its first clamp(hi - 32 * lane, 0, 32) candidates: the high word of 32 ones shifted up by that many.
            const int to = min(max(static_cast<int>(hi) - static_cast<int>(lane << 5), 0), 32);
            const uint32_t keep = static_cast<uint32_t>((0xFFFFFFFFull << to) >> 32) & (lane == 0u ? ~0u << lo : ~0u);
            const RecLane rl = rec_lane_at(cur.group_abs, lane << 5);
            if (stamps) { // diagnostics: how long the planes take to arrive once they are requested
                const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                plane_wait += __builtin_amdgcn_s_memrealtime() - t1;
            }
            if constexpr (THR < 0) {
                // The runtime-threshold build (max_dist 5, the scan_generic knob): one loop, every guide's budget from the class
                // bits of its word -- thr minus the 0, 1 or 2 mismatches it has in the successor slice.
                for (uint32_t g = g_begin; g < g_end; g += kGuideGroup) {
                    const FineSlotGroup gg = *reinterpret_cast<const FineSlotGroup *>(gword_stream + g);
#pragma unroll
                    for (uint32_t uu = 0; uu < kGuideGroup; ++uu) {
                        if (g + uu >= g_end) break;
                        const uint32_t cls = (gg.s[uu].word >> 24) & 3u;
                        if (cls > thr) continue;
                        PrevSlice prev;
                        const uint32_t ok = near_plane12<-1>(c, gg.s[uu].word, thr - cls, keep, prev);
                        if (__ballot(ok != 0u) != 0ull) {
                            note_candidates<TAIL && LEAN>(fine_dup(ok, prev, dup_filter), gg.s[uu].id, nullptr, 5u, rl, lane, w, raw, raw_used, max_chunks, counters);
                            own_chunk = true;
                        }
                    }
                }
                continue;
            }
            // class 1 (one mismatch in the successor slice): budget THR - 1 over the 12 positions; then class 0: budget THR
            const uint32_t gmid = cur.gmid < g_begin ? g_begin : cur.gmid > g_end ? g_end : cur.gmid;
            if constexpr (THR >= 1) {
                {
                    for (uint32_t g = g_begin; g < gmid; g += kGuideGroup) {
                        const FineSlotGroup gg = *reinterpret_cast<const FineSlotGroup *>(gword_stream + g);
#pragma unroll
                        for (uint32_t uu = 0; uu < kGuideGroup; ++uu) {
                            if (g + uu >= gmid) break;
                            PrevSlice prev;
                            const uint32_t ok = near_plane12<(THR < 1 ? 0 : THR - 1)>(c, gg.s[uu].word, thr - 1u, keep, prev);
                            if (__ballot(ok != 0u) != 0ull) {
                                note_candidates<TAIL && LEAN>(fine_dup(ok, prev, dup_filter), gg.s[uu].id, nullptr, 5u, rl, lane, w, raw, raw_used, max_chunks, counters);
                                own_chunk = true;
                            }
                        }
                    }
                }
            }
            for (uint32_t g = gmid; g < g_end; g += kGuideGroup) {
                const FineSlotGroup gg = *reinterpret_cast<const FineSlotGroup *>(gword_stream + g);
#pragma unroll
                for (uint32_t uu = 0; uu < kGuideGroup; ++uu) {
                    if (g + uu >= g_end) break;
                    PrevSlice prev;
                    const uint32_t ok = near_plane12<THR>(c, gg.s[uu].word, thr, keep, prev);
                    if (__ballot(ok != 0u) != 0ull) {
                        note_candidates<TAIL && LEAN>(fine_dup(ok, prev, dup_filter), gg.s[uu].id, nullptr, 5u, rl, lane, w, raw, raw_used, max_chunks, counters);
                        own_chunk = true;
                    }
                }
            }
            continue;
        }

        // ---- one tile: 2048 candidates, tile k of the item, guide slots [g_begin, g_end) -----------
        // The unit: 2048 consecutive candidates of the bucket from lane group cur.group_abs + 64 k on; lane l takes the
        // 32 of group (first + l).  Bucket-level items start on a tile; a window of the pruned scan may start on any lane
        // group and then straddles two tiles -- the same eight 16-byte loads per lane, from two places.  (A window at the
        // very end of the stream would reach past it: those lanes read the last tile instead, and `keep` hides them.)
        const uint32_t glane = cur.group_abs + (k << 6) + lane;
        const uint32_t tile = __builtin_amdgcn_readfirstlane(glane >> 6), grp = lane; // (whole tiles: uniform)
        // comparisons made here: the unit's real candidates (only a bucket's last one is short) x the real guides
        compared += static_cast<unsigned long long>((k + 1u == cur.n_tiles) ? cur.last_cands : kTileCands) * (g_end - g_begin);
        const uint4 *__restrict__ src =
            reinterpret_cast<const uint4 *>(scan_stream + static_cast<uint64_t>(tile) * kTileCands) + grp;
        uint32_t c[kPlanes];
#pragma unroll
        for (int q = 0; q < kPlanes / 4; ++q) {
            const uint4 t4 = src[q * 64];
            c[4 * q + 0] = t4.x; c[4 * q + 1] = t4.y; c[4 * q + 2] = t4.z; c[4 * q + 3] = t4.w;
        }
        // the lane's candidates that are the item's: offsets [lo, hi) of the tile
        const int lo = (k == 0u) ? static_cast<int>(cur.window & 0xFFFFu) : 0;
        const int hi = (k + 1u == cur.n_tiles) ? static_cast<int>(cur.window >> 16) : static_cast<int>(kTileCands);
        const int below = lo - static_cast<int>(lane * 32u), upto = hi - static_cast<int>(lane * 32u);
        const uint32_t keep = (below <= 0 ? ~0u : below >= 32 ? 0u : ~0u << below) &
                              (upto >= 32 ? ~0u : upto <= 0 ? 0u : ~0u >> (32 - upto));
        const RecLane rl = rec_lane(tile, grp * 32u);
        if (stamps) { // diagnostics: how long the planes take to arrive once they are requested
            const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            plane_wait += __builtin_amdgcn_s_memrealtime() - t1;
        }
        // Guide slots are padded to groups of 8 with a word (all T); the padding slots behind the last guide are skipped
        // below, one that does come near a real candidate would be dropped by k_verify.
        for (uint32_t g = g_begin; g < g_end; g += kGuideGroup) {
            const GuideGroup gg = *reinterpret_cast<const GuideGroup *>(gword_stream + g);
#pragma unroll
            for (uint32_t uu = 0; uu < kGuideGroup; ++uu) {
                if (g + uu >= g_end) break; // padding slots of the bucket's last group (scalar test, not taken: free)
                const uint32_t ok = near_plane<THR>(c, gg.w[uu], thr, keep);
                if (__ballot(ok != 0u) != 0ull) { // ~4 % of the (guide, tile) pairs on random data
                    note_candidates(ok, g + uu, nullptr, 5u, rl, lane, w, raw, raw_used, max_chunks, counters);
                    own_chunk = true;
                }
            }
        }
    }
    if constexpr (FINE && TAIL) {
        if ((w.tail & kTailOn) != 0u && lane == 0 && wave_runs()[kRunCursor + 2u] != 0u) atomicAdd(&vc.counters->scan_verified, wave_runs()[kRunCursor + 2u]);
    }
    if constexpr (lds) {
        // what the host and k_verify have to know of the buffers: the chunks' worth of records that never took a chunk, and the
        // last chunk that holds any
        if (lane == 0 && wave_bufs()[kBufDrained] != 0u) atomicAdd(&counters->lds_chunks, wave_bufs()[kBufDrained]);
        if (lane == 0 && wave_bufs()[kBufTop] != 0u) atomicMax(&counters->raw_top, wave_bufs()[kBufTop]);
    }
    // the launch's own end: behind the tails, by the workgroup's last wave
    if (tail_launch && lane == 0 && atomicAdd(tails_done_p, 1u) == (blockDim.x >> 6) - 1u)
        atomicMax(span + 1, static_cast<unsigned long long>(__builtin_amdgcn_s_memrealtime()));
    if (stamps && lane == 0) {
        stamps[4 * wave_id] = t_start;
        stamps[4 * wave_id + 1] = __builtin_amdgcn_s_memrealtime();
        stamps[4 * wave_id + 2] = (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11))) << 32) |
                                  __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); // XCC_ID, HW_ID
        stamps[4 * wave_id + 3] = units_done | (plane_wait << 32);
    }
}

// INVARIANT: `vc` is the FIRST parameter.  scan_tail reads it at offset 0 of the kernel-argument segment (and checks what it
// finds there against `raw` and `raw_used`).
// LEAN (with TAIL): the build for a lean batch (Workspace::lean_tail), whose waves on the pruned plan note into LDS and
// verify from there; every other batch runs the build whose records go through the raw buffer, as they always did.
template <int THR, bool TAIL, bool LEAN>
__global__ __launch_bounds__(1024, 8) void k_scan(VerifyCtx vc,
                                                  const uint32_t *__restrict__ scan_stream,
                                                  const ScanItem *__restrict__ items_full,
                                                  const ScanItem *__restrict__ items_fine,
                                                  const PlanInfo *__restrict__ plan,
                                                  const RangeStart *__restrict__ range_start,
                                                  const uint32_t *__restrict__ gword_full,
                                                  const FineSlot *__restrict__ gword_fine, uint64_t *raw,
                                                  uint32_t *raw_used, uint32_t max_chunks, Counters *counters, uint32_t thr,
                                                  unsigned long long *stamps, uint64_t *__restrict__ scan_count,
                                                  unsigned long long *span, uint32_t n_tiles, uint32_t slice_bits)
{
    __shared__ uint32_t next_unit;
    __shared__ uint32_t waves_done;
    __shared__ uint32_t tails_done;
    __shared__ unsigned long long wg_compared;
    __shared__ uint4 tail_masks[16][64]; // per wave: the guide masks of 8 passes of a short unit (short_unit_masks)
    // stamps (diagnostics, normally null): per wave {start, end} in 100 MHz ticks, {XCC_ID, HW_ID} and the number of
    // tiles it took; nothing else reads them
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { next_unit = 0; waves_done = 0; wg_compared = 0ull; if (TAIL) tails_done = 0; }
    __syncthreads();
    if (blockIdx.x >= plan->n_ranges) {
        if (threadIdx.x == 0) scan_count[blockIdx.x] = 0ull;
        return;
    }
    if (threadIdx.x == 0) atomicMin(span, t_start); // the launch's own span: first workgroup in, last one out
    // the plan of this batch: bucket-level items, or the successor-byte groups of the pruned scan (k_fine_plan)
    if (plan->fine != 0u)
        scan_range<THR, true, TAIL, LEAN>(scan_stream, items_fine, plan, range_start, gword_fine, tail_masks[threadIdx.x >> 6], raw, raw_used, max_chunks, counters, thr, stamps,
                              scan_count, &next_unit, &waves_done, &wg_compared, t_start, span, n_tiles, slice_bits, vc, &tails_done);
    else
        scan_range<THR, false, TAIL, LEAN>(scan_stream, items_full, plan, range_start, gword_full, tail_masks[threadIdx.x >> 6], raw, raw_used, max_chunks, counters, thr, stamps,
                               scan_count, &next_unit, &waves_done, &wg_compared, t_start, span, n_tiles, slice_bits, vc, &tails_done);
}

template <int THR>
static void launch_scan_thr(const ImageView &v, const Workspace &ws, const Tuning &tn, uint32_t thr, uint32_t prune_mode,
                            const VerifyCtx &vc, hipStream_t stream)
{
    // pruned scan: the items and guide words grouped by (bucket, successor byte); the plan says which list counts
    if (vc.scan_verify != 0u && vc.lean_tail != 0u && prune_mode != 0u)
        hipLaunchKernelGGL((k_scan<THR, true, true>), dim3(tn.scan_blocks), dim3(tn.scan_threads), 0, stream, vc, v.scan, ws.items,
                           ws.fitems, ws.plan, ws.range_start, ws.gword, ws.fword,
                           ws.raw, ws.raw_used, static_cast<uint32_t>(ws.cap_chunks), ws.counters, thr, ws.stamps, ws.scan_count,
                           ws.scan_span + 2u * ws.span_slot, v.n_tiles, v.slice_width);
    else if (vc.scan_verify != 0u)
        hipLaunchKernelGGL((k_scan<THR, true, false>), dim3(tn.scan_blocks), dim3(tn.scan_threads), 0, stream, vc, v.scan, ws.items,
                           prune_mode ? ws.fitems : ws.items, ws.plan, ws.range_start, ws.gword, ws.fword,
                           ws.raw, ws.raw_used, static_cast<uint32_t>(ws.cap_chunks), ws.counters, thr, ws.stamps, ws.scan_count,
                           ws.scan_span + 2u * ws.span_slot, v.n_tiles, v.slice_width);
    else
        hipLaunchKernelGGL((k_scan<THR, false, false>), dim3(tn.scan_blocks), dim3(tn.scan_threads), 0, stream, vc, v.scan, ws.items,
                           prune_mode ? ws.fitems : ws.items, ws.plan, ws.range_start, ws.gword, ws.fword,
                           ws.raw, ws.raw_used, static_cast<uint32_t>(ws.cap_chunks), ws.counters, thr, ws.stamps, ws.scan_count,
                           ws.scan_span + 2u * ws.span_slot, v.n_tiles, v.slice_width);
}

void launch_scan(const ImageView &v, const Workspace &ws, const Tuning &tn, const uint64_t *d_guides, uint32_t n,
                 const ScoreParams &p, uint32_t prune_mode, void *stream_)
{
    const int max_dist = p.max_dist;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (max_dist < 0) { // isslScoreOfftargets.cpp:382: no distance satisfies 0 <= dist <= maxDist -- nothing is compared
        (void)hipMemsetAsync(ws.scan_count, 0, 8ull * tn.scan_blocks, stream);
        return;
    }
    const uint32_t thr = max_dist > 31 ? 31u : static_cast<uint32_t>(max_dist);
    const VerifyCtx vc = make_verify_ctx(v, ws, tn, d_guides, n, p); // the waves' verify tail (scan_tail)
    // the runtime-threshold build serves max_dist > 4 (and, forced by the scan_generic knob, the tests of that build)
    if (tn.scan_generic || thr > 4) launch_scan_thr<-1>(v, ws, tn, thr, prune_mode, vc, stream);
    else if (thr == 0) launch_scan_thr<0>(v, ws, tn, thr, prune_mode, vc, stream);
    else if (thr == 1) launch_scan_thr<1>(v, ws, tn, thr, prune_mode, vc, stream);
    else if (thr == 2) launch_scan_thr<2>(v, ws, tn, thr, prune_mode, vc, stream);
    else if (thr == 3) launch_scan_thr<3>(v, ws, tn, thr, prune_mode, vc, stream);
    else launch_scan_thr<4>(v, ws, tn, thr, prune_mode, vc, stream);
}

} // namespace issl
