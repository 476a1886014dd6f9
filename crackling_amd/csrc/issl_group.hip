// Hit grouping: the keys that lie beyond their guide's hit slots, sorted by guide (counting sort over a device-wide prefix sum).
#include <hip/hip_runtime.h>

#include "issl_kernels.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// hit grouping: counting sort of the keys by guide
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_prefix_block_sums(const uint32_t *__restrict__ in, uint32_t n,
                                                           uint32_t *__restrict__ sums, uint32_t slot_hits)
{
    short_kernel_priority();
    __shared__ uint64_t lds[256];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * 8u;
    uint64_t s = 0;
    for (uint32_t i = 0; i < 8; ++i)
        if (base + i < n) s += grouped_hits(in[base + i], slot_hits);
    uint64_t total;
    (void)block_exclusive_scan(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = static_cast<uint32_t>(total);
}

__global__ __launch_bounds__(256) void k_prefix_of_sums(uint32_t *__restrict__ sums, uint32_t n_blocks)
{
    short_kernel_priority();
    __shared__ uint64_t lds[256];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t val = i < n_blocks ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(val, lds, &total);
        if (i < n_blocks) sums[i] = static_cast<uint32_t>(carry + ex);
        carry += total;
    }
}

__global__ __launch_bounds__(256) void k_prefix_apply(const uint32_t *__restrict__ in, uint32_t n,
                                                      const uint32_t *__restrict__ sums, uint32_t *__restrict__ out,
                                                      uint32_t *__restrict__ big, Counters *__restrict__ counters,
                                                      uint32_t slot_hits)
{
    short_kernel_priority();
    __shared__ uint64_t lds[256];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * 8u;
    uint32_t val[8];
    uint64_t s = 0;
    uint32_t nb = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t c = (base + i < n) ? in[base + i] : 0u;
        nb += c > kReplayLds;
        val[i] = grouped_hits(c, slot_hits);
        s += val[i];
    }
    if (nb != 0u) { // guides for k_replay_mid / k_replay_big: one reservation per thread
        uint32_t at = atomicAdd(&counters->n_big, nb);
        for (uint32_t i = 0; i < 8; ++i)
            if (base + i < n && in[base + i] > kReplayLds) big[at++] = base + i;
    }
    uint64_t run = block_exclusive_scan(s, lds, nullptr) + sums[blockIdx.x];
    for (uint32_t i = 0; i < 8; ++i) {
        if (base + i < n) out[base + i] = static_cast<uint32_t>(run);
        run += val[i];
    }
}

// Whole prefix sum in one workgroup (used while n is moderate; saves two launches): every thread sums its own run of
// consecutive counts (16-byte loads), ONE scan over the 1024 run totals, then every thread writes its run's prefixes --
// two barriers in all, where a loop over chunks of 4096 counts paid three per chunk (0.06 ms at 100 k guides).  The list
// of guides with more than kReplayLds hits comes out of the same scan (their number rides in a second scanned word), in
// guide order and without an atomic: on indexes where most guides are such (skewed genomes, the 3 G-line index) one
// returning atomic per guide from a single workgroup cost more than the rest of the grouping (2 ms per 100 k guides).
// With hit slots only those guides have anything in the grouped arrays (grouped_hits), and when k_verify saw no guide
// outgrow its slots there is nothing to do at all.
__global__ __launch_bounds__(1024) void k_prefix_single(const uint32_t *__restrict__ in, uint32_t n,
                                                        uint32_t *__restrict__ out, uint32_t *__restrict__ big,
                                                        Counters *__restrict__ counters, uint32_t slot_hits)
{
    short_kernel_priority();
    if (slot_hits >= kReplayLds && counters->overflowed == 0u) return; // (n_big stays 0: k_group_scatter and the replays of many-hit guides return at once)
    __shared__ uint32_t wave_sum[16], wave_big[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per = ((n + 1023u) / 1024u + 3u) & ~3u; // counts per thread, a multiple of 4: the runs start 16-byte aligned
    const uint32_t i0 = threadIdx.x * per;
    uint32_t s = 0, b = 0;
    for (uint32_t k = 0; k < per; k += 4) {
        const uint32_t i = i0 + k;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (i + 3 < n) q = *reinterpret_cast<const uint4 *>(in + i);
        else { if (i < n) q.x = in[i]; if (i + 1 < n) q.y = in[i + 1]; if (i + 2 < n) q.z = in[i + 2]; }
        s += grouped_hits(q.x, slot_hits) + grouped_hits(q.y, slot_hits) + grouped_hits(q.z, slot_hits) + grouped_hits(q.w, slot_hits);
        b += (q.x > kReplayLds) + (q.y > kReplayLds) + (q.z > kReplayLds) + (q.w > kReplayLds);
    }
    uint32_t x = s, xb = b; // inclusive scans of s and b inside the wave
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64), yb = __shfl_up(xb, d, 64);
        if (lane >= d) { x += y; xb += yb; }
    }
    if (lane == 63) { wave_sum[wave] = x; wave_big[wave] = xb; }
    __syncthreads();
    uint32_t run = x - s, brun = xb - b;
    for (uint32_t wv = 0; wv < wave; ++wv) { run += wave_sum[wv]; brun += wave_big[wv]; }
    if (threadIdx.x == 1023u) counters->n_big = brun + b;
    for (uint32_t k = 0; k < per; k += 4) {
        const uint32_t i = i0 + k;
        if (i >= n) break;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (i + 3 < n) q = *reinterpret_cast<const uint4 *>(in + i);
        else { q.x = in[i]; if (i + 1 < n) q.y = in[i + 1]; if (i + 2 < n) q.z = in[i + 2]; }
        const uint32_t ex = grouped_hits(q.x, slot_hits), ey = grouped_hits(q.y, slot_hits), ez = grouped_hits(q.z, slot_hits),
                       ew = grouped_hits(q.w, slot_hits);
        const uint4 o = make_uint4(run, run + ex, run + ex + ey, run + ex + ey + ez);
        if (i + 3 < n) *reinterpret_cast<uint4 *>(out + i) = o;
        else { out[i] = o.x; if (i + 1 < n) out[i + 1] = o.y; if (i + 2 < n) out[i + 2] = o.z; }
        run += ex + ey + ez + ew;
        if (q.x > kReplayLds) big[brun++] = i; // guides for k_replay_mid / k_replay_big
        if (q.y > kReplayLds) big[brun++] = i + 1;
        if (q.z > kReplayLds) big[brun++] = i + 2;
        if (q.w > kReplayLds) big[brun++] = i + 3;
    }
}

// (One 32-byte record {key, terms, rank} per hit instead of the three arrays -- written by k_verify, moved by this
// kernel, read by the replay -- was measured in round 3: verify +7 %, this kernel +35 %: the passes are bound by the
// bytes they move, not by the number of streams; profiles/r03_ab_hit_records.log.)
__global__ __launch_bounds__(kChunkRecs) void k_group_scatter(const uint64_t *__restrict__ raw,
                                                              const uint32_t *__restrict__ raw_used,
                                                              const Counters *__restrict__ counters, uint32_t cap_chunks,
                                                              const uint32_t *__restrict__ gcount,
                                                              const uint32_t *__restrict__ goff,
                                                              const uint32_t *__restrict__ rank,
                                                              const double2 *__restrict__ pay,
                                                              uint64_t *__restrict__ sorted, double2 *__restrict__ terms,
                                                              uint32_t slot_hits)
{
    short_kernel_priority();
    // hit slots: only guides with more hits than fit their slots left anything to group -- on an even index none
    if (slot_hits >= kReplayLds && counters->n_big == 0u) return;
    uint32_t n_chunks = counters->raw_chunks;
    if (n_chunks > cap_chunks) n_chunks = cap_chunks;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        // (everything that does not depend on the key is asked for at once: the pass is a chain of dependent loads)
        const uint64_t *recs = raw + static_cast<uint64_t>(chunk) * kChunkRecs;
        const uint32_t t = threadIdx.x + 1u;
        const uint64_t slot = static_cast<uint64_t>(chunk) * (kChunkRecs - 1u) + (threadIdx.x < kChunkRecs - 1u ? threadIdx.x : kChunkRecs - 2u);
        const uint64_t key = recs[t < kChunkRecs ? t : 0u];
        const uint32_t my_rank = rank[slot];
        const double2 my_pay = pay[slot];
        const uint32_t used = raw_used[chunk] & ~kChunkVerified; // (a chunk its scan wave verified: the same keys, ranks and terms as k_verify leaves)
        if (t >= used || t >= kChunkRecs || key == kDeadKey) continue;
        const uint32_t guide = static_cast<uint32_t>(key >> kKeyGuideShift);
        const uint32_t to = goff[guide] + my_rank; // rank: k_verify's
        sorted[to] = key;
        if (gcount[guide] <= kMidHits) terms[to] = my_pay; // (the many-hit replay makes its own)
    }
}

void launch_group_hits(const Workspace &ws, uint32_t n, void *stream_)
{
    if (ws.lean_tail) return; // (predicted: no guide beyond its hit slots, nothing to group; k_replay checks)
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t m = n + 1; // gcount[n] = 0 so that goff[n] = total
    if (m <= (1u << 18)) {
        hipLaunchKernelGGL(k_prefix_single, dim3(1), dim3(1024), 0, stream, ws.gcount, m, ws.goff, ws.gcur_big,
                           ws.counters, ws.slot_hits);
    } else {
        const uint32_t blocks = (m + kScanChunk - 1) / kScanChunk;
        hipLaunchKernelGGL(k_prefix_block_sums, dim3(blocks), dim3(256), 0, stream, ws.gcount, m, ws.blocksum, ws.slot_hits);
        hipLaunchKernelGGL(k_prefix_of_sums, dim3(1), dim3(256), 0, stream, ws.blocksum, blocks);
        hipLaunchKernelGGL(k_prefix_apply, dim3(blocks), dim3(256), 0, stream, ws.gcount, m, ws.blocksum, ws.goff,
                           ws.gcur_big, ws.counters, ws.slot_hits);
    }
    hipLaunchKernelGGL(k_group_scatter, dim3(kTailGrid), dim3(kChunkRecs), 0, stream, ws.raw, ws.raw_used, ws.counters,
                       static_cast<uint32_t>(ws.cap_chunks), ws.gcount, ws.goff, ws.rank, reinterpret_cast<const double2 *>(ws.pay),
                       ws.sorted, reinterpret_cast<double2 *>(ws.terms), ws.slot_hits);
}

} // namespace issl
