// Off-target report: per-guide profile by distance, and the expanded record list.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "issl_kernels.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// off-target report: profile by distance, record list
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x)
{
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(x), d, 64), hi = __shfl_xor(static_cast<uint32_t>(x >> 32), d, 64);
        x += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return x;
}

// The profile stands where the replay stands, and splits the guides as it does: THREADS == 64, one wave per guide, every
// guide of up to kReplayLds hits (k_replay's); THREADS == 256, one workgroup per entry of the many-hit guide list the
// grouping pass made (k_replay_mid's and k_replay_big's).  A bin does not depend on the order of the hits, so nothing is
// ranked: hit r of a guide is slot r of its hit slots (distance and count in SlotRec::pad, k_verify) or, beyond them
// and on batches without slots, key r of its grouped segment, whose site is read again.  Every lane counts its own hits
// in registers; the wave adds them up with shuffles, the workgroup through LDS: no atomic per hit.
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void k_profile(ImageView v, Workspace ws, const uint64_t *__restrict__ guides, uint32_t n,
                                                      issl_profile *__restrict__ out)
{
    short_kernel_priority();
    constexpr bool BIG = THREADS > 64u;
    constexpr uint32_t WAVES = THREADS / 64u;
    __shared__ uint32_t part_sites[WAVES][ISSL_PROFILE_BINS + 1];
    __shared__ uint64_t part_occ[WAVES][ISSL_PROFILE_BINS + 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // (what k_replay tells the host: a guide beyond its hit slots; a batch enqueued without the grouping pass is run again)
    if (!BIG && blockIdx.x == 0 && lane == 0 && ws.counters->overflowed != 0u) atomicOr(&ws.sticky[0], ws.lean_tail ? 6u : 4u);
    const uint32_t n_work = BIG ? ws.counters->n_big : n;
    for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const uint32_t g = BIG ? ws.gcur_big[w] : w;
        const uint32_t h = ws.gcount[g];
        if (!BIG && h > kReplayLds) continue;
        const uint32_t in_slots = h < ws.slot_hits ? h : ws.slot_hits;
        const SlotRec *__restrict__ srec = ws.slots + static_cast<uint64_t>(g) * ws.slot_hits;
        uint32_t sites[ISSL_PROFILE_BINS] = {};
        uint64_t occs[ISSL_PROFILE_BINS] = {};
        auto count = [&](uint32_t dist, uint32_t occ) {
#pragma unroll
            for (uint32_t d = 0; d < ISSL_PROFILE_BINS; ++d) {
                sites[d] += dist == d ? 1u : 0u;
                occs[d] += dist == d ? occ : 0u;
            }
        };
        for (uint32_t i = threadIdx.x; i < in_slots; i += THREADS) {
            const uint64_t pad = srec[i].pad;
            count(static_cast<uint32_t>(pad >> 32), static_cast<uint32_t>(pad));
        }
        if (h > in_slots) {
            const uint64_t gsig = guides[g];
            const uint64_t *__restrict__ keys = ws.sorted + ws.goff[g];
            for (uint32_t i = in_slots + threadIdx.x; i < h; i += THREADS) {
                const issl_hit rec = hit_terms(v, gsig, g, keys[i], false, false, false).rec;
                count(rec.dist, rec.occ);
            }
        }
#pragma unroll
        for (uint32_t d = 0; d < ISSL_PROFILE_BINS; ++d) {
            const uint32_t s = wave_sum_u32(sites[d]);
            const uint64_t o = wave_sum_u64(occs[d]);
            if (lane == d) { part_sites[wave][d] = s; part_occ[wave][d] = o; }
        }
        __syncthreads();
        if (threadIdx.x < ISSL_PROFILE_BINS) {
            uint32_t s = 0;
            uint64_t o = 0;
            for (uint32_t k = 0; k < WAVES; ++k) { s += part_sites[k][threadIdx.x]; o += part_occ[k][threadIdx.x]; }
            out[g].sites[threadIdx.x] = s;
            out[g].occurrences[threadIdx.x] = o;
        } else if (threadIdx.x == ISSL_PROFILE_BINS) {
            out[g].pad = 0u;
        }
        __syncthreads();
    }
}

void launch_profile(const ImageView &v, const Workspace &ws, const uint64_t *d_guides, uint32_t n, issl_profile *d_out,
                    void *stream)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_profile<64>, dim3(n < 65536u ? n : 65536u), dim3(64), 0, static_cast<hipStream_t>(stream), v, ws,
                       d_guides, n, d_out);
    if (ws.lean_tail) return; // (predicted: no guide with more than kReplayLds hits; the kernel above checks)
    hipLaunchKernelGGL(k_profile<256>, dim3(2048), dim3(256), 0, static_cast<hipStream_t>(stream), v, ws, d_guides, n, d_out);
}

__global__ __launch_bounds__(256) void k_report_offsets(const uint32_t *__restrict__ goff, uint32_t n, uint64_t base,
                                                        uint64_t *__restrict__ offsets)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= n; i += gridDim.x * 256u) offsets[i] = base + goff[i];
}

// One record per thread: the site's signature is read where k_verify read it, the terms are k_verify's own arithmetic
// (score_terms) on the same three inputs.  The 40-byte records of a workgroup leave through LDS as one run of 8-byte
// words, so that every store instruction of a wave covers 512 consecutive bytes.
constexpr uint32_t kEmitWords = sizeof(issl_offtarget) / 8u;
static_assert(sizeof(issl_offtarget) == 40 && sizeof(issl_profile) == 88, "report structs: include/issl_hip.h");
__global__ __launch_bounds__(256) void k_report_emit(ImageView v, const uint64_t *__restrict__ guides,
                                                     const issl_hit *__restrict__ hits, uint32_t n_records,
                                                     uint32_t guide_base, uint64_t *__restrict__ out_words)
{
    __shared__ uint64_t stage[256u * kEmitWords];
    const uint64_t low = (1ull << v.slice_width) - 1ull;
    for (uint32_t first = blockIdx.x * 256u; first < n_records; first += gridDim.x * 256u) {
        const uint32_t i = first + threadIdx.x;
        if (i < n_records) {
            const issl_hit h = hits[i];
            const uint64_t gsig = guides[h.guide];
            uint64_t ot;
            if (v.occ8) { // site table in host memory: the signature from the scan planes, as k_verify has it
                const uint32_t bucket = (h.slice << v.slice_width) + static_cast<uint32_t>((gsig >> (v.slice_width * h.slice)) & low);
                ot = candidate_signature(v, bucket, v.tile_first[bucket] + (h.pos >> 11), h.pos & (kTileCands - 1u));
            } else {
                ot = v.sites[h.id] & kSigMask;
            }
            double mit, cfd;
            int dist;
            score_terms(v, gsig, ot, h.occ, true, true, mit, cfd, dist);
            uint64_t *s = stage + threadIdx.x * kEmitWords;
            s[0] = ot;
            s[1] = static_cast<uint64_t>(__double_as_longlong(mit));
            s[2] = static_cast<uint64_t>(__double_as_longlong(cfd));
            s[3] = static_cast<uint64_t>(guide_base + h.guide) | (static_cast<uint64_t>(h.id) << 32);
            s[4] = static_cast<uint64_t>(h.occ) | (static_cast<uint64_t>(static_cast<uint32_t>(dist) & 0xFFFFu) << 32) |
                   (static_cast<uint64_t>(h.slice & 0xFFFFu) << 48);
        }
        __syncthreads();
        const uint32_t have = (n_records - first < 256u ? n_records - first : 256u) * kEmitWords;
        uint64_t *dst = out_words + static_cast<uint64_t>(first) * kEmitWords;
        for (uint32_t k = threadIdx.x; k < have; k += 256u) dst[k] = stage[k];
        __syncthreads();
    }
}

void launch_report_offsets(const Workspace &ws, uint32_t n, uint64_t base, uint64_t *d_offsets, void *stream)
{
    const uint32_t blocks = std::min<uint32_t>((n + 256u) / 256u, 4096u);
    hipLaunchKernelGGL(k_report_offsets, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), ws.goff, n, base, d_offsets);
}

void launch_report_emit(const ImageView &v, const Workspace &ws, const uint64_t *d_guides, uint32_t n_records,
                        uint32_t guide_base, issl_offtarget *d_out, void *stream)
{
    if (n_records == 0) return;
    const uint32_t blocks = std::min<uint32_t>((n_records + 255u) / 256u, 16384u);
    hipLaunchKernelGGL(k_report_emit, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), v, d_guides, ws.d_hitrec,
                       n_records, guide_base, reinterpret_cast<uint64_t *>(d_out));
}

} // namespace issl
