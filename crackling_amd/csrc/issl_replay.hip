// The three replays: a guide's hits in the reference's scan order, their terms added up with its early exit.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "issl_kernels.hpp"

namespace issl {

// ------------------------------------------------------------------------------------------------
// replay: ordered MIT/CFD accumulation, one wave per guide
// ------------------------------------------------------------------------------------------------

// Ascending sort of data[0..n) by the whole workgroup.  Bitonic network with every comparator
// ascending; comparators that touch an index >= n are no-ops (virtual +inf padding).
__device__ inline void wave_sort(uint64_t *data, uint32_t n)
{
    if (n < 2) return;
    uint32_t np = 1;
    while (np < n) np <<= 1;
    for (uint32_t k = 2; k <= np; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (np >> 1); t += blockDim.x) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); // bit log2(j) of i is 0
                const uint32_t l = (j == (k >> 1)) ? (i ^ (k - 1u)) : (i | j);
                if (l < n) {
                    const uint64_t a = data[i], b = data[l];
                    if (a > b) { data[i] = b; data[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ inline double bcast_f64(double x, int lane)
{
    const uint64_t u = __double_as_longlong(x);
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(u), lane);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(u >> 32), lane);
    return __longlong_as_double((static_cast<uint64_t>(hi) << 32) | lo);
}

// The value lane (l ^ M) holds, for the lane masks the network below uses.  Inside a row of 16 lanes a DPP modifier does
// it; across rows ds_swizzle (32-lane halves, no address register) or ds_bpermute_b32.
template <uint32_t M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x)
{
    const int xi = static_cast<int>(x);
    if constexpr (M == 1u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0xB1, 0xF, 0xF, false));       // quad_perm:[1,0,3,2]
    else if constexpr (M == 2u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0x4E, 0xF, 0xF, false));  // quad_perm:[2,3,0,1]
    else if constexpr (M == 3u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0x1B, 0xF, 0xF, false));  // quad_perm:[3,2,1,0]
    else if constexpr (M == 7u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0x141, 0xF, 0xF, false)); // row_half_mirror
    else if constexpr (M == 8u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0x128, 0xF, 0xF, false)); // row_ror:8
    else if constexpr (M == 15u) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(xi, xi, 0x140, 0xF, 0xF, false)); // row_mirror
    else if constexpr (M < 32u) return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(xi, static_cast<int>(0x1Fu | (M << 10)))); // and 31, or 0, xor M
    else return static_cast<uint32_t>(__shfl_xor(xi, static_cast<int>(M), 64));
}

template <uint32_t M>
__device__ __forceinline__ uint64_t lane_xor64(uint64_t x)
{
    return (static_cast<uint64_t>(lane_xor<M>(static_cast<uint32_t>(x >> 32))) << 32) | lane_xor<M>(static_cast<uint32_t>(x));
}

// One stage of the network below: element e = lane * R + r meets element e ^ X.  The bits of X below R pick the partner's
// register (resolved when the stage is compiled), the bits above it the partner's lane; the lower of the two elements --
// bit TOP of e clear -- keeps the smaller word.
template <uint32_t R, uint32_t X, uint32_t TOP>
__device__ __forceinline__ void sort_stage(uint64_t (&w)[R], uint32_t lane)
{
    constexpr uint32_t RX = X & (R - 1u), LX = X / R;
    if constexpr (LX == 0u) {
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            if ((r & TOP) == 0u) { // (TOP < R here: the pair is two registers of the lane)
                const uint64_t a = w[r], b = w[r ^ RX];
                const bool swap = a > b;
                w[r] = swap ? b : a;
                w[r ^ RX] = swap ? a : b;
            }
        }
    } else {
        const bool low = (lane & (TOP / R)) == 0u;
        uint64_t other[R];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) other[r] = lane_xor64<LX>(w[r ^ RX]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) w[r] = ((other[r] < w[r]) == low) ? other[r] : w[r];
    }
}

template <uint32_t R, uint32_t K, uint32_t J>
__device__ __forceinline__ void sort_merge(uint64_t (&w)[R], uint32_t lane)
{
    if constexpr (J >= 1u) {
        sort_stage<R, J, J>(w, lane); // e meets e | J
        sort_merge<R, K, J / 2u>(w, lane);
    }
}

template <uint32_t R, uint32_t K>
__device__ __forceinline__ void sort_level(uint64_t (&w)[R], uint32_t lane)
{
    if constexpr (K <= 64u * R) {
        sort_stage<R, K - 1u, K / 2u>(w, lane); // e meets e ^ (K - 1): two ascending runs of K / 2 become a bitonic pair of halves
        sort_merge<R, K, K / 4u>(w, lane);
        sort_level<R, 2u * K>(w, lane);
    }
}

// Ascending sort of the 64 * R distinct words the wave holds in registers, element lane * R + r in w[r] of `lane`: wave_sort's
// network (every comparator ascending) with the pairs that share a lane exchanged in registers and the others through
// lane_xor -- no LDS round trip and no index arithmetic per stage.  The words are distinct (a hit's index is in their low
// bits; padding words differ from every hit's), so a lane and its partner always agree on who keeps which.
template <uint32_t R>
__device__ __forceinline__ void wave_sort_regs(uint64_t (&w)[R], uint32_t lane)
{
    sort_level<R, 2u>(w, lane);
}

// Adds the terms of a chunk of cnt <= 64 hits to the running totals in walking order (:394, :460) and applies the exit test
// of :467-496 after every hit.  `chunk_lds`: the chunk's terms in LDS, {mit, cfd} per hit in walking order, zeros behind the
// last hit up to a multiple of 8; lane l also holds the terms of hit l (0.0 beyond cnt).  The sums are a serial chain of
// f64 additions -- the order is part of the result -- read from LDS, every lane the same 16 bytes: one load and two
// additions per hit (passing them from lane to lane through scalar registers cost four readlanes more; the walk shares
// its SIMD with seven other waves, what it costs is instructions: replay 0.37 -> 0.30 ms, 4.2 -> 3.5 on the skewed index).
// The exit test is not part of the chain: every lane keeps the totals as they stood after ITS hit, the tests run side by
// side afterwards, and the first lane that passes decides where the walk stops.  (Testing inside the chain costs a
// compare, a branch and their latencies per hit: ~200 cycles against ~50.)
// Returns true when the walk stops; `kept` counts the hits that were scored, the totals are those at that point.
// SPLIT (k_replay): in the first pass the even lanes add up the MIT terms and the odd lanes the CFD terms, 8
// bytes and ONE addition per lane and hit instead of 16 bytes and two -- each sum is the same chain of additions.
template <bool SPLIT>
__device__ __forceinline__ bool accumulate_chunk(double mit_term, double cfd_term, uint32_t cnt, const ScoreParams &p,
                                                 uint32_t lane, double &tot_mit, double &tot_cfd, uint32_t &kept,
                                                 const double2 *chunk_lds)
{
    auto passes = [&](double m, double c) {
        if (p.method == ISSL_METHOD_AND) return m > p.maximum_sum && c > p.maximum_sum;
        if (p.method == ISSL_METHOD_OR) return m > p.maximum_sum || c > p.maximum_sum;
        if (p.method == ISSL_METHOD_AVG) return ((m + c) / 2.0) > p.maximum_sum;
        if (p.method == ISSL_METHOD_MIT) return m > p.maximum_sum;
        if (p.method == ISSL_METHOD_CFD) return c > p.maximum_sum;
        return false;
    };
    // First the totals behind the chunk alone (the same additions in the same order).  Terms are products of
    // non-negative table values and counts, so the totals only grow and every exit test is monotone in them: when the
    // totals behind the chunk do not pass, no hit inside it did, and the per-hit bookkeeping below is not needed.  (A
    // table with a negative entry, or a NaN, takes the careful pass.)
    {
        double tm = tot_mit, tc = tot_cfd;
        if constexpr (SPLIT) {
            const double *half_lds = reinterpret_cast<const double *>(chunk_lds) + (lane & 1u);
            double acc = (lane & 1u) ? tot_cfd : tot_mit;
            for (uint32_t l0 = 0; l0 < cnt; l0 += 8) {
#pragma unroll
                for (uint32_t l = 0; l < 8; ++l) acc += half_lds[2u * (l0 + l)];
            }
            tm = bcast_f64(acc, 0);
            tc = bcast_f64(acc, 1);
        } else {
            for (uint32_t l0 = 0; l0 < cnt; l0 += 8) {
#pragma unroll
                for (uint32_t l = 0; l < 8; ++l) { // x + 0.0 == x: the zeros behind the last hit change nothing
                    const double2 t = chunk_lds[l0 + l];
                    tm += t.x;
                    tc += t.y;
                }
            }
        }
        const bool grows = __ballot(lane < cnt && !(mit_term >= 0.0 && cfd_term >= 0.0)) == 0ull;
        if (grows && !passes(tm, tc)) {
            kept += cnt;
            tot_mit = tm;
            tot_cfd = tc;
            return false;
        }
    }
    double tm = tot_mit, tc = tot_cfd, mine_m = 0.0, mine_c = 0.0;
    for (uint32_t l0 = 0; l0 < cnt; l0 += 8) {
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            const double2 t = chunk_lds[l0 + l];
            tm += t.x;
            tc += t.y;
            if (lane == l0 + l) { mine_m = tm; mine_c = tc; }
        }
    }
    const bool exit_here = passes(mine_m, mine_c);
    const uint64_t exits = __ballot(exit_here && lane < cnt);
    if (exits != 0ull) {
        const int first = __builtin_ctzll(exits);
        kept += static_cast<uint32_t>(first) + 1u;
        tot_mit = bcast_f64(mine_m, first);
        tot_cfd = bcast_f64(mine_c, first);
        return true;
    }
    kept += cnt;
    tot_mit = tm;
    tot_cfd = tc;
    return false;
}

template <bool DUMP>
__global__ __launch_bounds__(64, DUMP ? 4 : 8) void k_replay(ImageView v, Workspace ws, const uint64_t *__restrict__ guides,
                                               uint32_t n, ScoreParams p, double *__restrict__ out_mit,
                                               double *__restrict__ out_cfd, uint32_t *__restrict__ out_kept,
                                               issl_hit *__restrict__ hits_or_null)
{
    short_kernel_priority();
    issl_hit *const out_hits = DUMP ? hits_or_null : nullptr; // (the expanded records cost registers the plain replay does not pay for)
    __shared__ uint64_t keys[kReplayLds];
    __shared__ __attribute__((aligned(16))) double2 ord[64]; // the terms of the chunk being walked, in key order
    const bool calc_mit = p.method == ISSL_METHOD_MIT || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const bool calc_cfd = p.method == ISSL_METHOD_CFD || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const uint32_t lane = threadIdx.x;
    // A guide beyond its hit slots in this batch: the lane's next batches get the whole tail; a batch that was enqueued
    // WITHOUT it (Workspace::lean_tail) is run again.
    if (blockIdx.x == 0 && lane == 0 && ws.counters->overflowed != 0u) atomicOr(&ws.sticky[0], ws.lean_tail ? 6u : 4u);

    for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
        const uint32_t h = ws.gcount[g];
        if (h > kReplayLds) continue; // k_replay_mid's, k_replay_big's
        // the guide's keys and terms: in its hit slots, or (no slots: issl_dump_hits, ...) its segment of the grouped arrays
        const bool slots = ws.slot_hits >= kReplayLds;
        const uint32_t h0 = slots ? 0u : ws.goff[g];
        const SlotRec *__restrict__ srec = ws.slots + static_cast<uint64_t>(g) * ws.slot_hits;
        const uint64_t *__restrict__ skeys = ws.sorted + h0;
        const double2 *__restrict__ sterms = reinterpret_cast<const double2 *>(ws.terms) + h0;
        auto key_of = [&](uint32_t i) { return slots ? srec[i].key : skeys[i]; };
        auto terms_of = [&](uint32_t i) { return slots ? *reinterpret_cast<const double2 *>(&srec[i].mit) : sterms[i]; };
        const uint64_t gsig = guides[g];
        double tot_mit = 0.0, tot_cfd = 0.0;
        uint32_t kept = 0;
        bool stop = false;

        // Running totals in key order, same operations as the reference's (:394,:460), early exit of :467-496.
        auto accumulate = [&](double mit_term, double cfd_term, uint32_t cnt) {
            stop = accumulate_chunk<true>(mit_term, cfd_term, cnt, p, lane, tot_mit, tot_cfd, kept, ord);
        };

        // The terms of every hit were computed by k_verify and sit next to the keys (key_of / terms_of above);
        // what is left is putting them in key order and adding them up.  issl_dump_hits also wants the expanded
        // records: those are looked up here (hit_terms), the totals still come from the stored terms.
        if (h <= 64) {
            // Common case: no sort.  Lane l takes key l and its terms, finds the rank of its key among the h keys by
            // counting, and drops the terms at that rank; lane r then owns the r-th hit in key order.
            uint64_t key = ~0ull;
            double2 mine = make_double2(0.0, 0.0);
            issl_hit rec{};
            if (lane < h) {
                key = key_of(lane);
                mine = terms_of(lane);
                if (out_hits) rec = hit_terms(v, gsig, g, key, calc_mit, calc_cfd, true).rec;
            }
            uint32_t rank = 0;
            for (uint32_t j = 0; j < h; ++j) {
                const uint32_t klo = __builtin_amdgcn_readlane(static_cast<uint32_t>(key), static_cast<int>(j));
                const uint32_t khi = __builtin_amdgcn_readlane(static_cast<uint32_t>(key >> 32), static_cast<int>(j));
                const uint64_t other = (static_cast<uint64_t>(khi) << 32) | klo;
                rank += (other < key) ? 1u : 0u;
            }
            if (lane < h) {
                ord[rank] = mine;
                if (out_hits) out_hits[h0 + rank] = rec;
            } else {
                ord[lane] = make_double2(0.0, 0.0); // (ranks are below h: nobody else writes here)
            }
            __syncthreads();
            const double2 t = ord[lane];
            accumulate(t.x, t.y, h);
        } else {
            // (slice, position) of every key with the key's index behind it, sorted; the terms follow by index
            uint64_t *data = keys;
            auto word_of = [&](uint32_t i) { return ((key_of(i) & ((1ull << kKeyGuideShift) - 1ull)) << 9) | i; }; // h <= 512
            // Up to 256 hits: sorted in registers (wave_sort_regs), 2 / 4 words per lane, ~0 behind the last hit; the sorted words
            // go to LDS once, for the chunks below to pick up by position
            auto sort_in_registers = [&](auto words_per_lane) {
                constexpr uint32_t R = decltype(words_per_lane)::value;
                uint64_t w[R];
#pragma unroll
                for (uint32_t r = 0; r < R; ++r) w[r] = lane * R + r < h ? word_of(lane * R + r) : ~0ull;
                wave_sort_regs<R>(w, lane);
#pragma unroll
                for (uint32_t r = 0; r < R; ++r) keys[lane * R + r] = w[r];
            };
            if (h <= 128u) sort_in_registers(std::integral_constant<uint32_t, 2u>{});
            else if (h <= 256u) sort_in_registers(std::integral_constant<uint32_t, 4u>{});
            else { // (eight words per lane spill at the 64 registers that keep eight waves on a SIMD: beyond 256 hits, in LDS)
                for (uint32_t i = lane; i < h; i += 64) keys[i] = word_of(i);
                __syncthreads();
                wave_sort(data, h);
            }
            __syncthreads();
            for (uint32_t base = 0; base < h && !stop; base += 64) {
                const uint32_t idx = base + lane;
                double2 mine = make_double2(0.0, 0.0);
                if (idx < h) {
                    const uint64_t sv = data[idx];
                    mine = terms_of(static_cast<uint32_t>(sv & 511ull));
                    if (out_hits)
                        out_hits[h0 + idx] = hit_terms(v, gsig, g, (static_cast<uint64_t>(g) << kKeyGuideShift) | (sv >> 9), calc_mit, calc_cfd, true).rec;
                }
                __syncthreads(); // (the walk of the chunk before has read `ord`)
                ord[lane] = mine;
                __syncthreads();
                accumulate(mine.x, mine.y, (h - base < 64u) ? h - base : 64u);
            }
        }
        if (lane == 0) {
            out_mit[g] = 10000.0 / (100.0 + tot_mit); // :505
            out_cfd[g] = 10000.0 / (100.0 + tot_cfd); // :506
            if (out_kept) out_kept[g] = kept;
        }
        __syncthreads();
    }
}

// Guides with kReplayLds < hits <= kMidHits (on skewed data four guides in ten): one 256-thread workgroup each, the terms
// k_verify left fetched by the hit's index.  One slice at a time, as the reference walks them (:330): the slice's keys are
// gathered into LDS, ranked by counting (no barrier inside: a bitonic network over 2048 keys costs 66 barrier-separated
// stages, 170 us per guide), their terms fetched -- all of the slice's at once -- and dropped at their ranks; wave 0 then
// walks the terms in LDS.  Such a guide usually leaves through the early exit (:467-496) inside its first slice (median:
// 295 hits walked of 1024 found), and the slices behind the exit are never touched.  A guide with a slice of more than
// kMidSlice hits is handed on to k_replay_big (second list).
// Round 4, later: (a) a slice of more than kMidDirect hits is ranked INSIDE 256 groups of the range its ids span (one
// counting pass in LDS puts the ids in group order first): len * len / 256 comparisons on evenly spread ids instead of
// len * len -- the kernel was bound by the vector instructions of the all-against-all count (0.67 G of them per 100 k guides
// of the skewed index); (b) the workgroups take the entries of the guide list one at a time from a device-wide ticket
// (asked for one guide ahead), not every gridDim-th entry: the 2048 workgroups are not all resident (7 per CU), and the
// stragglers of a static split ran alone on an empty chip for a quarter of the launch.
constexpr uint32_t kMidSlice = 1024;
constexpr uint32_t kBigSmall = 16384; // up to this many hits of a guide: the 256-thread build of k_replay_big
constexpr uint32_t kMidDirect = 256;  // up to this many hits in a slice: ranked against all of them, one per thread
// The next entry of the many-hit guide list for this workgroup (`which`: Counters::replay_next), handed to all its threads
// through LDS; the ticket after it is asked for at once, so that its round trip runs beside the guide's work.  (Two LDS
// words, used in turn: a wave that is late reading this guide's entry must not find the next one's there.)
struct ReplayTicket {
    uint32_t next = 0, turn = 0;
};
__device__ __forceinline__ uint32_t replay_take(ReplayTicket &t, uint32_t *cur /*LDS[2]*/, Counters *counters, uint32_t which,
                                                bool first, uint32_t n_entries)
{
    // no more entries than workgroups (a small batch, a few many-hit guides): one each, no ticket, no barrier -- the kernel then
    // lasts as long as its slowest guide, and the round trip of the atomic is part of that
    if (n_entries <= gridDim.x) return first ? blockIdx.x : n_entries;
    if (threadIdx.x == 0) {
        if (first) t.next = atomicAdd(&counters->replay_next[which], 1u);
        cur[t.turn] = t.next;
    }
    __syncthreads();
    const uint32_t b = cur[t.turn];
    t.turn ^= 1u;
    if (threadIdx.x == 0) t.next = atomicAdd(&counters->replay_next[which], 1u);
    return b;
}

__global__ __launch_bounds__(256, 6) void k_replay_mid(ImageView v, Workspace ws, const uint64_t *__restrict__ guides,
                                                    ScoreParams p, double *__restrict__ out_mit,
                                                    double *__restrict__ out_cfd, uint32_t *__restrict__ out_kept,
                                                    issl_hit *__restrict__ out_hits)
{
    short_kernel_priority();
    __shared__ __attribute__((aligned(16))) uint32_t head[kMidSlice]; // the slice's keys: site ids or positions (distinct) ...
    __shared__ uint16_t head_idx[kMidSlice];                           // ... and the index of the hit each belongs to
    __shared__ __attribute__((aligned(16))) double2 tmc[kMidSlice];    // its terms {mit, cfd} in key order (before that: the
                                                                       // slice's ids and hit indexes in group order)
    __shared__ uint32_t slice_cnt[kMaxSlices];
    __shared__ uint32_t group_at[257], group_cur[256], id_min, id_max;
    __shared__ uint32_t head_fill, stopped_s, carry_kept, cur_entry[2];
    __shared__ double carry_mit, carry_cfd;
    const bool calc_mit = p.method == ISSL_METHOD_MIT || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const bool calc_cfd = p.method == ISSL_METHOD_CFD || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_big = ws.counters->n_big;
    const double2 *__restrict__ terms2 = reinterpret_cast<const double2 *>(ws.terms);
    if (blockIdx.x >= n_big) return; // (more workgroups than entries -- on an even index there are none: no ticket is taken)
    ReplayTicket ticket;
    for (bool first = true;; first = false) {
        const uint32_t b = replay_take(ticket, cur_entry, ws.counters, 0u, first, n_big);
        if (b >= n_big) break;
        const uint32_t g = ws.gcur_big[b];
        const uint32_t h = ws.gcount[g];
        if (h > kMidHits) { // (uniform) k_replay_big's: onto the list of its 256-thread build, or -- from the far end of the same array -- of the other
            if (threadIdx.x == 0) {
                if (h <= kBigSmall) ws.gcur_big2[atomicAdd(&ws.counters->n_big2, 1u)] = g;
                else ws.gcur_big2[static_cast<uint32_t>(ws.cap_guides) - atomicAdd(&ws.counters->n_big3, 1u)] = g;
            }
            continue;
        }
        const uint32_t h0 = ws.goff[g];
        const uint64_t gsig = guides[g];
        // hit i of the guide: in its hit slots below slot_hits, in its segment of the grouped arrays from there on
        const uint32_t in_slots = ws.slot_hits;
        const SlotRec *__restrict__ srec = ws.slots + static_cast<uint64_t>(g) * in_slots;
        const uint64_t *__restrict__ gkeys = ws.sorted + h0;
        // diagnostics (ISSL_SCAN_STAMPS): phase clocks of the first 4096 listed guides, like k_replay_big's
        unsigned long long *st = (ws.stamps && b < 4096u) ? ws.stamps + kStampsMid + 16u * b : nullptr;
        if (st && threadIdx.x == 0) { st[0] = __builtin_amdgcn_s_memrealtime(); st[1] = h; st[15] = blockIdx.x; st[14] = 1; }
        if (threadIdx.x < kMaxSlices) slice_cnt[threadIdx.x] = 0;
        if (threadIdx.x == 0) { stopped_s = 0; carry_mit = 0.0; carry_cfd = 0.0; carry_kept = 0; }
        __syncthreads();
        // the guide's keys, eight per thread, all asked for at once and kept in registers: every later phase works from
        // them (a phase that goes back to memory costs a round trip of microseconds, and a guide is a chain of phases)
        uint64_t mykey[kMidHits / 256];
#pragma unroll
        for (uint32_t k = 0; k < kMidHits / 256; ++k) {
            const uint32_t i = k * 256u + threadIdx.x;
            mykey[k] = i < h ? (i < in_slots ? srec[i].key : gkeys[i]) : ~0ull;
        }
#pragma unroll
        for (uint32_t k = 0; k < kMidHits / 256; ++k) { // hits per slice (one LDS atomic per wave and slice present)
            if (k * 256u >= h) break;
            const uint32_t sl = mykey[k] != ~0ull ? static_cast<uint32_t>(mykey[k] >> kKeySliceShift) & kKeySliceMask : kKeySliceMask;
            for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) {
                const uint64_t mm = __ballot(sl == s2);
                if (mm != 0ull && lane == 0) atomicAdd(&slice_cnt[s2], static_cast<uint32_t>(__builtin_popcountll(mm)));
            }
        }
        __syncthreads();
        uint32_t longest = 0;
        for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) longest = slice_cnt[s2] > longest ? slice_cnt[s2] : longest;
        if (longest > kMidSlice) { // (uniform) a slice that does not fit: the slice-by-slice kernel with the larger buffers
            if (threadIdx.x == 0) ws.gcur_big2[atomicAdd(&ws.counters->n_big2, 1u)] = g;
            __syncthreads(); // (the next guide's reset of slice_cnt must not overtake a wave that is still reading it)
            continue;
        }
        if (st && threadIdx.x == 0) st[2] = __builtin_amdgcn_s_memrealtime();
        uint32_t walked = 0; // hits of the slices done so far (= where this slice's hits start in scoring order)
        for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) {
            const uint32_t len = slice_cnt[s2];
            if (len == 0) continue;
            const bool grouped_rank = len > kMidDirect; // (uniform)
            if (threadIdx.x == 0) { head_fill = 0; id_min = 0xFFFFFFFFu; id_max = 0u; }
            group_cur[threadIdx.x] = 0;
            __syncthreads();
            uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
            for (uint32_t k = 0; k < kMidHits / 256; ++k) { // gather the slice's keys (one cursor bump per wave)
                if (k * 256u >= h) break;
                const uint64_t key = mykey[k];
                const bool mine = key != ~0ull && (static_cast<uint32_t>(key >> kKeySliceShift) & kKeySliceMask) == s2;
                const uint64_t mm = __ballot(mine);
                if (mm == 0ull) continue;
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&head_fill, static_cast<uint32_t>(__builtin_popcountll(mm)));
                at = __builtin_amdgcn_readfirstlane(at);
                if (mine) {
                    const uint32_t to = at + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mm >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mm), 0u));
                    const uint32_t id = static_cast<uint32_t>(key);
                    head[to] = id;
                    head_idx[to] = static_cast<uint16_t>(k * 256u + threadIdx.x);
                    mn = id < mn ? id : mn;
                    mx = id > mx ? id : mx;
                }
            }
            if (grouped_rank && mn <= mx) { atomicMin(&id_min, mn); atomicMax(&id_max, mx); } // the range the slice's ids span
            __syncthreads();
            // Rank by counting against the WHOLE slice (the keys are distinct: ids / positions are), K keys per thread, the
            // slice's ids read four at a time by every thread at once; then the terms to their ranks.
            auto rank_against_all = [&](auto k_tag) {
                constexpr uint32_t K = decltype(k_tag)::value;
                if (threadIdx.x < 4u && len + threadIdx.x < ((len + 3u) & ~3u)) head[len + threadIdx.x] = 0xFFFFFFFFu; // (read four at a time)
                __syncthreads();
                uint32_t mine[K], rk[K];
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) { mine[k] = threadIdx.x + k * 256u < len ? head[threadIdx.x + k * 256u] : 0xFFFFFFFFu; rk[k] = 0; }
                const uint4 *quads = reinterpret_cast<const uint4 *>(head);
#pragma unroll 4
                for (uint32_t j = 0; j < (len + 3u) / 4u; ++j) {
                    const uint4 q = quads[j];
#pragma unroll
                    for (uint32_t k = 0; k < K; ++k)
                        rk[k] += (q.x < mine[k] ? 1u : 0u) + (q.y < mine[k] ? 1u : 0u) + (q.z < mine[k] ? 1u : 0u) + (q.w < mine[k] ? 1u : 0u);
                }
#pragma unroll
                for (uint32_t k = 0; k < K; ++k) {
                    if (threadIdx.x + k * 256u >= len) continue;
                    const uint32_t idx = head_idx[threadIdx.x + k * 256u];
                    const double2 t2 = idx < in_slots ? *reinterpret_cast<const double2 *>(&srec[idx].mit) : terms2[h0 + idx];
                    tmc[rk[k]] = t2;
                    if (out_hits)
                        out_hits[h0 + walked + rk[k]] = hit_terms(v, gsig, g, (static_cast<uint64_t>(g) << kKeyGuideShift) |
                                                                      (static_cast<uint64_t>(s2) << kKeySliceShift) | mine[k],
                                                                  calc_mit, calc_cfd, true).rec;
                }
            };
            if (!grouped_rank) {
                rank_against_all(std::integral_constant<uint32_t, 1u>{});
            } else {
                // Ranked inside 256 groups of the range the ids span (the hits of a guide in one slice share the slice's bases:
                // on a text-sorted index their ids lie in a narrow range far from zero): group sizes, their prefix, the ids and
                // hit indexes in group order (in the memory the terms will take), then every id against its own group only.
                // Ids that pile up in one group -- a repeat family: neighbours in the text-sorted site table -- leave nothing to
                // gain there: a slice whose largest group holds more than a quarter of it is ranked against all of it.
                const uint32_t low = id_min, top = id_max - low;
                const uint32_t shift = top < 256u ? 0u : 24u - static_cast<uint32_t>(__builtin_clz(top)); // (id - low) >> shift < 256
#pragma unroll
                for (uint32_t k = 0; k < kMidSlice / 256; ++k)
                    if (threadIdx.x + k * 256u < len) atomicAdd(&group_cur[(head[threadIdx.x + k * 256u] - low) >> shift], 1u);
                __syncthreads();
                if (threadIdx.x < 64) { // exclusive scan of the 256 group sizes by one wave, 4 per lane; the cursors start there
                    uint32_t v4[4], sum = 0, big = 0;
                    for (uint32_t k = 0; k < 4; ++k) { v4[k] = group_cur[threadIdx.x * 4 + k]; sum += v4[k]; big = v4[k] > big ? v4[k] : big; }
                    uint32_t x = sum;
                    for (uint32_t d = 1; d < 64; d <<= 1) {
                        const uint32_t y = __shfl_up(x, d, 64);
                        if (threadIdx.x >= d) x += y;
                    }
                    for (uint32_t d = 32; d > 0; d >>= 1) { const uint32_t y = __shfl_xor(big, d, 64); big = y > big ? y : big; }
                    uint32_t run = x - sum;
                    for (uint32_t k = 0; k < 4; ++k) { group_at[threadIdx.x * 4 + k] = run; group_cur[threadIdx.x * 4 + k] = run; run += v4[k]; }
                    if (threadIdx.x == 63) group_at[256] = run;
                    if (threadIdx.x == 0) id_max = big; // (the range is in registers: the word now says how large the largest group is)
                }
                __syncthreads();
                if (id_max * 4u > len) { // (uniform)
                    if (len <= 512u) rank_against_all(std::integral_constant<uint32_t, 2u>{});
                    else rank_against_all(std::integral_constant<uint32_t, 4u>{});
                } else {
                uint32_t *ids2 = reinterpret_cast<uint32_t *>(tmc);                 // [kMidSlice]
                uint16_t *idx2 = reinterpret_cast<uint16_t *>(ids2 + kMidSlice);    // [kMidSlice]
#pragma unroll
                for (uint32_t k = 0; k < kMidSlice / 256; ++k) {
                    const uint32_t i = threadIdx.x + k * 256u;
                    if (i >= len) continue;
                    const uint32_t id = head[i];
                    const uint32_t to = atomicAdd(&group_cur[(id - low) >> shift], 1u);
                    ids2[to] = id;
                    idx2[to] = head_idx[i];
                }
                if (threadIdx.x < 4u && len + threadIdx.x < ((len + 3u) & ~3u)) ids2[len + threadIdx.x] = 0xFFFFFFFFu; // (read four at a time)
                __syncthreads();
                // every id against its own group, four ids per LDS read: the quads that cover the group also hold ids of the
                // groups around it -- smaller ones below (each counts: the rank starts at the quad, not at the group), larger
                // ones and the padding above (none counts); id and hit index go to the id's rank (`head`, `head_idx`: their
                // first contents are in group order now), so that nothing is carried across the barrier but the arrays
                const uint4 *quads2 = reinterpret_cast<const uint4 *>(ids2);
#pragma unroll
                for (uint32_t k = 0; k < kMidSlice / 256; ++k) {
                    const uint32_t i = threadIdx.x + k * 256u;
                    if (i < len) {
                        const uint32_t id = ids2[i];
                        const uint32_t g0 = group_at[(id - low) >> shift], g1 = group_at[((id - low) >> shift) + 1u];
                        uint32_t r = g0 & ~3u;
                        for (uint32_t j = g0 >> 2; j < (g1 + 3u) >> 2; ++j) {
                            const uint4 q = quads2[j];
                            r += (q.x < id ? 1u : 0u) + (q.y < id ? 1u : 0u) + (q.z < id ? 1u : 0u) + (q.w < id ? 1u : 0u);
                        }
                        head[r] = id;
                        head_idx[r] = idx2[i];
                    }
                }
                __syncthreads(); // (everybody has read the ids in group order: the terms may land on them)
#pragma unroll
                for (uint32_t k = 0; k < kMidSlice / 256; ++k) {
                    const uint32_t i = threadIdx.x + k * 256u;
                    if (i < len) {
                        const uint32_t idx = head_idx[i];
                        tmc[i] = idx < in_slots ? *reinterpret_cast<const double2 *>(&srec[idx].mit) : terms2[h0 + idx];
                        if (out_hits)
                            out_hits[h0 + walked + i] = hit_terms(v, gsig, g, (static_cast<uint64_t>(g) << kKeyGuideShift) |
                                                                      (static_cast<uint64_t>(s2) << kKeySliceShift) | head[i],
                                                                  calc_mit, calc_cfd, true).rec;
                    }
                }
                }
            }
            if (threadIdx.x < 8u && len + threadIdx.x < ((len + 7u) & ~7u)) tmc[len + threadIdx.x] = make_double2(0.0, 0.0); // (walked eight at a time)
            __syncthreads();
            if (st && threadIdx.x == 0 && walked == 0) { st[3] = __builtin_amdgcn_s_memrealtime(); st[4] = len; }
            if (threadIdx.x < 64) { // wave 0 walks the slice
                double tot_mit = carry_mit, tot_cfd = carry_cfd;
                uint32_t kept = carry_kept;
                bool stop = false;
                for (uint32_t base = 0; base < len && !stop; base += 64) {
                    const uint32_t idx = base + lane;
                    const double2 mine2 = idx < len ? tmc[idx] : make_double2(0.0, 0.0);
                    stop = accumulate_chunk<false>(mine2.x, mine2.y, (len - base < 64u) ? len - base : 64u, p, lane, tot_mit, tot_cfd, kept,
                                            tmc + base);
                }
                if (lane == 0) { carry_mit = tot_mit; carry_cfd = tot_cfd; carry_kept = kept; stopped_s = stop ? 1u : 0u; }
            }
            __syncthreads();
            walked += len;
            if (stopped_s != 0u) break; // (uniform) the slices behind the exit are never touched
        }
        if (threadIdx.x == 0) {
            out_mit[g] = 10000.0 / (100.0 + carry_mit); // :505
            out_cfd[g] = 10000.0 / (100.0 + carry_cfd); // :506
            if (out_kept) out_kept[g] = carry_kept;
            if (st) { st[7] = __builtin_amdgcn_s_memrealtime(); st[8] = carry_kept; st[9] = walked; }
        }
        __syncthreads();
    }
}

// Sort by counting for the slices of a big guide: positions (low 32 key bits; guide and slice are common to the
// slice) sit in LDS, every thread finds the rank of its K positions by comparing them with all `len` of them
// (broadcast reads, no barrier inside) and writes the full keys to their final places.  A bitonic network over the same
// keys costs ~80-90 workgroup barriers; positions are distinct, so the ranks are a permutation.
template <uint32_t K, uint32_t THREADS>
__device__ __forceinline__ void rank_sort_slice(const uint32_t *pos_lds, uint32_t len, uint64_t high_bits,
                                                uint64_t *__restrict__ dst)
{
    uint32_t mine[K], rk[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t idx = threadIdx.x + k * THREADS;
        mine[k] = idx < len ? pos_lds[idx] : 0xFFFFFFFFu;
        rk[k] = 0;
    }
    // four positions per LDS read (the array is padded with 0xFFFFFFFF, which is below nothing), several reads in
    // flight: the loop is bound by LDS latency otherwise
    const uint4 *quads = reinterpret_cast<const uint4 *>(pos_lds);
    const uint32_t n_quads = (len + 3u) >> 2;
#pragma unroll 4
    for (uint32_t j = 0; j < n_quads; ++j) {
        const uint4 q = quads[j];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k)
            rk[k] += (q.x < mine[k] ? 1u : 0u) + (q.y < mine[k] ? 1u : 0u) + (q.z < mine[k] ? 1u : 0u) +
                     (q.w < mine[k] ? 1u : 0u);
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k)
        if (threadIdx.x + k * THREADS < len) dst[rk[k]] = high_bits | mine[k];
}

// Longer slices: the same ranking, but only against the positions that share the top 8 bits (of the slice's largest
// position): one counting pass groups the positions by those bits in `grouped`, then every position is ranked inside
// its group -- len * len / 256 comparisons on evenly spread positions instead of len * len.
__device__ __forceinline__ void rank_sort_slice_grouped(const uint32_t *pos_lds, uint32_t *grouped, uint32_t *group_at /*[257]*/,
                                                        uint32_t *group_cur /*[256]*/, uint32_t *max_pos, uint32_t *min_pos,
                                                        uint32_t len, uint64_t high_bits, uint64_t *__restrict__ dst)
{
    if (threadIdx.x < 256) group_cur[threadIdx.x] = 0;
    if (threadIdx.x == 0) { *max_pos = 0; *min_pos = 0xFFFFFFFFu; }
    __syncthreads();
    uint32_t m = 0, mn = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) { const uint32_t q = pos_lds[i]; m = q > m ? q : m; mn = q < mn ? q : mn; }
    atomicMax(max_pos, m);
    atomicMin(min_pos, mn);
    __syncthreads();
    // (the hits of a guide in one slice share the slice's bases: on a text-sorted index their ids lie in a narrow range far
    // from zero, so the groups divide the range they span, not the values)
    const uint32_t low = *min_pos, top = *max_pos - low;
    const uint32_t shift = top < 256u ? 0u : 24u - static_cast<uint32_t>(__builtin_clz(top)); // group = (pos - low) >> shift < 256
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) atomicAdd(&group_cur[(pos_lds[i] - low) >> shift], 1u);
    __syncthreads();
    if (threadIdx.x < 64) { // exclusive scan of the 256 group sizes by one wave, 4 per lane
        uint32_t v4[4], sum = 0;
        for (uint32_t k = 0; k < 4; ++k) { v4[k] = group_cur[threadIdx.x * 4 + k]; sum += v4[k]; }
        uint32_t x = sum;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (threadIdx.x >= d) x += y;
        }
        uint32_t run = x - sum;
        for (uint32_t k = 0; k < 4; ++k) { group_at[threadIdx.x * 4 + k] = run; run += v4[k]; }
        if (threadIdx.x == 63) group_at[256] = run;
    }
    __syncthreads();
    if (threadIdx.x < 256) group_cur[threadIdx.x] = group_at[threadIdx.x];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
        const uint32_t pos = pos_lds[i];
        grouped[atomicAdd(&group_cur[(pos - low) >> shift], 1u)] = pos;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
        const uint32_t pos = grouped[i];
        const uint32_t g0 = group_at[(pos - low) >> shift], g1 = group_at[((pos - low) >> shift) + 1u];
        uint32_t rk = g0;
        for (uint32_t j = g0; j < g1; ++j) rk += grouped[j] < pos ? 1u : 0u;
        dst[rk] = high_bits | pos;
    }
}

// Guides with many hits (dense neighbourhoods, repeats): one 1024-thread workgroup each, one slice at a time: sort
// the slice's keys (by counting in LDS up to 8192 per slice, else a bitonic network in HBM), compute the terms of its
// hits in parallel, let wave 0 add them up in key order with the reference's running totals and early exit.
template <uint32_t THREADS, uint32_t LDS_HITS>
__global__ __launch_bounds__(THREADS, THREADS < 1024u ? 6 : 4) void k_replay_big(ImageView v, Workspace ws, const uint64_t *__restrict__ guides,
                                                     ScoreParams p, double *__restrict__ out_mit,
                                                     double *__restrict__ out_cfd, uint32_t *__restrict__ out_kept,
                                                     issl_hit *__restrict__ out_hits)
{
    short_kernel_priority();
    __shared__ __attribute__((aligned(16))) uint32_t pos_lds[LDS_HITS];
    __shared__ uint32_t grouped[LDS_HITS];
    __shared__ uint32_t group_at[257], group_cur[256], max_pos, min_pos;
    __shared__ uint32_t outer_at[257]; // a slice beyond the LDS: where its 256 id groups start once it is in group order
    __shared__ uint32_t slice_cnt[kMaxSlices], slice_off[kMaxSlices + 1], slice_cur[kMaxSlices];
    __shared__ uint32_t walk_stopped, head_groups, head_count, head_fill;
    __shared__ __attribute__((aligned(16))) double2 walk_terms[64]; // wave 0: the terms of the 64 hits it is adding up
    const bool calc_mit = p.method == ISSL_METHOD_MIT || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const bool calc_cfd = p.method == ISSL_METHOD_CFD || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR ||
                          p.method == ISSL_METHOD_AVG;
    const uint32_t lane = threadIdx.x & 63u;
    // The guides of this build: a list k_replay_mid has made while it went through the shared one (more than kMidHits hits, or
    // handed on; the 1024-thread build's from the far end of the array).  (Each build used to walk the whole shared list and skip
    // what was not its own: 40 k entries of three dependent loads each, for the few dozen guides of the 1024-thread build.)
    const uint32_t n_mine = THREADS < 1024u ? ws.counters->n_big2 : ws.counters->n_big3;
    __shared__ uint32_t cur_entry[2];
    if (blockIdx.x >= n_mine) return; // (more workgroups than entries: no ticket is taken)
    ReplayTicket ticket;
    for (bool first = true;; first = false) { // (entries by ticket, as in k_replay_mid)
        const uint32_t b = replay_take(ticket, cur_entry, ws.counters, THREADS < 1024u ? 1u : 2u, first, n_mine);
        if (b >= n_mine) break;
        const uint32_t g = THREADS < 1024u ? ws.gcur_big2[b] : ws.gcur_big2[static_cast<uint32_t>(ws.cap_guides) - b];
        const uint32_t h = ws.gcount[g];
        const uint32_t h0 = ws.goff[g];
        // k_replay_mid's, or the other build's: up to kBigSmall hits a 256-thread workgroup with 2048 hits per slice in
        // LDS (eight per CU: what such a guide costs is a chain of barriers and memory round trips, and what counts is
        // how many are in flight), beyond that 1024 threads with 7680 (two per CU).  (uniform over the workgroup)
        const uint64_t gsig = guides[g];
        uint64_t *seg = ws.sorted + h0;
        uint64_t *tmp = ws.raw + h0; // the raw records are dead once they are grouped; the buffer holds >= all hits
        // diagnostics (ISSL_SCAN_STAMPS, tools/replay_stamps.py): phase clocks of the first 4096 big guides
        unsigned long long *st = (ws.stamps && b < 4096u) ? ws.stamps + (THREADS < 1024u ? kStampsBig256 : kStampsBig1024) + 16u * b : nullptr; // (behind k_replay_mid's)
        if (st && threadIdx.x == 0) { st[0] = __builtin_amdgcn_s_memrealtime(); st[1] = h; st[15] = blockIdx.x; }

        // The scoring order is (slice, position in bucket) and the walk usually ends inside the first slice (the
        // totals pass the threshold, :467-496): split the keys by slice (bits 32..34) and sort and walk one slice at
        // a time -- a fifth of the sorting work per step, in LDS up to 8192 hits PER SLICE, and none at all for the
        // slices behind the exit.
        if (threadIdx.x < kMaxSlices) { slice_cnt[threadIdx.x] = 0; slice_cur[threadIdx.x] = 0; }
        // hit slots: the guide's first slot_hits keys join the rest in its segment (h > slot_hits here: all of them are there)
        for (uint32_t i = threadIdx.x; i < (ws.slot_hits < h ? ws.slot_hits : h); i += blockDim.x) seg[i] = ws.slots[static_cast<uint64_t>(g) * ws.slot_hits + i].key;
        __syncthreads();
        for (uint32_t base = 0; base < h; base += blockDim.x) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t sl = i < h ? static_cast<uint32_t>(seg[i] >> kKeySliceShift) & kKeySliceMask : kKeySliceMask;
            for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) {
                const uint64_t m = __ballot(sl == s2);
                if (m != 0ull && lane == 0) atomicAdd(&slice_cnt[s2], static_cast<uint32_t>(__builtin_popcountll(m)));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t run = 0;
            for (uint32_t s2 = 0; s2 < kMaxSlices; ++s2) { slice_off[s2] = run; run += slice_cnt[s2]; }
            slice_off[kMaxSlices] = run;
        }
        __syncthreads();
        for (uint32_t base = 0; base < h; base += blockDim.x) {
            const uint32_t i = base + threadIdx.x;
            const uint64_t key = i < h ? seg[i] : 0ull;
            const uint32_t sl = i < h ? static_cast<uint32_t>(key >> kKeySliceShift) & kKeySliceMask : kKeySliceMask;
            for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) {
                const uint64_t m = __ballot(sl == s2);
                if (m == 0ull) continue;
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&slice_cur[s2], static_cast<uint32_t>(__builtin_popcountll(m)));
                at = __builtin_amdgcn_readfirstlane(at);
                if (sl == s2)
                    tmp[slice_off[s2] + at + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u))] = key;
            }
        }
        __syncthreads();

        if (st && threadIdx.x == 0) st[2] = __builtin_amdgcn_s_memrealtime();
        double tot_mit = 0.0, tot_cfd = 0.0;
        uint32_t kept = 0;
        bool stop = false;
        auto accumulate = [&](double mit_term, double cfd_term, uint32_t cnt) { // (wave 0 only)
            __builtin_amdgcn_wave_barrier();
            walk_terms[lane] = make_double2(mit_term, cfd_term);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            stop = accumulate_chunk<false>(mit_term, cfd_term, cnt, p, lane, tot_mit, tot_cfd, kept, walk_terms);
        };
        for (uint32_t s2 = 0; s2 < v.n_slices; ++s2) {
            const uint32_t off = slice_off[s2], len = slice_cnt[s2];
            if (len == 0) continue; // uniform over the workgroup
            if (st && threadIdx.x == 0 && s2 == 0) { st[3] = __builtin_amdgcn_s_memrealtime(); st[4] = len; }
            uint64_t *dst = seg + off;
            const uint64_t high_bits = (static_cast<uint64_t>(g) << kKeyGuideShift) | (static_cast<uint64_t>(s2) << kKeySliceShift);
            // Terms of hits [from, to) of the slice (dst[] holds them in key order) by the whole workgroup, a block of
            // blockDim.x at a time, each block added up in key order by wave 0 before the next one is worked out: a
            // guide like this usually leaves through the early exit within its first hits (:467-496), and the terms
            // cost two or three random reads each.  Leaves walk_stopped set when the exit was taken.
            auto walk = [&](uint32_t from, uint32_t to) {
                for (uint32_t blk = from; blk < to; blk += blockDim.x) {
                    const uint32_t i = blk + threadIdx.x;
                    if (i < to) {
                        const HitTerms t = hit_terms(v, gsig, g, dst[i], calc_mit, calc_cfd, out_hits != nullptr);
                        ws.terms[2ull * (h0 + off + i)] = t.mit;
                        ws.terms[2ull * (h0 + off + i) + 1] = t.cfd;
                        if (out_hits) out_hits[h0 + off + i] = t.rec;
                    }
                    __syncthreads();
                    if (threadIdx.x < 64) {
                        const uint32_t end = (to - blk < blockDim.x) ? to : blk + blockDim.x;
                        for (uint32_t base = blk; base < end && !stop; base += 64) {
                            const uint32_t idx = base + lane;
                            const double mit_term = idx < end ? ws.terms[2ull * (h0 + off + idx)] : 0.0;
                            const double cfd_term = idx < end ? ws.terms[2ull * (h0 + off + idx) + 1] : 0.0;
                            accumulate(mit_term, cfd_term, (end - base < 64u) ? end - base : 64u);
                        }
                        if (lane == 0) walk_stopped = stop ? 1u : 0u;
                    }
                    __syncthreads();
                    if (walk_stopped != 0u) break; // uniform
                }
            };
            auto sort_in_lds = [&](uint32_t n, uint64_t *out) { // pos_lds[0 .. n) -> out[0 .. n) in key order
                if (n <= THREADS) rank_sort_slice<1, THREADS>(pos_lds, n, high_bits, out);
                else rank_sort_slice_grouped(pos_lds, grouped, group_at, group_cur, &max_pos, &min_pos, n, high_bits, out);
                __syncthreads();
            };
            uint32_t walked = 0;
            uint32_t g_low = 0, g_shift = 0, g_done = 0; // the id groups of the head pass: (id - g_low) >> g_shift; the first g_done are walked
            if (threadIdx.x == 0) walk_stopped = 0;
            __syncthreads();
            if (len > THREADS) {
                // A guide like this all but always leaves through the early exit within the hits with the smallest ids of
                // its first slice (median: ~250 hits walked of thousands found), so those are tried first: the slice's
                // positions are counted by their top eight bits, the leading groups that hold at least 384 of them are
                // gathered, ranked by counting and walked; only a guide that survives them pays for the order of the whole
                // slice (a ranking inside unevenly filled groups in LDS; beyond the LDS a bitonic network in HBM of ~140
                // stages of memory round trips, which used to set the kernel's duration).
                if (threadIdx.x < 256) group_cur[threadIdx.x] = 0;
                if (threadIdx.x == 0) { max_pos = 0; min_pos = 0xFFFFFFFFu; head_fill = 0; }
                __syncthreads();
                uint32_t m = 0, mn = 0xFFFFFFFFu;
                for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) { const uint32_t q = static_cast<uint32_t>(tmp[off + i]); m = q > m ? q : m; mn = q < mn ? q : mn; }
                atomicMax(&max_pos, m);
                atomicMin(&min_pos, mn);
                __syncthreads();
                const uint32_t low = min_pos, top = max_pos - low; // (groups of the RANGE the slice's ids span: see rank_sort_slice_grouped)
                const uint32_t shift = top < 256u ? 0u : 24u - static_cast<uint32_t>(__builtin_clz(top));
                for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) atomicAdd(&group_cur[(static_cast<uint32_t>(tmp[off + i]) - low) >> shift], 1u);
                __syncthreads();
                if (threadIdx.x == 0) {
                    uint32_t run = 0, nb = 0;
                    while (nb < 256u && run < 384u) run += group_cur[nb++];
                    head_groups = nb;
                    head_count = run;
                }
                __syncthreads();
                const uint32_t nb = head_groups, cnt = head_count;
                g_low = low; g_shift = shift;
                constexpr uint32_t kHeadMax = 4u * THREADS < LDS_HITS ? 4u * THREADS : LDS_HITS; // what rank_sort_slice<4> takes
                if (cnt <= kHeadMax && cnt < len) {
                    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
                        const uint32_t q = static_cast<uint32_t>(tmp[off + i]);
                        if (((q - low) >> shift) < nb) pos_lds[atomicAdd(&head_fill, 1u)] = q;
                    }
                    __syncthreads();
                    for (uint32_t i = cnt + threadIdx.x; i < ((cnt + 3u) & ~3u); i += blockDim.x) pos_lds[i] = 0xFFFFFFFFu;
                    __syncthreads();
                    if (cnt <= THREADS) rank_sort_slice<1, THREADS>(pos_lds, cnt, high_bits, dst);
                    else rank_sort_slice<4, THREADS>(pos_lds, cnt, high_bits, dst);
                    __syncthreads();
                    walk(0u, cnt);
                    walked = cnt;
                    g_done = nb;
                }
            }
            if (walk_stopped == 0u && walked < len) { // (uniform) the whole slice in key order
                if (len <= LDS_HITS) {
                    for (uint32_t i = threadIdx.x; i < ((len + 3u) & ~3u); i += blockDim.x)
                        pos_lds[i] = i < len ? static_cast<uint32_t>(tmp[off + i]) : 0xFFFFFFFFu;
                    __syncthreads();
                    sort_in_lds(len, dst);
                } else {
                    // A slice beyond the LDS.  Its keys go into group order first -- the 256 groups of the range its ids span
                    // that the head pass counted (group_cur), one pass with the cursors in LDS --, then run after run of
                    // consecutive groups that fit the LDS is sorted there and walked: the exit (:467-496) usually comes before
                    // the second run, and no run costs more than a slice that fits.  (A bitonic network over the whole slice in
                    // HBM, ~140 stages of memory round trips, set the duration of this kernel before: 0.5 ms per batch on the
                    // skewed index for a few dozen guides.)  Only a single group beyond the LDS -- ids piled up in 1/256 of the
                    // range -- still takes the network, alone.
                    if (threadIdx.x < 64) { // exclusive scan of the 256 group sizes by one wave, 4 per lane; the cursors start there
                        uint32_t v4[4], sum = 0;
                        for (uint32_t k = 0; k < 4; ++k) { v4[k] = group_cur[threadIdx.x * 4 + k]; sum += v4[k]; }
                        uint32_t x = sum;
                        for (uint32_t d = 1; d < 64; d <<= 1) {
                            const uint32_t y = __shfl_up(x, d, 64);
                            if (threadIdx.x >= d) x += y;
                        }
                        uint32_t run = x - sum;
                        for (uint32_t k = 0; k < 4; ++k) { outer_at[threadIdx.x * 4 + k] = run; group_cur[threadIdx.x * 4 + k] = run; run += v4[k]; }
                        if (threadIdx.x == 63) outer_at[256] = run;
                    }
                    __syncthreads();
                    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
                        const uint64_t key = tmp[off + i];
                        dst[atomicAdd(&group_cur[(static_cast<uint32_t>(key) - g_low) >> g_shift], 1u)] = key;
                    }
                    __syncthreads();
                    for (uint32_t g_lo = g_done; g_lo < 256u;) { // (uniform: every thread reads the same LDS words)
                        const uint32_t start = outer_at[g_lo];
                        uint32_t g_hi = g_lo + 1u;
                        while (g_hi < 256u && outer_at[g_hi + 1u] - start <= LDS_HITS) ++g_hi;
                        const uint32_t n = outer_at[g_hi] - start;
                        g_lo = g_hi;
                        if (n == 0u) continue;
                        if (n <= LDS_HITS) {
                            for (uint32_t i = threadIdx.x; i < ((n + 3u) & ~3u); i += blockDim.x)
                                pos_lds[i] = i < n ? static_cast<uint32_t>(dst[start + i]) : 0xFFFFFFFFu;
                            __syncthreads();
                            sort_in_lds(n, dst + start);
                        } else {
                            wave_sort(dst + start, n);
                            __syncthreads();
                        }
                        walk(start, start + n);
                        if (walk_stopped != 0u) break;
                    }
                    walked = len; // (nothing is left for the walk below)
                }
            }
            if (st && threadIdx.x == 0 && s2 == 0) st[5] = __builtin_amdgcn_s_memrealtime();
            if (walk_stopped == 0u) walk(walked, len);
            if (walk_stopped != 0u) break; // uniform: the slices behind the exit are never sorted
        }
        if (threadIdx.x == 0) {
            out_mit[g] = 10000.0 / (100.0 + tot_mit); // :505
            out_cfd[g] = 10000.0 / (100.0 + tot_cfd); // :506
            if (out_kept) out_kept[g] = kept;
            if (st) { st[7] = __builtin_amdgcn_s_memrealtime(); st[8] = kept; }
        }
        __syncthreads();
    }
}

void launch_replay(const ImageView &v, const Workspace &ws, const uint64_t *d_guides, uint32_t n,
                   const ScoreParams &p, double *d_mit, double *d_cfd, uint32_t *d_kept, issl_hit *d_hitrec,
                   void *stream)
{
    if (n == 0) return;
    const uint32_t grid = n < 65536u ? n : 65536u;
    const auto replay = d_hitrec ? k_replay<true> : k_replay<false>;
    hipLaunchKernelGGL(replay, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream),
                       v, ws, d_guides, n, p, d_mit, d_cfd, d_kept, d_hitrec);
    if (ws.lean_tail) return; // (predicted: no guide with more than kReplayLds hits; k_replay checks)
    hipLaunchKernelGGL(k_replay_mid, dim3(2048), dim3(256), 0, static_cast<hipStream_t>(stream), v, ws, d_guides, p,
                       d_mit, d_cfd, d_kept, d_hitrec);
    hipLaunchKernelGGL((k_replay_big<256, 2048>), dim3(2048), dim3(256), 0, static_cast<hipStream_t>(stream), v, ws, d_guides, p,
                       d_mit, d_cfd, d_kept, d_hitrec);
    hipLaunchKernelGGL((k_replay_big<1024, kBigLds>), dim3(512), dim3(1024), 0, static_cast<hipStream_t>(stream), v, ws, d_guides, p,
                       d_mit, d_cfd, d_kept, d_hitrec);
}

} // namespace issl
