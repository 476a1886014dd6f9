// k_verify: the exact test of the scan's raw records, keys and MIT / CFD terms of the hits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "issl_kernels.hpp"

namespace issl {

// Exact check of the raw records, IN PLACE: one thread per record, one chunk per 128-thread workgroup.
// A record that survives becomes a hit: key guide<<37 | slice<<32 | site id (list-order layouts: position in the
// bucket's list), rank inside its guide from the per-guide counter, MIT / CFD terms.  With hit slots the first
// ws.slot_hits hits of a guide are written to its slots; what lies beyond overwrites the record with its key for the
// grouping pass; every other slot of the chunk becomes kDeadKey.  The rules are verify_record's (issl_kernels.hpp): the
// scan's waves apply them to the chunks they have filled themselves, between two of their units, and mark those chunks
// (kChunkVerified); this kernel takes what is not marked -- whole buckets, list-order layouts, the chunks beyond a wave's
// list of reservations, every chunk of a batch whose tail was not armed -- and carries the sticky flags.
// MARKS = false: the build for a batch whose scan had no tail (Workspace::scan_verify 0): no chunk can be marked, header and
// record are asked for together, as they were before there was a tail.
template <bool MARKS>
__global__ __launch_bounds__(kChunkRecs, 8) void k_verify(VerifyCtx c, const PlanInfo *__restrict__ plan, uint32_t *sticky, uint32_t cap_chunks)
{
    short_kernel_priority();
    const uint32_t prune_mode = plan->fine; // what the scan of this batch worked through
    uint32_t n_chunks = c.counters->raw_chunks;
    const bool none_marked = !MARKS || c.counters->scan_verified == 0u; // (a marked chunk has added its records to the counter)
    if (blockIdx.x == 0 && threadIdx.x == 0) { // what the host needs to know after any number of batches
        if (c.counters->raw_overflow) atomicOr(&sticky[0], 1u);
        atomicMax(&sticky[1], n_chunks + (MARKS ? c.counters->lds_chunks : 0u)); // (what the batch would ask for, run in full; lds_chunks: 0 but behind k_scan's build for lean batches)
        if (plan->error) atomicOr(&sticky[2], plan->error);
    }
    if (n_chunks > cap_chunks) n_chunks = cap_chunks;
    // a lean batch on the pruned plan (k_scan<THR, true, true>, launch_scan_thr): its waves note into LDS and say where the last
    // chunk with records is; where they verified everything there, none -- the launch and the sticky words are all that is left
    // of this kernel
    if (MARKS && c.lean_tail != 0u && prune_mode != 0u && c.counters->raw_top < n_chunks) n_chunks = c.counters->raw_top;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        // The passes behind the scan are chains of dependent loads at full occupancy: what they cost is the number of
        // links.  The chunk's header first: a chunk its scan wave has verified is left without asking for its records.
        // Then the record, then the stream record and the guide's signature (bucket-level plan: the guide slot's two
        // words) together, then -- nothing more before the exact test.
        // (Where the scan's waves verified nothing -- a small batch, a plan without a tail -- no chunk is marked, and header and
        // record are asked for together as they always were: the extra link is 2 us of a 64-guide batch's 64.)
        const uint64_t *recs = c.raw + static_cast<uint64_t>(chunk) * kChunkRecs;
        const uint32_t t = threadIdx.x + 1u;
        uint64_t rec_any = 0ull;
        if (none_marked) rec_any = recs[t < kChunkRecs ? t : 0u];
        const uint32_t used = c.raw_used[chunk];
        if (MARKS && (used & kChunkVerified)) continue;
        const bool in_use = t < used && t < kChunkRecs; // every lane stays: the counting is done by the wave
        const uint64_t rec = !in_use ? 0ull : none_marked ? rec_any : recs[t];
        verify_record<false>(c, prune_mode, rec, in_use, chunk, t, threadIdx.x & 63u);
    }
}

VerifyCtx make_verify_ctx(const ImageView &v, const Workspace &ws, const Tuning &tn, const uint64_t *d_guides, uint32_t n, const ScoreParams &p)
{
    VerifyCtx c;
    c.v = v;
    c.guides = d_guides;
    c.raw = ws.raw;
    c.raw_used = ws.raw_used;
    c.gidx = ws.gidx;
    c.gbucket = ws.gbucket;
    c.gcount = ws.gcount;
    c.slots = ws.slots;
    c.rank = ws.rank;
    c.pay = ws.pay;
    c.counters = ws.counters;
    c.n = n;
    c.slot_hits = ws.slot_hits;
    c.lean_tail = ws.lean_tail;
    c.max_dist = p.max_dist;
    c.calc_mit = (p.method == ISSL_METHOD_MIT || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR || p.method == ISSL_METHOD_AVG) ? 1u : 0u;
    c.calc_cfd = (p.method == ISSL_METHOD_CFD || p.method == ISSL_METHOD_AND || p.method == ISSL_METHOD_OR || p.method == ISSL_METHOD_AVG) ? 1u : 0u;
    (void)tn;
    c.scan_verify = (v.srec || v.sid) ? ws.scan_verify : 0u;
    return c;
}

void launch_verify(const ImageView &v, const Workspace &ws, const Tuning &tn, const uint64_t *d_guides, uint32_t n, const ScoreParams &p, void *stream)
{
    if (p.max_dist < 0) return;
    // (the kernel strides over the chunks the scan used: a small batch's few thousand need no 16 384 workgroups to start and leave)
    const uint32_t grid = n < 256u ? std::max<uint32_t>(2048u, 64u * n) : kTailGrid;
    const VerifyCtx c = make_verify_ctx(v, ws, tn, d_guides, n, p);
    if (c.scan_verify != 0u)
        hipLaunchKernelGGL(k_verify<true>, dim3(std::min(grid, kTailGrid)), dim3(kChunkRecs), 0, static_cast<hipStream_t>(stream), c, ws.plan, ws.sticky,
                           static_cast<uint32_t>(ws.cap_chunks));
    else
        hipLaunchKernelGGL(k_verify<false>, dim3(std::min(grid, kTailGrid)), dim3(kChunkRecs), 0, static_cast<hipStream_t>(stream), c, ws.plan, ws.sticky,
                           static_cast<uint32_t>(ws.cap_chunks));
}

} // namespace issl
