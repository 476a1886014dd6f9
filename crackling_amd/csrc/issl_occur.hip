// The Bowtie step on a resident genome (issl_genome_occurrences*, include/issl_hip.h): Crackling.py:600-725 as an exact
// count of occurrences.  The reference aligns eight reads per guide -- its 20-mer followed by AGG, CGG, GGG, TGG, AAG, CAG,
// GAG, TAG -- and looks only at alignments without a mismatch.  A read occurs on strand 0 where the text holds it and on
// strand 1 where the text holds its reverse complement, so every occurrence is a window of 23 characters that matches
// [ACGT]{21}[AG]G (forward; 20-mer = the first 20, variant from characters 20 and 21) or C[CT][ACGT]{21} (reverse; 20-mer =
// the reverse complement of the last 20, variant from characters 2 and 1).
//
// One call, everything on one stream.  First a pass over all signatures for bits above the 20 bases.  Then, for a piece
// of up to 2^22 queries:
//   query prep   as for locate (issl_genome.hpp): keys sorted with their query index, runs collapsed to ranks, bitmap.
//                The sorted words of every piece are kept for the verdicts
//   scan         k_occur_scan, one pass over the text on the grid of k_match_*: occur_at reads a position's 23 bytes once
//                for both patterns; bitmap, then the binary search in the distinct keys.  A true occurrence updates the
//                state of its rank: an OR that sets the variant's "aligned" bit and, when it was set already, its
//                "repeated" bit; an add to the rank's 64-bit count; for variant 0 a minimum of position | strand.  All
//                three commute, so the state after the kernel is the same on every run.  A variant that is known to be
//                repeated is not written again: 200 000 occurrences of one read are two ORs and 200 000 adds
//   rows         k_occur_rows: one thread per query, a repeated one too: the counts of its rank to its row, and nb with
//                the first occurrence of read 0 as one word for the verdicts
// and behind the last piece, over all queries:
//   targets      k_occur_target: the query whose verdict a query's group of eight SAM lines sets, as the reference looks it
//                up (issl_hip.h: "verdicts"): the last query of the page with a given key, found by a binary search in
//                the sorted words of the pieces the page runs over.  Of the groups that name a query the last one wins:
//                an atomic maximum of group index + 1, which commutes.  A page is i / page_length, or, with explicit
//                boundaries (issl_genome_occurrences_paged*: the pages of a batched run start again with every batch),
//                the page whose [starts[p], starts[p + 1]) holds i, found by a binary search (k_occur_target_paged);
//                k_occur_pages_check refuses boundaries that do not tile [0, n) before any row is written
//   verdicts     k_occur_verdict: one thread per query completes its row from the word of its source
//   events       only for issl_genome_occurrences_paged_events_device: the reference's `failed` figure (Crackling.py:709-717)
//                counts, per page, the groups that reject the query they name while it is not rejected -- the groups are
//                walked in page order, and of a query named reject, accept, reject the rows know the last group only.
//                k_occur_target* leaves (named query << 32 | group) per group; a stable radix sort on the named query puts
//                every query's groups side by side in the order they are walked; k_occur_events counts a rejecting group
//                whose predecessor names another query or does not reject.  An output beside the rows: they do not change
// Pieces and pages change no row: a rank's state depends on the text and its key alone, and a page's queries are looked up
// wherever they lie.  The host waits for the signature check, once per piece before its buffers are released, and at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/issl_hip.h"
#include "issl_genome.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"

namespace issl {
namespace {

static_assert(sizeof(issl_occurrence) == 32, "issl_occurrence is 32 bytes");

constexpr uint32_t kLdsRecords = 4096; // record starts k_occur_verdict keeps in LDS (32 KiB)

constexpr unsigned long long kOwnFirst = 1ull << 42; // own word: bits 0..41 position << 1 | strand, 42 set when read 0 occurs,
constexpr uint32_t kOwnNbShift = 48;                 // 48.. nb

// State of one distinct key of a piece.
struct Ranks {
    uint32_t *flags;            // bits 0..7 aligned, 8..15 repeated
    unsigned long long *total;  // occurrences of all eight variants
    unsigned long long *first;  // least position << 1 | strand of variant 0, ~0 when there is none
};

// Occurrences at position i: bit 0 = forward, bit 1 = reverse; the key of each 20-mer (text order, as k_query_words) and
// its variant.  Both from the same 23 codes.
__device__ __forceinline__ uint32_t occur_at(const uint8_t *__restrict__ s, uint64_t i, uint64_t len, uint64_t &key_fwd,
                                             uint32_t &var_fwd, uint64_t &key_rev, uint32_t &var_rev)
{
    if (i + 23 > len) return 0;
    uint32_t code[23];
    bool body = true; // characters 2..20 are [ACGT] in both patterns
#pragma unroll
    for (int k = 0; k < 23; ++k) code[k] = base_code(s[i + k]);
#pragma unroll
    for (int k = 2; k <= 20; ++k) body = body && code[k] < 4u;
    if (!body) return 0;
    const bool fwd = code[0] < 4u && code[1] < 4u && (code[21] == 0u || code[21] == 2u) && code[22] == 2u;
    const bool rev = code[0] == 1u && (code[1] == 1u || code[1] == 3u) && code[21] < 4u && code[22] < 4u;
    if (!fwd && !rev) return 0;
    uint64_t kf = 0, kr = 0;
#pragma unroll
    for (int p = 0; p < 20; ++p) {
        kf |= static_cast<uint64_t>(code[p] & 3u) << (2 * (19 - p));
        kr |= static_cast<uint64_t>(3u - (code[22 - p] & 3u)) << (2 * (19 - p));
    }
    key_fwd = kf;
    key_rev = kr;
    var_fwd = code[20] + (code[21] == 0u ? 4u : 0u);
    var_rev = (3u - code[2]) + (code[1] == 3u ? 4u : 0u);
    return (fwd ? 1u : 0u) | (rev ? 2u : 0u);
}

// ---- queries -----------------------------------------------------------------------------------------------------

// *bad != 0: a signature carries bits above its 20 bases.
__global__ __launch_bounds__(256) void k_occur_check(const uint64_t *__restrict__ sites, uint64_t n, uint32_t *__restrict__ bad)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && (sites[i] >> 40)) *bad = 1u;
}

// *bad != 0: starts[0 .. n_pages] is not 0 = starts[0] <= starts[1] <= ... <= starts[n_pages] = n.
__global__ __launch_bounds__(256) void k_occur_pages_check(const uint64_t *__restrict__ starts, uint64_t n_pages, uint64_t n,
                                                           uint32_t *__restrict__ bad)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p > n_pages) return;
    const uint64_t at = starts[p];
    if ((p == 0 && at != 0) || (p == n_pages ? at != n : starts[p + 1] < at)) *bad = 1u;
}

// ---- the scan of the text ----------------------------------------------------------------------------------------

__device__ __forceinline__ void note_occurrence(const Ranks &st, uint32_t rank, uint32_t variant, uint64_t pos, uint32_t strand)
{
    const uint32_t one = 1u << variant, both = one | (one << 8);
    if ((__atomic_load_n(&st.flags[rank], __ATOMIC_RELAXED) & both) != both) {
        // which of two occurrences comes second does not matter: the second one, whichever it is, sets the bit
        if (atomicOr(&st.flags[rank], one) & one) atomicOr(&st.flags[rank], one << 8);
    }
    atomicAdd(&st.total[rank], 1ull);
    if (variant == 0) {
        const unsigned long long at = (pos << 1) | strand;
        if (__atomic_load_n(&st.first[rank], __ATOMIC_RELAXED) > at) atomicMin(&st.first[rank], at);
    }
}

// ctr[0]: occurrences of queried reads; ctr[1], ctr[2]: matches of the two patterns and those of them the bitmap let
// through (the figures of the timing line).  One atomic per counter and workgroup.
__global__ __launch_bounds__(256) void k_occur_scan(const uint8_t *__restrict__ s, uint64_t len, Probe q, Ranks st,
                                                    unsigned long long *__restrict__ ctr)
{
    __shared__ uint32_t wave_cnt[3][4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t nr = *q.n_ranks;
    uint32_t cnt = 0, matches = 0, passed = 0;
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a, b;
        uint32_t va, vb;
        const uint64_t pos = base + k;
        const uint32_t m = occur_at(s, pos, len, a, va, b, vb);
        matches += (m & 1u) + (m >> 1);
        if (m & 1u) {
            const int rank = probe_key(q, nr, a, passed);
            if (rank >= 0) {
                note_occurrence(st, static_cast<uint32_t>(rank), va, pos, 0u);
                ++cnt;
            }
        }
        if (m & 2u) {
            const int rank = probe_key(q, nr, b, passed);
            if (rank >= 0) {
                note_occurrence(st, static_cast<uint32_t>(rank), vb, pos, 1u);
                ++cnt;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        cnt += __shfl_down(cnt, d, 64);
        matches += __shfl_down(matches, d, 64);
        passed += __shfl_down(passed, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_cnt[0][threadIdx.x >> 6] = cnt;
        wave_cnt[1][threadIdx.x >> 6] = matches;
        wave_cnt[2][threadIdx.x >> 6] = passed;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t t = wave_cnt[threadIdx.x][0] + wave_cnt[threadIdx.x][1] + wave_cnt[threadIdx.x][2] + wave_cnt[threadIdx.x][3];
        if (t) atomicAdd(&ctr[threadIdx.x], static_cast<unsigned long long>(t));
    }
}

// ---- rows --------------------------------------------------------------------------------------------------------

// The counts of query i's rank to its row (the verdict's half is written by k_occur_verdict), and own[i].
__global__ __launch_bounds__(256) void k_occur_rows(const uint32_t *__restrict__ qrank, uint32_t n, Ranks st,
                                                    ulonglong2 *__restrict__ rows, unsigned long long *__restrict__ own)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = qrank[i];
    const uint32_t f = st.flags[r];
    const unsigned long long total = st.total[r], first = st.first[r];
    const uint32_t aligned = f & 0xFFu, repeated = (f >> 8) & 0xFFu;
    const uint32_t nb = static_cast<uint32_t>(__builtin_popcount(aligned) + __builtin_popcount(repeated));
    const uint64_t n_perfect = total > 0xFFFFFFFFull ? 0xFFFFFFFFull : total;
    rows[2ull * i] = make_ulonglong2(0ull, 0xFFFFFFFFull | (n_perfect << 32));
    rows[2ull * i + 1] = make_ulonglong2(static_cast<uint64_t>(aligned) | (static_cast<uint64_t>(repeated) << 8) |
                                             (static_cast<uint64_t>(nb) << 16),
                                         0ull);
    own[i] = (first != ~0ull ? (first | kOwnFirst) : 0ull) | (static_cast<unsigned long long>(nb) << kOwnNbShift);
}

// ---- verdicts ----------------------------------------------------------------------------------------------------

struct Pages {
    const uint64_t *sorted; // piece m's sorted words at sorted + (m << kPieceBits)
    uint64_t n, page_length;
};

// The last query of [lo, hi) -- one page, or a part of it -- that carries `key`, or ~0.
__device__ __forceinline__ uint64_t last_with_key(const Pages &pg, uint64_t key, uint64_t lo, uint64_t hi)
{
    for (uint64_t m = (hi - 1) >> kPieceBits;; --m) {
        const uint64_t base = m << kPieceBits;
        const uint64_t *w = pg.sorted + base;
        const uint32_t nm = static_cast<uint32_t>(pg.n - base < kPieceSites ? pg.n - base : kPieceSites);
        const uint64_t from = lo > base ? lo - base : 0, to = hi - base < nm ? hi - base : nm; // the piece's share of [lo, hi)
        const uint64_t bound = (key << kPieceBits) | (to - 1);
        uint32_t a = 0, b = nm; // first word above bound
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if (w[mid] <= bound) a = mid + 1;
            else b = mid;
        }
        if (a) {
            const uint64_t x = w[a - 1];
            if ((x >> kPieceBits) == key && (x & (kPieceSites - 1)) >= from) return base + (x & (kPieceSites - 1));
        }
        if (base <= lo) return ~0ull;
    }
}

// src[t]: 1 + the last query whose group names query t, 0 when none does.  [lo, hi): the page of query i.  named (may be
// null): named[i] = t << 32 | i, for the events.
__device__ __forceinline__ void note_target(const uint64_t *__restrict__ sites, const unsigned long long *__restrict__ own,
                                            const Pages &pg, uint32_t *__restrict__ src, uint64_t *__restrict__ named, uint64_t i,
                                            uint64_t lo, uint64_t hi)
{
    const uint64_t sig = sites[i];
    uint64_t key = 0;
#pragma unroll
    for (int p = 0; p < 20; ++p) key |= ((sig >> (2 * p)) & 3ull) << (2 * (19 - p));
    uint64_t t = ~0ull;
    const unsigned long long o = own[i];
    const uint32_t b0 = sig & 3u, b1 = (sig >> 2) & 3u;
    if ((o & kOwnFirst) && (o & 1ull) && b0 == 1u && (b1 == 1u || b1 == 3u)) {
        // read 0 is printed reverse-complemented: C, C or T, T, the rest of the guide backwards.  Its first 20 characters
        // may be another guide's 20-mer, and its last three, N[AG]G, are then one of that guide's reads
        uint64_t other = (1ull << 38) | (1ull << 36) | (3ull << 34); // C C T
#pragma unroll
        for (int j = 0; j < 17; ++j) other |= (3ull - ((sig >> (2 * (19 - j))) & 3ull)) << (2 * (16 - j));
        t = last_with_key(pg, other, lo, hi);
    }
    if (t == ~0ull) t = last_with_key(pg, key, lo, hi); // i itself at the least
    if (t != ~0ull) atomicMax(&src[t], static_cast<uint32_t>(i) + 1u);
    if (named) named[i] = (t << 32) | i; // (t == ~0: behind every query, and k_occur_events passes it over)
}

__global__ __launch_bounds__(256) void k_occur_target(const uint64_t *__restrict__ sites, const unsigned long long *__restrict__ own,
                                                      Pages pg, uint32_t *__restrict__ src)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= pg.n) return;
    const uint64_t lo = pg.page_length ? i / pg.page_length * pg.page_length : 0;
    const uint64_t hi = pg.page_length && pg.n - lo > pg.page_length ? lo + pg.page_length : pg.n;
    note_target(sites, own, pg, src, nullptr, i, lo, hi);
}

// First p in [0, n_pages] with starts[p] > i: at least 1, as starts[0] is 0.  The page of query i is p - 1.
__device__ __forceinline__ uint64_t page_above(const uint64_t *__restrict__ starts, uint64_t n_pages, uint64_t i)
{
    uint64_t a = 0, b = n_pages;
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (starts[mid] <= i) a = mid + 1;
        else b = mid;
    }
    return a;
}

// The same for pages given by their boundaries (checked by k_occur_pages_check): the page of query i is the last p with
// starts[p] <= i -- behind any empty page that starts there too -- and starts[n_pages] = n lies above every query.
__global__ __launch_bounds__(256) void k_occur_target_paged(const uint64_t *__restrict__ sites,
                                                            const unsigned long long *__restrict__ own, Pages pg,
                                                            const uint64_t *__restrict__ starts, uint64_t n_pages,
                                                            uint32_t *__restrict__ src, uint64_t *__restrict__ named)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= pg.n) return;
    const uint64_t a = page_above(starts, n_pages, i);
    note_target(sites, own, pg, src, named, i, starts[a - 1], starts[a]);
}

// named: the words of k_occur_target_paged, sorted by the query they name and, under one query, by group.  Group k counts
// for its page when it rejects and the group before it names another query or does not reject: the named query is not
// rejected at that moment.  One atomic per wave whose counting lanes share a page, else one per lane.
__global__ __launch_bounds__(256) void k_occur_events(const uint64_t *__restrict__ named, const unsigned long long *__restrict__ own,
                                                      uint64_t n, const uint64_t *__restrict__ starts, uint64_t n_pages,
                                                      uint32_t *__restrict__ events)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    bool counts = false;
    uint64_t page = 0;
    if (k < n) {
        const uint64_t x = named[k], i = x & 0xFFFFFFFFull;
        counts = (x >> 32) != 0xFFFFFFFFull && (own[i] >> kOwnNbShift) > 1u;
        if (counts && k) {
            const uint64_t y = named[k - 1];
            if ((y >> 32) == (x >> 32) && (own[y & 0xFFFFFFFFull] >> kOwnNbShift) > 1u) counts = false;
        }
        if (counts) page = page_above(starts, n_pages, i) - 1;
    }
    const uint64_t m = __ballot(counts);
    if (!m) return;
    const uint64_t page0 = __shfl(static_cast<unsigned long long>(page), __builtin_ctzll(m));
    if (__all(!counts || page == page0)) {
        if (lanes_before(m) == 0 && counts && page < n_pages) atomicAdd(&events[page], static_cast<uint32_t>(__popcll(m)));
    } else if (counts && page < n_pages) {
        atomicAdd(&events[page], 1u);
    }
}

// Row t: owner, code, source, and the first occurrence of read 0 of its source (its own when no group names it).
template <bool kLds>
__global__ __launch_bounds__(256) void k_occur_verdict(const unsigned long long *__restrict__ own, const uint32_t *__restrict__ src,
                                                       uint64_t n, const uint64_t *__restrict__ starts, uint32_t n_records,
                                                       ulonglong2 *__restrict__ rows)
{
    __shared__ uint64_t tab[kLds ? kLdsRecords : 1];
    if (kLds) {
        for (uint32_t r = threadIdx.x; r < n_records; r += 256) tab[r] = starts[r];
        __syncthreads();
    }
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    const uint32_t s = src[t];
    const unsigned long long o = own[s ? s - 1 : t];
    const uint64_t owner = s ? 1u : 0u;
    const uint64_t code = !s ? 2u : (o >> kOwnNbShift) > 1u ? 0u : 1u;
    uint64_t pos = 0, record = 0xFFFFFFFFull, strand = 0;
    if ((o & kOwnFirst) && n_records) {
        const uint64_t at = (o & (kOwnFirst - 1)) >> 1;
        const uint32_t rec = kLds ? last_not_above(tab, n_records, at) : last_not_above(starts, n_records, at);
        record = rec;
        pos = at - (kLds ? tab[rec] : starts[rec]);
        strand = o & 1ull;
    }
    // {pos; record, n_perfect} {aligned, repeated, nb, strand, owner, code, two zero bytes; source, four zero bytes}
    ulonglong2 head = rows[2 * t], tail = rows[2 * t + 1];
    head.x = pos;
    head.y = (head.y & 0xFFFFFFFF00000000ull) | record;
    tail.x = (tail.x & 0xFFFFFFull) | (strand << 24) | (owner << 32) | (code << 40);
    tail.y = s ? static_cast<uint64_t>(s - 1) : 0xFFFFFFFFull;
    rows[2 * t] = head;
    rows[2 * t + 1] = tail;
}

// ---- host --------------------------------------------------------------------------------------------------------

// Queries [at, at + n_piece) of the call: the counts of their rows, own[at ..], sorted_all[at ..].
int occur_piece(const issl_genome *g, const uint64_t *d_all, size_t at, size_t n_piece, uint64_t *sorted_all,
                unsigned long long *own_all, issl_occurrence *d_rows, hipStream_t stream)
{
    const uint32_t n = static_cast<uint32_t>(n_piece);
    StageTimer clock(g->timing, stream);
    const uint32_t q_blocks = (n + 255) / 256;
    Arena qa;
    QueryPrep prep;
    prep.reserve(qa, n);
    const size_t o_flags = qa.reserve(4ull * n), o_total = qa.reserve(8ull * n), o_min = qa.reserve(8ull * n);
    HIP_TRY(hipMalloc(&qa.buf.p, qa.size));
    const Ranks st{qa.at<uint32_t>(o_flags), qa.at<unsigned long long>(o_total), qa.at<unsigned long long>(o_min)};
    HIP_TRY(hipMemsetAsync(st.flags, 0, o_min - o_flags, stream)); // flags and total
    HIP_TRY(hipMemsetAsync(st.first, 0xFF, 8ull * n, stream));
    // -- query prep: the sorted words stay in sorted_all[at ..] for the verdicts
    if (int rc = prep.enqueue(qa, d_all + at, sorted_all + at, true, stream)) return rc;
    const Probe &probe = prep.probe;
    uint32_t *qrank = prep.qrank;
    unsigned long long *ctr = prep.ctr; // 0 occurrences, 1 matches, 2 passed
    HIP_TRY(hipGetLastError());
    clock.note("prep");
    // -- scan
    const uint32_t blocks = g->len < 23 ? 0u : static_cast<uint32_t>((g->len + kPosPerBlock - 1) / kPosPerBlock);
    if (blocks) {
        hipLaunchKernelGGL(k_occur_scan, dim3(blocks), dim3(256), 0, stream, static_cast<const uint8_t *>(g->seq.p), g->len, probe,
                           st, ctr);
        HIP_TRY(hipGetLastError());
    }
    clock.note("scan");
    // -- rows
    hipLaunchKernelGGL(k_occur_rows, dim3(q_blocks), dim3(256), 0, stream, qrank, n, st, reinterpret_cast<ulonglong2 *>(d_rows + at),
                       own_all + at);
    HIP_TRY(hipGetLastError());
    unsigned long long seen[3] = {};
    if (g->timing) HIP_TRY(hipMemcpyAsync(seen, ctr, sizeof seen, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // the piece's buffers are released on return
    clock.note("rows");
    if (g->timing)
        std::fprintf(stderr, "[issl occurrences] %u sites:%s | matches %llu filter passed %llu occurrences %llu\n", n,
                     clock.line.c_str(), seen[1], seen[2], seen[0]);
    return ISSL_OK;
}

// The pages of a call: page_length (0: one page), or, when d_starts is not null, n_pages + 1 boundaries in device memory.
struct PageSpec {
    size_t page_length;
    const uint64_t *d_starts;
    size_t n_pages;
    uint32_t *d_events = nullptr; // with d_starts: n_pages words, the events of every page
};

int occurrences_device(issl_genome *g, const uint64_t *d_sites, size_t n, const PageSpec &pages, issl_occurrence *d_rows,
                       hipStream_t stream)
{
    HIP_TRY(hipSetDevice(g->device));
    if (n == 0 && !(pages.d_starts && pages.n_pages)) return ISSL_OK;
    if (n >= 0xFFFFFFFFull) { // a row names its source in 32 bits
        set_error("more than 2^32 - 2 sites in one call: split the query at a page boundary");
        return ISSL_E_UNSUPPORTED;
    }
    if (pages.d_starts && pages.n_pages >= (size_t(1) << 39)) { // (2^31 - 1 workgroups of 256; n allows no more that hold a site)
        set_error("more than 2^39 pages in one call");
        return ISSL_E_UNSUPPORTED;
    }
    Arena all;
    const size_t o_sorted = all.reserve(8 * n), o_own = all.reserve(8 * n), o_src = all.reserve(4 * n), o_bad = all.reserve(8);
    const bool events = pages.d_events && pages.d_starts;
    const size_t o_named = all.reserve(events ? 8 * n : 0), o_named_tmp = all.reserve(events ? 8 * n : 0),
                 o_named_hist = all.reserve(events ? 4 * radix_hist_words(radix_sort_blocks(n)) : 0);
    HIP_TRY(hipMalloc(&all.buf.p, all.size));
    if (events && pages.n_pages) HIP_TRY(hipMemsetAsync(pages.d_events, 0, 4 * pages.n_pages, stream));
    uint64_t *sorted_all = all.at<uint64_t>(o_sorted);
    unsigned long long *own_all = all.at<unsigned long long>(o_own);
    uint32_t *src = all.at<uint32_t>(o_src), *bad = all.at<uint32_t>(o_bad); // bad[0]: signatures, bad[1]: boundaries
    const uint32_t blocks = static_cast<uint32_t>((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(bad, 0, 8, stream));
    if (n) hipLaunchKernelGGL(k_occur_check, dim3(blocks), dim3(256), 0, stream, d_sites, static_cast<uint64_t>(n), bad);
    if (pages.d_starts)
        hipLaunchKernelGGL(k_occur_pages_check, dim3(static_cast<uint32_t>(pages.n_pages / 256 + 1)), dim3(256), 0, stream,
                           pages.d_starts, static_cast<uint64_t>(pages.n_pages), static_cast<uint64_t>(n), bad + 1);
    HIP_TRY(hipGetLastError());
    uint32_t is_bad[2] = {};
    HIP_TRY(hipMemcpyAsync(is_bad, bad, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (is_bad[0]) {
        set_error("a signature carries bits above its 20 bases");
        return ISSL_E_ARG;
    }
    if (is_bad[1]) {
        set_error("page_starts: " + std::to_string(pages.n_pages + 1) + " boundaries that start at 0, never decrease and end at " +
                  std::to_string(n));
        return ISSL_E_ARG;
    }
    if (n == 0) return ISSL_OK;
    for (size_t at = 0; at < n; at += kPieceSites)
        if (int rc = occur_piece(g, d_sites, at, std::min(kPieceSites, n - at), sorted_all, own_all, d_rows, stream)) return rc;
    // -- verdicts
    StageTimer clock(g->timing, stream);
    HIP_TRY(hipMemsetAsync(src, 0, 4 * n, stream));
    const Pages pg{sorted_all, n, pages.d_starts ? 0 : pages.page_length};
    if (pages.d_starts)
        hipLaunchKernelGGL(k_occur_target_paged, dim3(blocks), dim3(256), 0, stream, d_sites, own_all, pg, pages.d_starts,
                           static_cast<uint64_t>(pages.n_pages), src, events ? all.at<uint64_t>(o_named) : nullptr);
    else
        hipLaunchKernelGGL(k_occur_target, dim3(blocks), dim3(256), 0, stream, d_sites, own_all, pg, src);
    HIP_TRY(hipGetLastError());
    const uint64_t *starts = static_cast<const uint64_t *>(g->starts.p);
    const uint32_t n_records = static_cast<uint32_t>(g->records.size());
    if (n_records <= kLdsRecords)
        hipLaunchKernelGGL(k_occur_verdict<true>, dim3(blocks), dim3(256), 0, stream, own_all, src, static_cast<uint64_t>(n), starts,
                           n_records, reinterpret_cast<ulonglong2 *>(d_rows));
    else
        hipLaunchKernelGGL(k_occur_verdict<false>, dim3(blocks), dim3(256), 0, stream, own_all, src, static_cast<uint64_t>(n), starts,
                           n_records, reinterpret_cast<ulonglong2 *>(d_rows));
    HIP_TRY(hipGetLastError());
    Events<2> ev;
    if (events) { // (the words lie in group order: a stable sort on the named query alone)
        clock.note("verdicts");
        if (g->timing) { // the sort and the count by HIP events, for the timing line
            if (int rc = ev.create()) return rc;
            HIP_TRY(hipEventRecord(ev.e[0], stream));
        }
        const uint64_t *named = radix_sort_async(all.at<uint64_t>(o_named), all.at<uint64_t>(o_named_tmp), n, 32, 64,
                                                 all.at<uint32_t>(o_named_hist), stream);
        hipLaunchKernelGGL(k_occur_events, dim3(blocks), dim3(256), 0, stream, named, own_all, static_cast<uint64_t>(n), pages.d_starts,
                           static_cast<uint64_t>(pages.n_pages), pages.d_events);
        HIP_TRY(hipGetLastError());
        if (ev.e[1]) HIP_TRY(hipEventRecord(ev.e[1], stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note(events ? "events" : "verdicts");
    if (ev.e[1]) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        char buf[64];
        std::snprintf(buf, sizeof buf, " (sort and k_occur_events %.4f ms by events)", ms);
        clock.line += buf;
    }
    if (g->timing) std::fprintf(stderr, "[issl occurrences]%s\n", clock.line.c_str());
    return ISSL_OK;
}

// pages.d_starts: HOST memory here.
int occurrences_host(issl_genome *g, const uint64_t *sites, size_t n, PageSpec pages, issl_occurrence *rows)
{
    HIP_TRY(hipSetDevice(g->device));
    if (n == 0 && !(pages.d_starts && pages.n_pages)) return ISSL_OK;
    // a page may run over several pieces and its verdicts are looked up in all of them: all queries at once
    DevBuf d_sites, d_rows, d_starts;
    if (n) {
        HIP_TRY(hipMalloc(&d_sites.p, 8 * n));
        HIP_TRY(hipMalloc(&d_rows.p, sizeof(issl_occurrence) * n));
        HIP_TRY(hipMemcpy(d_sites.p, sites, 8 * n, hipMemcpyHostToDevice));
    }
    if (pages.d_starts) {
        HIP_TRY(hipMalloc(&d_starts.p, 8 * (pages.n_pages + 1)));
        HIP_TRY(hipMemcpy(d_starts.p, pages.d_starts, 8 * (pages.n_pages + 1), hipMemcpyHostToDevice));
        pages.d_starts = static_cast<const uint64_t *>(d_starts.p);
    }
    if (int rc = occurrences_device(g, static_cast<const uint64_t *>(d_sites.p), n, pages, static_cast<issl_occurrence *>(d_rows.p),
                                    nullptr))
        return rc;
    if (n) HIP_TRY(hipMemcpy(rows, d_rows.p, sizeof(issl_occurrence) * n, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

int issl_genome_occurrences(issl_genome *g, const uint64_t *sites, size_t n, size_t page_length, issl_occurrence *rows)
{
    if (!g || (n && (!sites || !rows))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::occurrences_host(g, sites, n, issl::PageSpec{page_length, nullptr, 0}, rows); });
}

int issl_genome_occurrences_device(issl_genome *g, const uint64_t *d_sites, size_t n, size_t page_length, issl_occurrence *d_rows,
                                   void *stream)
{
    if (!g || (n && (!d_sites || !d_rows))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        return issl::occurrences_device(g, d_sites, n, issl::PageSpec{page_length, nullptr, 0}, d_rows, static_cast<hipStream_t>(stream));
    });
}

int issl_genome_occurrences_paged(issl_genome *g, const uint64_t *sites, size_t n, const uint64_t *page_starts, size_t n_pages,
                                  issl_occurrence *rows)
{
    if (!g || (n && (!sites || !rows)) || (!page_starts && (n || n_pages))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::occurrences_host(g, sites, n, issl::PageSpec{0, page_starts, n_pages}, rows); });
}

int issl_genome_occurrences_paged_device(issl_genome *g, const uint64_t *d_sites, size_t n, const uint64_t *d_page_starts,
                                         size_t n_pages, issl_occurrence *d_rows, void *stream)
{
    if (!g || (n && (!d_sites || !d_rows)) || (!d_page_starts && (n || n_pages))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        return issl::occurrences_device(g, d_sites, n, issl::PageSpec{0, d_page_starts, n_pages}, d_rows,
                                        static_cast<hipStream_t>(stream));
    });
}

int issl_genome_occurrences_paged_events_device(issl_genome *g, const uint64_t *d_sites, size_t n, const uint64_t *d_page_starts,
                                                size_t n_pages, issl_occurrence *d_rows, uint32_t *d_page_events, void *stream)
{
    if (!g || (n && (!d_sites || !d_rows)) || (!d_page_starts && (n || n_pages)) || (!d_page_events && n_pages))
        return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        return issl::occurrences_device(g, d_sites, n, issl::PageSpec{0, d_page_starts, n_pages, d_page_events}, d_rows,
                                        static_cast<hipStream_t>(stream));
    });
}

} // extern "C"
