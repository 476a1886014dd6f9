// The ALT haplotypes of indels as text (issl_vcf_indels, issl_haplotypes_*; include/issl_hip.h).  An indel becomes a strip:
// the window - 1 bases ahead of the trimmed edit, ALT', the window - 1 bases behind it, cut from the resident text as it
// stands.  The strips, one record each, are a second issl_genome (text, starts, pos_bits), so the variant search
// (issl_variants.hip) searches them through its public entry points, unchanged.  This unit's own: the REF check of the
// entries against the resident text, the gather of the strips, and the pass that turns a row of the strip search (strip,
// offset) into a row in reference coordinates.  What these kernels do per byte and per row is issl_haplotypes_text.hpp's,
// which tools/haplotypes_sanitize.cpp checks on the CPU.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_genome_handle.hpp"
#include "issl_haplotypes_text.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"

struct issl_haplotypes {
    issl_genome strips;   // text, starts, one record per strip; device and timing as the genome's at the open
    issl::DevBuf table;   // haplotypes_text::Strip per strip
    uint32_t window = 0;
};

namespace issl {
namespace {

namespace ht = haplotypes_text;

constexpr uint32_t kWavesPerBlock = 4;

// One wave per entry, its lanes striding the bases of the untrimmed REF: every base lies in the set of its text byte, or
// *failed becomes the smallest index of an entry where one does not.  The host has checked that REF lies inside its record.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_indel_check(const uint8_t *__restrict__ s, const uint8_t *__restrict__ alleles,
                                                                     const ht::RefPlace *__restrict__ places, uint32_t n,
                                                                     uint32_t *__restrict__ failed)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (k >= n) return;
    const uint32_t lane = threadIdx.x & 63;
    const ht::RefPlace pl = places[k];
    bool bad = false;
    for (uint32_t i = lane; i < pl.ref_len; i += 64) bad |= !ht::ref_in_text(s[pl.at + i], alleles[pl.ref_at + i]);
    if (__ballot(bad) && lane == 0) atomicMin(failed, static_cast<uint32_t>(k));
}

// One wave per strip, its lanes striding the strip's bytes, the separator included.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_strip_build(const uint8_t *__restrict__ s, const uint8_t *__restrict__ alleles,
                                                                     const ht::Strip *__restrict__ strips,
                                                                     const ht::StripSource *__restrict__ sources, uint32_t n,
                                                                     uint8_t *__restrict__ out)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (k >= n) return;
    const ht::Strip t = strips[k];
    const ht::StripSource f = sources[k];
    const uint32_t bytes = ht::strip_length(t, f) + 1;
    for (uint32_t i = threadIdx.x & 63; i < bytes; i += 64) out[f.to + i] = ht::strip_byte(s, alleles, t, f, i);
}

// One thread per row: the 40-byte row of the strip search (record = strip, pos = offset in it) -> the 48-byte row.
__global__ __launch_bounds__(256) void k_haplotype_rows(const uint64_t *__restrict__ in, uint64_t total, const ht::Strip *__restrict__ strips,
                                                        uint64_t *__restrict__ out)
{
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j >= total) return;
    const uint64_t *row = in + 5 * j; // issl_variant_hit: pos, site[4], record | query, mism | strand | dist | n_var | reserved
    const uint32_t k = static_cast<uint32_t>(row[3]);
    const ht::Strip t = strips[k];
    uint64_t pos;
    int32_t edit_at;
    ht::strip_row(t, row[0], pos, edit_at);
    uint64_t *o = out + 6 * j; // issl_haplotype_hit: ..., indel | edit_at
    o[0] = pos;
    o[1] = row[1];
    o[2] = row[2];
    o[3] = t.record | (row[3] >> 32 << 32);
    o[4] = row[4];
    o[5] = k | (static_cast<uint64_t>(static_cast<uint32_t>(edit_at)) << 32);
}

int open_haplotypes(issl_genome *g, const issl_indel *indels, size_t n, const char *alleles, size_t alleles_len, int window,
                    issl_haplotypes **out)
{
    if (window < 1 || window > 32) {
        set_error("window " + std::to_string(window) + ": the pattern's length, 1 to 32");
        return ISSL_E_ARG;
    }
    if (n > 0xFFFFFFFFull) {
        set_error("more than 2^32 - 1 indels");
        return ISSL_E_UNSUPPORTED;
    }
    const RecordTable table(g);
    std::vector<ht::Strip> strips;
    std::vector<ht::StripSource> sources;
    std::vector<ht::RefPlace> places;
    std::vector<uint64_t> starts;
    uint64_t text_len = 0;
    std::string upper, err;
    if (!ht::plan_strips(indels, n, alleles, alleles_len, table.starts.data(), table.lengths.data(), table.size(), static_cast<uint32_t>(window),
                         strips, sources, places, starts, text_len, upper, err)) {
        set_error(err);
        return ISSL_E_ARG;
    }
    if (text_len >> 41) {
        set_error("strip text of " + std::to_string(text_len) + " bytes: a search word holds positions below 2^41");
        return ISSL_E_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(g->device));
    std::unique_ptr<issl_haplotypes> h(new issl_haplotypes());
    h->window = static_cast<uint32_t>(window);
    issl_genome &sg = h->strips;
    sg.device = g->device;
    sg.len = text_len;
    sg.pos_bits = bits_for(std::max<uint64_t>(2, sg.len));
    const char *timing = std::getenv("ISSL_LOCATE_TIMING");
    sg.timing = timing && timing[0] == '1';
    if (n == 0) {
        *out = h.release();
        return ISSL_OK;
    }
    sg.records.resize(n);
    for (size_t k = 0; k < n; ++k) {
        sg.records[k].start = starts[k];
        sg.records[k].length = ht::strip_length(strips[k], sources[k]);
        sg.n_bases += sg.records[k].length;
    }
    const uint32_t count = static_cast<uint32_t>(n), blocks = static_cast<uint32_t>((n + kWavesPerBlock - 1) / kWavesPerBlock);
    DevBuf d_alleles, d_places, d_sources, d_failed;
    HIP_TRY(hipMalloc(&d_alleles.p, upper.size()));
    HIP_TRY(hipMalloc(&d_places.p, sizeof(ht::RefPlace) * n));
    HIP_TRY(hipMalloc(&d_failed.p, 4));
    HIP_TRY(hipMemcpy(d_alleles.p, upper.data(), upper.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_places.p, places.data(), sizeof(ht::RefPlace) * n, hipMemcpyHostToDevice));
    uint32_t failed = 0xFFFFFFFFu;
    HIP_TRY(hipMemcpy(d_failed.p, &failed, 4, hipMemcpyHostToDevice));
    StageTimer clock(sg.timing, static_cast<hipStream_t>(nullptr));
    hipLaunchKernelGGL(k_indel_check, dim3(blocks), dim3(64 * kWavesPerBlock), 0, nullptr, static_cast<const uint8_t *>(g->seq.p),
                       static_cast<const uint8_t *>(d_alleles.p), static_cast<const ht::RefPlace *>(d_places.p), count,
                       static_cast<uint32_t *>(d_failed.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&failed, d_failed.p, 4, hipMemcpyDeviceToHost));
    clock.note("check");
    if (failed != 0xFFFFFFFFu) {
        set_error("indel " + std::to_string(failed) + ": the text does not hold its REF; no handle was made");
        return ISSL_E_ARG;
    }
    HIP_TRY(hipMalloc(&sg.seq.p, text_len));
    HIP_TRY(hipMalloc(&sg.starts.p, 8 * n));
    HIP_TRY(hipMalloc(&h->table.p, sizeof(ht::Strip) * n));
    HIP_TRY(hipMalloc(&d_sources.p, sizeof(ht::StripSource) * n));
    HIP_TRY(hipMemcpy(sg.starts.p, starts.data(), 8 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->table.p, strips.data(), sizeof(ht::Strip) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sources.p, sources.data(), sizeof(ht::StripSource) * n, hipMemcpyHostToDevice));
    clock.note("upload");
    hipLaunchKernelGGL(k_strip_build, dim3(blocks), dim3(64 * kWavesPerBlock), 0, nullptr, static_cast<const uint8_t *>(g->seq.p),
                       static_cast<const uint8_t *>(d_alleles.p), static_cast<const ht::Strip *>(h->table.p),
                       static_cast<const ht::StripSource *>(d_sources.p), count, static_cast<uint8_t *>(sg.seq.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    clock.note("build");
    if (sg.timing)
        std::fprintf(stderr, "[issl haplotypes] %u indels, window %d, %llu bytes of strips:%s\n", count, window,
                     static_cast<unsigned long long>(text_len), clock.line.c_str());
    *out = h.release();
    return ISSL_OK;
}

// The rows of a call whose counting call gave `total` > 0 rows (and d_offsets): the strip search's rows into a scratch of
// 40-byte rows, then this unit's pass over them into d_hits.  d_q, d_offsets, d_hits: device memory.
int fill_rows(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *d_q, size_t n, int max_dist, int max_variants,
              uint64_t *d_offsets, issl_haplotype_hit *d_hits, size_t total, size_t *n_total, hipStream_t stream)
{
    DevBuf scratch;
    HIP_TRY(hipMalloc(&scratch.p, sizeof(issl_variant_hit) * total));
    if (int rc = issl_genome_search_variants_device(&h->strips, pat, d_q, n, max_dist, max_variants, d_offsets,
                                                    static_cast<issl_variant_hit *>(scratch.p), total, n_total, stream))
        return rc;
    StageTimer clock(h->strips.timing, stream);
    hipLaunchKernelGGL(k_haplotype_rows, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint64_t *>(scratch.p), static_cast<uint64_t>(total), static_cast<const ht::Strip *>(h->table.p),
                       reinterpret_cast<uint64_t *>(d_hits));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    clock.note("map");
    if (h->strips.timing) std::fprintf(stderr, "[issl haplotypes]%s\n", clock.line.c_str());
    return ISSL_OK;
}

// pat->length is the window the strips were built for.
int check_window(const issl_haplotypes *h, const issl_search_pattern *pat)
{
    if (pat->length == h->window) return ISSL_OK;
    set_error("the pattern has " + std::to_string(pat->length) + " positions, the strips serve windows of " + std::to_string(h->window));
    return ISSL_E_ARG;
}

} // namespace
} // namespace issl

extern "C" {

int issl_vcf_indels(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                    size_t n_records, issl_indel *out, size_t cap, size_t *n, char *alleles, size_t alleles_cap, size_t *alleles_len,
                    issl_vcf_indel_counts *counts)
{
    if ((!vcf && len) || (n_records && (!names || !name_lens || !lengths)) || !n || !alleles_len || (!out && cap) || (!alleles && alleles_cap))
        return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        std::string err;
        if (issl::haplotypes_text::vcf_indels(vcf, len, names, name_lens, lengths, n_records, out, cap, n, alleles, alleles_cap, alleles_len,
                                              counts, err))
            return ISSL_OK;
        issl::set_error(err);
        return ISSL_E_ARG;
    });
}

int issl_haplotypes_open(issl_genome *g, const issl_indel *indels, size_t n, const char *alleles, size_t alleles_len, int window,
                         issl_haplotypes **out)
{
    if (out) *out = nullptr;
    if (!g || !out || (!indels && n) || (!alleles && alleles_len)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int { return issl::open_haplotypes(g, indels, n, alleles, alleles_len, window, out); });
}

int issl_haplotypes_open_vcf(issl_genome *g, const char *vcf, size_t len, int window, issl_vcf_indel_counts *counts, issl_haplotypes **out)
{
    if (out) *out = nullptr;
    if (!g || !out || (!vcf && len)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        const issl::RecordTable table(g);
        std::string err, alleles;
        std::vector<issl_indel> indels;
        issl_vcf_indel_counts c{};
        if (!issl::haplotypes_text::read_vcf_indels(vcf, len, table.names.data(), table.name_lens.data(), table.lengths.data(), table.size(), indels,
                                                    alleles, c, err)) {
            issl::set_error(err);
            return ISSL_E_ARG;
        }
        if (counts) *counts = c;
        return issl::open_haplotypes(g, indels.data(), indels.size(), alleles.data(), alleles.size(), window, out);
    });
}

int issl_haplotypes_info(const issl_haplotypes *h, uint64_t *n_indels, uint64_t *text_bytes, uint32_t *window)
{
    if (!h || !n_indels || !text_bytes || !window) return issl::fail(ISSL_E_ARG, "null argument");
    *n_indels = h->strips.records.size();
    *text_bytes = h->strips.len;
    *window = h->window;
    return ISSL_OK;
}

int issl_haplotypes_close(issl_haplotypes *h)
{
    if (!h) return ISSL_OK;
    if (h->strips.device >= 0) (void)hipSetDevice(h->strips.device);
    delete h;
    return ISSL_OK;
}

int issl_haplotypes_search(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                           int max_variants, uint64_t *offsets, issl_haplotype_hit *hits, size_t cap, size_t *n_total)
{
    if (!h || !pat || (!queries && n) || !offsets || !n_total || (!hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        if (int rc = issl::check_window(h, pat)) return rc;
        // the counting call of the host form checks the call and the queries, and gives offsets and the total
        if (int rc = issl_genome_search_variants(&h->strips, pat, queries, n, max_dist, max_variants, offsets, nullptr, 0, n_total)) return rc;
        const size_t total = *n_total;
        if (total == 0 || !hits || total > cap) return ISSL_OK;
        HIP_TRY(hipSetDevice(h->strips.device));
        issl::DevBuf d_q, d_offsets, d_hits;
        HIP_TRY(hipMalloc(&d_q.p, sizeof(issl_search_query) * n));
        HIP_TRY(hipMalloc(&d_offsets.p, 8 * (n + 1)));
        HIP_TRY(hipMalloc(&d_hits.p, sizeof(issl_haplotype_hit) * total));
        HIP_TRY(hipMemcpy(d_q.p, queries, sizeof(issl_search_query) * n, hipMemcpyHostToDevice));
        if (int rc = issl::fill_rows(h, pat, static_cast<const issl_search_query *>(d_q.p), n, max_dist, max_variants,
                                     static_cast<uint64_t *>(d_offsets.p), static_cast<issl_haplotype_hit *>(d_hits.p), total, n_total, nullptr))
            return rc;
        HIP_TRY(hipMemcpy(hits, d_hits.p, sizeof(issl_haplotype_hit) * total, hipMemcpyDeviceToHost));
        return ISSL_OK;
    });
}

int issl_haplotypes_search_device(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                  int max_dist, int max_variants, uint64_t *d_offsets, issl_haplotype_hit *d_hits, size_t cap,
                                  size_t *n_total, void *stream)
{
    if (!h || !pat || (!d_queries && n) || !d_offsets || !n_total || (!d_hits && cap)) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        if (int rc = issl::check_window(h, pat)) return rc;
        HIP_TRY(hipSetDevice(h->strips.device));
        // the counting call, then the filling call with room for the total
        if (int rc = issl_genome_search_variants_device(&h->strips, pat, d_queries, n, max_dist, max_variants, d_offsets, nullptr, 0, n_total, stream))
            return rc;
        const size_t total = *n_total;
        if (total == 0 || !d_hits || total > cap) return ISSL_OK;
        return issl::fill_rows(h, pat, d_queries, n, max_dist, max_variants, d_offsets, d_hits, total, n_total, static_cast<hipStream_t>(stream));
    });
}

int issl_haplotypes_search_profile(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *queries, size_t n,
                                   int max_dist, int max_variants, uint64_t *counts)
{
    if (!h || !pat || (n && (!queries || !counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        if (int rc = issl::check_window(h, pat)) return rc;
        return issl_genome_search_variants_profile(&h->strips, pat, queries, n, max_dist, max_variants, counts);
    });
}

int issl_haplotypes_search_profile_device(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *d_queries,
                                          size_t n, int max_dist, int max_variants, uint64_t *d_counts, void *stream)
{
    if (!h || !pat || (n && (!d_queries || !d_counts))) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        if (int rc = issl::check_window(h, pat)) return rc;
        return issl_genome_search_variants_profile_device(&h->strips, pat, d_queries, n, max_dist, max_variants, d_counts, stream);
    });
}

} // extern "C"
