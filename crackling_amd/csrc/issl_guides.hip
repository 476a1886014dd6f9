// Candidate guides from FASTA (issl_guides_*, include/issl_hip.h): the extraction step of Crackling.py:151-305 on the
// device.  Every 23-mer [ACGT]{21}GG (strand 0) and the reverse complement of every CC[ACGT]{21} (strand 1), upper case
// only, of the records that count; the distinct ones in the order the reference first meets them, each with the place of
// its first occurrence and the number of its occurrences.
//
// The reference walks file by file, record by record, and within a record first over all forward matches, then over
// all reverse matches.  The place of a match in that walk is its ordinal.  The text goes up at 1 B per base, '\n' behind
// every record, with the table of record starts.  Everything on one stream, made for the call:
//   count    k_guide_count on the grid of k_match_*: forward and reverse matches per workgroup (plain stores, one 64-bit
//            atomic per workgroup for the total); launch_scan turns them into the ranks in text order, per strand
//   bases    k_guide_bases: forward / reverse matches ahead of every record start = the scanned count of the start's
//            workgroup + a recount of the positions of that workgroup ahead of the start (nothing straddles a record)
//   emit     k_guide_emit: a match knows its rank in text order among the matches of its strand (workgroup base, rounds and
//            waves ahead of it in LDS, lanes ahead of it by ballot) and its record (a search between the records of the
//            workgroup's first and last position), hence its ordinal:
//              forward  rank + reverse matches of the records before its own
//              reverse  rank + forward matches of the records up to and including its own
//            and writes at index = ordinal: the 46-bit guide (base p at bits [2p, 2p + 2), A C G T = 0..3, as
//            encode_guide), text position << 1 | strand, and the sort word guide[0:32] << 32 | ordinal.  No atomic that
//            returns a place, and the ordinal is dense: 32 bits for 2^32 - 1 matches of a text of any length
//   sort     guide (46 bits) and ordinal (32 bits) are more than a word of radix_sort_async, so a permutation is sorted:
//            four stable passes over the low 32 guide bits the word carries, k_guide_high swaps them for the 14 high
//            ones (a gather through the ordinal), two more passes.  The words started in ordinal order and every pass
//            is stable: equal guides end up side by side, ordinals ascending
//   runs     k_guide_gather lines the full guides up in sorted order; k_guide_heads counts run heads per workgroup,
//            launch_scan ranks them; k_guide_ranks: a head writes where its run starts and its ordinal -- the least of
//            the run; k_guide_runs: one word per distinct guide, least ordinal << 32 | run length
//   files    k_guide_files, one thread per match in sorted order: the input of a match is found from its place in the
//            text, and the k-th word of a run is the guide's k-th occurrence in the reference's walk (ordinals ascend
//            inside a run).  Per input: its matches, those behind their run's head (they met a guide seen before), the
//            second words of runs (a guide becomes a repeated one here) and the heads (a new guide).  What the reference's
//            log prints per file (Crackling.py:254-258); the runs are gone once the call returns, so it is counted here.
//            Sums in LDS for the first kLdsFiles inputs, one global atomic per counter and workgroup
//   order    four passes over the ordinal half: distinct guides in first-seen order
//   finish   k_guide_finish: one thread per guide: guide and place through the ordinal, the record by a search in the
//            start table (in LDS up to 4096 records), one 32-byte record and the 40-bit signature of guide[0:20]
// The host waits three times: for the number of matches (sizes the buffers of the sort), for the number of distinct
// guides (sizes the output) and for the end.  Peak: the text + 32 B per match + 8 B per distinct guide + the output
// (40 B per distinct guide).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <functional>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <unordered_set>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_guides.hpp"
#include "issl_host.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"


namespace issl {
namespace {

constexpr uint32_t kLdsRecords = 4096; // record starts k_guide_finish keeps in LDS (32 KiB)
constexpr uint32_t kRounds = kPosPerBlock / 256;

static_assert(sizeof(issl_guide) == 32, "issl_guide is 32 bytes");
static_assert(kRounds == 16, "a thread keeps its matches of a strand in 16 bits, a wave scans 16 rounds x 4 waves");

// ---- the scan of the text ----------------------------------------------------------------------------------------

// Matches starting at position i: bit 0 = [ACGT]{21}GG, bit 1 = CC[ACGT]{21}; both from the same 23 codes.  guide_fwd:
// the 23 characters; guide_rev: their complement read backwards (only the guide of a set bit is meaningful).
__device__ __forceinline__ uint32_t guide_at(const uint8_t *__restrict__ s, uint64_t i, uint64_t len, uint64_t &guide_fwd,
                                             uint64_t &guide_rev)
{
    if (i + 23 > len) return 0;
    uint32_t code[23];
    bool body = true; // characters 2..20 are [ACGT] in both patterns
#pragma unroll
    for (int k = 0; k < 23; ++k) code[k] = base_code(s[i + k]);
#pragma unroll
    for (int k = 2; k <= 20; ++k) body = body && code[k] < 4u;
    if (!body) return 0;
    const bool fwd = code[0] < 4u && code[1] < 4u && code[21] == 2u && code[22] == 2u;
    const bool rev = code[0] == 1u && code[1] == 1u && code[21] < 4u && code[22] < 4u;
    if (!fwd && !rev) return 0;
    uint64_t gf = 0, gr = 0;
#pragma unroll
    for (int p = 0; p < 23; ++p) {
        gf |= static_cast<uint64_t>(code[p] & 3u) << (2 * p);
        gr |= static_cast<uint64_t>(3u - (code[22 - p] & 3u)) << (2 * p);
    }
    guide_fwd = gf;
    guide_rev = gr;
    return (fwd ? 1u : 0u) | (rev ? 2u : 0u);
}

// cnt_f[b], cnt_r[b]: matches of workgroup b's positions; *total: all of them, 64 bits, one atomic per workgroup.
__global__ __launch_bounds__(256) void k_guide_count(const uint8_t *__restrict__ s, uint64_t len, uint32_t *__restrict__ cnt_f,
                                                     uint32_t *__restrict__ cnt_r, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t wave_cnt[2][4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    uint32_t f = 0, r = 0;
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a, b;
        const uint32_t m = guide_at(s, base + k, len, a, b);
        f += m & 1u;
        r += m >> 1;
    }
    for (int d = 32; d > 0; d >>= 1) {
        f += __shfl_down(f, d, 64);
        r += __shfl_down(r, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_cnt[0][threadIdx.x >> 6] = f;
        wave_cnt[1][threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tf = wave_cnt[0][0] + wave_cnt[0][1] + wave_cnt[0][2] + wave_cnt[0][3];
        const uint32_t tr = wave_cnt[1][0] + wave_cnt[1][1] + wave_cnt[1][2] + wave_cnt[1][3];
        cnt_f[blockIdx.x] = tf;
        cnt_r[blockIdx.x] = tr;
        if (tf + tr) atomicAdd(total, static_cast<unsigned long long>(tf + tr));
    }
}

// rec_f[r], rec_r[r] (r = 0 .. n_records): matches at positions ahead of record r's start; r = n_records: ahead of the
// end of the text, that is all of them.  scan_f / scan_r: the scanned workgroup counts, n_blocks + 1 of them.
__global__ __launch_bounds__(256) void k_guide_bases(const uint8_t *__restrict__ s, uint64_t len, const uint64_t *__restrict__ starts,
                                                     uint32_t n_records, const uint32_t *__restrict__ scan_f,
                                                     const uint32_t *__restrict__ scan_r, uint32_t *__restrict__ rec_f,
                                                     uint32_t *__restrict__ rec_r)
{
    __shared__ uint32_t wave_cnt[2][4];
    for (uint64_t rec = blockIdx.x; rec <= n_records; rec += gridDim.x) {
        const uint64_t start = rec < n_records ? starts[rec] : len;
        const uint64_t block = start / kPosPerBlock, base = block * kPosPerBlock;
        const uint32_t ahead = static_cast<uint32_t>(start - base);
        uint32_t f = 0, r = 0;
        for (uint32_t k = threadIdx.x; k < ahead; k += 256) {
            uint64_t a, b;
            const uint32_t m = guide_at(s, base + k, len, a, b);
            f += m & 1u;
            r += m >> 1;
        }
        for (int d = 32; d > 0; d >>= 1) {
            f += __shfl_down(f, d, 64);
            r += __shfl_down(r, d, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            wave_cnt[0][threadIdx.x >> 6] = f;
            wave_cnt[1][threadIdx.x >> 6] = r;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            rec_f[rec] = scan_f[block] + wave_cnt[0][0] + wave_cnt[0][1] + wave_cnt[0][2] + wave_cnt[0][3];
            rec_r[rec] = scan_r[block] + wave_cnt[1][0] + wave_cnt[1][1] + wave_cnt[1][2] + wave_cnt[1][3];
        }
        __syncthreads();
    }
}

// Second pass.  A thread keeps which of its 16 positions matched, per strand, as 16 bits; ahead[strand][round * 4 + wave]
// becomes the number of the workgroup's matches in the rounds and waves before -- the positions of a round are
// consecutive, so (round, wave, lane) is the text order.  n: the number of matches, nothing is written at or above it.
// A matching position is read and packed a second time in the write loop (as k_locate_emit does) instead of keeping up to
// 16 guides per strand in registers; the alternative was not built, so what the second read costs is not measured.
__global__ __launch_bounds__(256) void k_guide_emit(const uint8_t *__restrict__ s, uint64_t len, const uint32_t *__restrict__ scan_f,
                                                    const uint32_t *__restrict__ scan_r, const uint64_t *__restrict__ starts,
                                                    uint32_t n_records, const uint32_t *__restrict__ rec_f,
                                                    const uint32_t *__restrict__ rec_r, uint64_t *__restrict__ keys,
                                                    uint64_t *__restrict__ places, uint64_t *__restrict__ words, uint32_t n)
{
    __shared__ uint32_t ahead[2][kRounds * 4];
    __shared__ uint32_t rec_range[2];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        const uint64_t last = (base + kPosPerBlock < len ? base + kPosPerBlock : len) - 1;
        rec_range[0] = last_not_above(starts, n_records, base);
        rec_range[1] = last_not_above(starts, n_records, last);
    }
    uint32_t fbits = 0, rbits = 0;
    for (uint32_t r = 0; r < kRounds; ++r) {
        uint64_t a, b;
        const uint32_t m = guide_at(s, base + r * 256 + threadIdx.x, len, a, b);
        fbits |= (m & 1u) << r;
        rbits |= (m >> 1) << r;
        const uint64_t bf = __ballot(m & 1u), br = __ballot(m >> 1);
        if (lane == 0) {
            ahead[0][r * 4 + wave] = static_cast<uint32_t>(__builtin_popcountll(bf));
            ahead[1][r * 4 + wave] = static_cast<uint32_t>(__builtin_popcountll(br));
        }
    }
    __syncthreads();
    if (wave < 2) { // exclusive scan of the 64 counts of strand `wave`
        const uint32_t x = ahead[wave][lane];
        uint32_t incl = x;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        ahead[wave][lane] = incl - x;
    }
    __syncthreads();
    const uint32_t rec_lo = rec_range[0], rec_cnt = rec_range[1] - rec_range[0] + 1;
    const uint32_t base_f = scan_f[blockIdx.x], base_r = scan_r[blockIdx.x];
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t two = ((fbits >> r) & 1u) | (((rbits >> r) & 1u) << 1);
        const uint64_t bf = __ballot(two & 1u), br = __ballot(two >> 1); // every lane takes part
        if (!two) continue;
        const uint64_t pos = base + r * 256 + threadIdx.x;
        uint64_t gf = 0, gr = 0;
        (void)guide_at(s, pos, len, gf, gr);
        const uint32_t rec = rec_lo + last_not_above(starts + rec_lo, rec_cnt, pos);
        if (two & 1u) {
            const uint32_t ord = base_f + ahead[0][r * 4 + wave] + lanes_before(bf) + rec_r[rec];
            if (ord < n) {
                keys[ord] = gf;
                places[ord] = pos << 1;
                words[ord] = (gf << 32) | ord;
            }
        }
        if (two & 2u) {
            const uint32_t ord = base_r + ahead[1][r * 4 + wave] + lanes_before(br) + rec_f[rec + 1];
            if (ord < n) {
                keys[ord] = gr;
                places[ord] = (pos << 1) | 1ull;
                words[ord] = (gr << 32) | ord;
            }
        }
    }
}

// ---- the permutation sort ------------------------------------------------------------------------------------------

// word = guide bits << 32 | ordinal: the low 32 guide bits are sorted, now the 14 above them.
__global__ __launch_bounds__(256) void k_guide_high(uint64_t *__restrict__ words, uint32_t n, const uint64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t ord = words[i] & 0xFFFFFFFFull;
    words[i] = ((keys[ord < n ? ord : 0] >> 32) << 32) | ord; // (an ordinal is below n; nothing is read beyond the keys)
}

__global__ __launch_bounds__(256) void k_guide_gather(const uint64_t *__restrict__ words, uint32_t n, const uint64_t *__restrict__ keys,
                                                      uint64_t *__restrict__ sorted_keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t ord = words[i] & 0xFFFFFFFFull;
    sorted_keys[i] = keys[ord < n ? ord : 0];
}

// ---- runs of equal guides --------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_guide_heads(const uint64_t *__restrict__ sorted_keys, uint32_t n, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool head = i < n && (i == 0 || sorted_keys[i - 1] != sorted_keys[i]);
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// first[b]: heads ahead of workgroup b.  The head of run k writes where the run starts and its ordinal, the least of
// the run; run_start[n_runs] = n closes the table.  Every address is written once.
__global__ __launch_bounds__(256) void k_guide_ranks(const uint64_t *__restrict__ sorted_keys, const uint64_t *__restrict__ words,
                                                     uint32_t n, const uint32_t *__restrict__ first, uint32_t n_runs,
                                                     uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_ord)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, wave = threadIdx.x >> 6;
    const bool head = i < n && (i == 0 || sorted_keys[i - 1] != sorted_keys[i]);
    const uint64_t heads = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(heads));
    __syncthreads();
    uint32_t rank = first[blockIdx.x] + lanes_before(heads);
    for (uint32_t v = 0; v < wave; ++v) rank += wave_cnt[v];
    if (head && rank < n_runs) {
        run_start[rank] = i;
        run_ord[rank] = static_cast<uint32_t>(words[i]);
    }
    if (i == 0) run_start[n_runs] = n;
}

__global__ __launch_bounds__(256) void k_guide_runs(const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ run_ord,
                                                    uint32_t n_runs, uint64_t *__restrict__ out)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n_runs) out[k] = (static_cast<uint64_t>(run_ord[k]) << 32) | (run_start[k + 1] - run_start[k]);
}

// ---- finish ------------------------------------------------------------------------------------------------------------

// Guide j of the set: runs[j] = ordinal of its first occurrence (below n, the number of matches) << 32 | occurrences.  *n_unique: guides seen once, one
// atomic per workgroup.
template <bool kLds>
__global__ __launch_bounds__(256) void k_guide_finish(const uint64_t *__restrict__ runs, uint32_t n_runs, const uint64_t *__restrict__ keys,
                                                      const uint64_t *__restrict__ places, uint32_t n, const uint64_t *__restrict__ starts,
                                                      uint32_t n_records, ulonglong2 *__restrict__ guides, uint64_t *__restrict__ sigs,
                                                      unsigned long long *__restrict__ n_unique)
{
    __shared__ uint64_t tab[kLds ? kLdsRecords : 1];
    __shared__ uint32_t wave_cnt[4];
    if (kLds) {
        for (uint32_t r = threadIdx.x; r < n_records; r += 256) tab[r] = starts[r];
        __syncthreads();
    }
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    bool once = false;
    if (j < n_runs) {
        const uint64_t run = runs[j], ord = (run >> 32) < n ? run >> 32 : 0, seen = run & 0xFFFFFFFFull;
        const uint64_t guide = keys[ord], place = places[ord], pos = place >> 1;
        const uint32_t rec = kLds ? last_not_above(tab, n_records, pos) : last_not_above(starts, n_records, pos);
        const uint64_t start = kLds ? tab[rec] : starts[rec];
        guides[2 * static_cast<uint64_t>(j)] = make_ulonglong2(guide, pos - start);                       // {guide23, start}
        guides[2 * static_cast<uint64_t>(j) + 1] = make_ulonglong2(rec | ((place & 1ull) << 32), seen);   // {record, strand, seen, 0}
        sigs[j] = guide & ((1ull << 40) - 1);
        once = seen == 1;
    }
    const uint64_t ones = __ballot(once);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__builtin_popcountll(ones));
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (t) atomicAdd(n_unique, static_cast<unsigned long long>(t));
    }
}

// counts[4 f ..]: matches, duplicates, second occurrences, first occurrences of input f (see "files" above).
constexpr uint32_t kLdsFiles = 256;
__global__ __launch_bounds__(256) void k_guide_files(const uint64_t *__restrict__ perm, const uint64_t *__restrict__ sorted_keys,
                                                     const uint64_t *__restrict__ places, uint32_t n,
                                                     const uint64_t *__restrict__ file_starts, uint32_t n_files,
                                                     uint32_t *__restrict__ counts)
{
    __shared__ uint32_t local[4 * kLdsFiles];
    const uint32_t n_local = n_files < kLdsFiles ? n_files : kLdsFiles;
    for (uint32_t c = threadIdx.x; c < 4 * n_local; c += 256) local[c] = 0;
    __syncthreads();
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        const uint64_t ord = perm[k] & 0xFFFFFFFFull, key = sorted_keys[k];
        const uint32_t file = last_not_above(file_starts, n_files, places[ord < n ? ord : 0] >> 1);
        const bool head = k == 0 || sorted_keys[k - 1] != key;
        const bool second = !head && (k == 1 || sorted_keys[k - 2] != key);
        uint32_t *to = file < kLdsFiles ? local + 4 * file : counts + 4ull * file;
        atomicAdd(to, 1u);
        atomicAdd(to + (head ? 3 : 1), 1u);
        if (second) atomicAdd(to + 2, 1u);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < 4 * n_local; c += 256)
        if (local[c]) atomicAdd(counts + c, local[c]);
}

// ---- host: the FASTA pass ------------------------------------------------------------------------------------------

// What str.strip() removes from ASCII text (py_blank of issl_extract.hip).
inline bool py_blank(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

// The records of one input that count (Crackling.py:193-252) appended to text, '\n' behind each.  Lines end at "\n",
// "\r\n" or a lone "\r" (Python's text mode) and are stripped; '>' first makes a header.  A record is finished by the
// next header and counts when its name is not in `recorded` -- or is empty while the sequence is not; it is then
// recorded.  The last record of the input counts whatever its name and is not recorded.  The record ahead of the first
// header has no name; without text it is no record.  what: the input's name for the message of a blank line.
int append_guide_records(const char *data, size_t len, const std::string &what, std::unordered_set<std::string> &recorded,
                         std::string &text, std::vector<FastaRecord> &records)
{
    std::string name;
    size_t rec_at = text.size();
    bool headed = false;
    auto finish = [&](bool last) {
        const size_t seq_len = text.size() - rec_at;
        const bool counts = last || !recorded.count(name) || (name.empty() && seq_len);
        if (counts && !last) recorded.insert(name);
        if (counts && (headed || seq_len)) {
            records.push_back({rec_at, seq_len, name});
            text.push_back('\n');
        } else {
            text.resize(rec_at);
        }
        rec_at = text.size();
    };
    size_t p = 0, line = 0;
    while (p < len) {
        size_t e = p;
        while (e < len && data[e] != '\n' && data[e] != '\r') ++e;
        size_t next = e < len ? e + 1 : len;
        if (e + 1 < len && data[e] == '\r' && data[e + 1] == '\n') ++next;
        ++line;
        size_t a = p, b = e;
        while (a < b && py_blank(data[a])) ++a;
        while (b > a && py_blank(data[b - 1])) --b;
        if (a == b) {
            set_error(what + " line " + std::to_string(line) + ": blank line (the reference stops here with an IndexError)");
            return ISSL_E_FORMAT;
        }
        if (data[a] == '>') {
            finish(false);
            name.assign(data + a + 1, b - a - 1);
            headed = true;
        } else {
            text.append(data + a, b - a);
        }
        p = next;
    }
    finish(true);
    return ISSL_OK;
}

// A lone directory stands for its files, top level only, in reverse sorted name order (ConfigManager.py:181-184).
int expand_guide_inputs(const char *const *paths, int n, std::vector<std::string> &inputs)
{
    struct stat st;
    if (n == 1 && ::stat(paths[0], &st) == 0 && S_ISDIR(st.st_mode)) {
        const std::string dir = paths[0];
        std::vector<std::string> names;
        if (DIR *d = ::opendir(dir.c_str())) {
            while (dirent *e = ::readdir(d)) {
                const std::string full = dir + "/" + e->d_name;
                if (::stat(full.c_str(), &st) == 0 && S_ISREG(st.st_mode)) names.push_back(e->d_name);
            }
            ::closedir(d);
        }
        std::sort(names.begin(), names.end(), std::greater<std::string>());
        for (const auto &f : names) inputs.push_back(dir + "/" + f);
        if (inputs.empty()) {
            set_error("no file in '" + dir + "'");
            return ISSL_E_IO;
        }
        return ISSL_OK;
    }
    inputs.assign(paths, paths + n);
    return ISSL_OK;
}

// ---- host: the device pass -----------------------------------------------------------------------------------------

// text and its records -> the set on `device`.  parse_ms: the host pass, for the timing line.
int extract_guides(const std::string &text, std::vector<FastaRecord> &records, std::vector<uint64_t> &file_starts, int device,
                   bool timing, double parse_ms, issl_guide_set **out)
{
    if (int rc = select_device(device, "the extraction")) return rc;
    const uint64_t len = text.size();
    if (len >> 41) {
        set_error("text of " + std::to_string(len) + " bytes: a guide's place holds positions below 2^41");
        return ISSL_E_UNSUPPORTED;
    }
    if (records.size() >= 0xFFFFFFFFull) {
        set_error("more than 2^32 - 2 records");
        return ISSL_E_UNSUPPORTED;
    }
    std::unique_ptr<issl_guide_set> g(new issl_guide_set());
    g->device = device;
    const uint32_t n_files = static_cast<uint32_t>(file_starts.size());
    file_starts.push_back(len);
    g->file_counts.assign(4ull * n_files, 0u);
    const uint32_t n_records = static_cast<uint32_t>(records.size());
    OwnedStream own; // ahead of the arenas: they are released first
    HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t stream = own.s;
    StageTimer clock(timing, stream);
    uint64_t n = 0;
    uint32_t n_runs = 0;
    unsigned long long ctr[2] = {}; // 0 matches, 1 guides seen once
    if (len >= 23 && n_records) {
        // -- the text, the record starts and what the text's size fixes
        const uint32_t blocks = static_cast<uint32_t>((len + kPosPerBlock - 1) / kPosPerBlock);
        Arena ta;
        const size_t o_seq = ta.reserve(len), o_starts = ta.reserve(8ull * n_records), o_ctr = ta.reserve(16),
                     o_cf = ta.reserve(4 * scan_words(blocks + 1ull)), o_cr = ta.reserve(4 * scan_words(blocks + 1ull)),
                     o_rf = ta.reserve(4 * (n_records + 1ull)), o_rr = ta.reserve(4 * (n_records + 1ull));
        HIP_TRY(hipMalloc(&ta.buf.p, ta.size));
        uint8_t *d_seq = ta.at<uint8_t>(o_seq);
        uint64_t *d_starts = ta.at<uint64_t>(o_starts);
        unsigned long long *d_ctr = ta.at<unsigned long long>(o_ctr);
        uint32_t *cnt_f = ta.at<uint32_t>(o_cf), *cnt_r = ta.at<uint32_t>(o_cr), *rec_f = ta.at<uint32_t>(o_rf),
                 *rec_r = ta.at<uint32_t>(o_rr);
        std::vector<uint64_t> starts(n_records);
        for (uint32_t r = 0; r < n_records; ++r) starts[r] = records[r].start;
        HIP_TRY(hipMemcpyAsync(d_seq, text.data(), len, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_starts, starts.data(), 8ull * n_records, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_ctr, 0, 16, stream));
        HIP_TRY(hipMemsetAsync(cnt_f + blocks, 0, 4, stream));
        HIP_TRY(hipMemsetAsync(cnt_r + blocks, 0, 4, stream));
        clock.note("upload");
        // -- count
        hipLaunchKernelGGL(k_guide_count, dim3(blocks), dim3(256), 0, stream, d_seq, len, cnt_f, cnt_r, d_ctr);
        HIP_TRY(hipGetLastError()); // a launch that fails is reported as such, at its stage
        HIP_TRY(hipMemcpyAsync(ctr, d_ctr, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        clock.note("count");
        n = ctr[0];
        if (n > 0xFFFFFFFFull) { // ordinals and the offsets of the radix passes are 32 bits (issl_radix.hpp)
            set_error("more than 2^32 - 1 matches in one call (" + std::to_string(n) + "): split the input");
            return ISSL_E_UNSUPPORTED;
        }
        if (n) {
            const uint32_t n32 = static_cast<uint32_t>(n), n_blocks = (n32 + 255) / 256;
            // -- ranks in text order, per strand, and the counts ahead of every record
            launch_scan(cnt_f, blocks + 1ull, stream);
            launch_scan(cnt_r, blocks + 1ull, stream);
            hipLaunchKernelGGL(k_guide_bases, dim3(std::min<uint32_t>(n_records + 1u, 1u << 20)), dim3(256), 0, stream, d_seq, len,
                               d_starts, n_records, cnt_f, cnt_r, rec_f, rec_r);
            HIP_TRY(hipGetLastError());
            // -- emit
            Arena ma;
            const size_t o_keys = ma.reserve(8 * n), o_places = ma.reserve(8 * n), o_wa = ma.reserve(8 * n), o_wb = ma.reserve(8 * n),
                         o_hist = ma.reserve(4 * radix_hist_words(radix_sort_blocks(n))),
                         o_first = ma.reserve(4 * scan_words(n_blocks + 1ull));
            HIP_TRY(hipMalloc(&ma.buf.p, ma.size));
            uint64_t *keys = ma.at<uint64_t>(o_keys), *places = ma.at<uint64_t>(o_places), *wa = ma.at<uint64_t>(o_wa),
                     *wb = ma.at<uint64_t>(o_wb);
            uint32_t *hist = ma.at<uint32_t>(o_hist), *first = ma.at<uint32_t>(o_first);
            hipLaunchKernelGGL(k_guide_emit, dim3(blocks), dim3(256), 0, stream, d_seq, len, cnt_f, cnt_r, d_starts, n_records, rec_f,
                               rec_r, keys, places, wa, n32);
            HIP_TRY(hipGetLastError());
            clock.note("emit");
            // -- the permutation by guide, ordinals ascending inside a run
            uint64_t *low = radix_sort_async(wa, wb, n, 32, 64, hist, stream);
            hipLaunchKernelGGL(k_guide_high, dim3(n_blocks), dim3(256), 0, stream, low, n32, keys);
            uint64_t *perm = radix_sort_async(low, low == wa ? wb : wa, n, 32, 48, hist, stream);
            uint64_t *sorted_keys = perm == wa ? wb : wa;
            hipLaunchKernelGGL(k_guide_gather, dim3(n_blocks), dim3(256), 0, stream, perm, n32, keys, sorted_keys);
            HIP_TRY(hipGetLastError());
            clock.note("sort");
            // -- runs
            HIP_TRY(hipMemsetAsync(first + n_blocks, 0, 4, stream));
            hipLaunchKernelGGL(k_guide_heads, dim3(n_blocks), dim3(256), 0, stream, sorted_keys, n32, first);
            launch_scan(first, n_blocks + 1ull, stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&n_runs, first + n_blocks, 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (n_runs == 0 || n_runs > n32) {
                set_error("guide collapse on the device: " + std::to_string(n_runs) + " distinct of " + std::to_string(n) + " matches");
                return ISSL_E_DEVICE;
            }
            Arena ra;
            const size_t o_rs = ra.reserve(4 * (n_runs + 1ull)), o_ro = ra.reserve(4ull * n_runs), o_fs = ra.reserve(8ull * n_files),
                         o_fc = ra.reserve(16ull * n_files);
            HIP_TRY(hipMalloc(&ra.buf.p, ra.size));
            HIP_TRY(hipMalloc(&g->guides.p, 32ull * n_runs));
            HIP_TRY(hipMalloc(&g->sigs.p, 8ull * n_runs));
            uint32_t *run_start = ra.at<uint32_t>(o_rs), *run_ord = ra.at<uint32_t>(o_ro);
            hipLaunchKernelGGL(k_guide_ranks, dim3(n_blocks), dim3(256), 0, stream, sorted_keys, perm, n32, first, n_runs, run_start,
                               run_ord);
            // -- per input, while the runs are there (in the arena of the runs: no allocation of its own)
            HIP_TRY(hipMemcpyAsync(ra.at<uint64_t>(o_fs), file_starts.data(), 8ull * n_files, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(ra.at<uint32_t>(o_fc), 0, 16ull * n_files, stream));
            Events<2> fe;
            if (timing) { // the kernel alone by HIP events, for the timing line
                if (int rc = fe.create()) return rc;
                HIP_TRY(hipEventRecord(fe.e[0], stream));
            }
            hipLaunchKernelGGL(k_guide_files, dim3(n_blocks), dim3(256), 0, stream, perm, sorted_keys, places, n32, ra.at<uint64_t>(o_fs),
                               n_files, ra.at<uint32_t>(o_fc));
            if (timing) HIP_TRY(hipEventRecord(fe.e[1], stream));
            HIP_TRY(hipMemcpyAsync(g->file_counts.data(), ra.at<uint32_t>(o_fc), 16ull * n_files, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipGetLastError());
            clock.note("files");
            if (timing) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, fe.e[0], fe.e[1])); // (note() synchronised the stream)
                char buf[64];
                std::snprintf(buf, sizeof buf, " (k_guide_files %.4f ms by events)", ms);
                clock.line += buf;
            }
            // perm and sorted_keys are read no more: the run words and the scratch of their sort take the two buffers
            const dim3 run_grid((n_runs + 255) / 256);
            hipLaunchKernelGGL(k_guide_runs, run_grid, dim3(256), 0, stream, run_start, run_ord, n_runs, wa);
            HIP_TRY(hipGetLastError());
            clock.note("runs");
            // -- first-seen order
            const uint64_t *runs = radix_sort_async(wa, wb, n_runs, 32, 64, hist, stream);
            HIP_TRY(hipGetLastError());
            clock.note("order");
            // -- finish
            ulonglong2 *d_guides = static_cast<ulonglong2 *>(g->guides.p);
            uint64_t *d_sigs = static_cast<uint64_t *>(g->sigs.p);
            if (n_records <= kLdsRecords)
                hipLaunchKernelGGL(k_guide_finish<true>, run_grid, dim3(256), 0, stream, runs, n_runs, keys, places, n32, d_starts, n_records,
                                   d_guides, d_sigs, d_ctr + 1);
            else
                hipLaunchKernelGGL(k_guide_finish<false>, run_grid, dim3(256), 0, stream, runs, n_runs, keys, places, n32, d_starts, n_records,
                                   d_guides, d_sigs, d_ctr + 1);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ctr + 1, d_ctr + 1, 8, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            clock.note("finish");
        }
    }
    if (timing)
        std::fprintf(stderr, "[issl guides] %llu bytes: parse %.3f ms%s | matches %llu guides %u unique %llu\n",
                     static_cast<unsigned long long>(len), parse_ms, clock.line.c_str(), ctr[0], n_runs, ctr[1]);
    g->n_matches = n;
    g->n_guides = n_runs;
    g->n_unique = ctr[1];
    g->records = std::move(records);
    g->file_starts = std::move(file_starts);
    *out = g.release();
    return ISSL_OK;
}

int copy_guides(const issl_guide_set *g, issl_guide *out)
{
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipMemcpy(out, g->guides.p, 32 * g->n_guides, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

bool timing_wanted()
{
    const char *t = std::getenv("ISSL_GUIDES_TIMING");
    return t && t[0] == '1';
}

} // namespace
} // namespace issl

extern "C" {

int issl_guides_extract(const char *const *files, const size_t *lens, int n_files, int device, issl_guide_set **out)
{
    if (out) *out = nullptr;
    if (!files || !lens || n_files <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    for (int f = 0; f < n_files; ++f)
        if (!files[f] && lens[f]) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        const bool timing = issl::timing_wanted();
        const double t0 = issl::now_ms();
        std::string text;
        std::vector<issl::FastaRecord> records;
        std::unordered_set<std::string> recorded;
        std::vector<uint64_t> file_starts;
        for (int f = 0; f < n_files; ++f) {
            file_starts.push_back(text.size());
            if (int rc = issl::append_guide_records(files[f], lens[f], "input " + std::to_string(f), recorded, text, records)) return rc;
        }
        return issl::extract_guides(text, records, file_starts, device, timing, issl::now_ms() - t0, out);
    });
}

int issl_guides_extract_files(const char *const *paths, int n_paths, int device, issl_guide_set **out)
{
    if (out) *out = nullptr;
    if (!paths || n_paths <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    for (int f = 0; f < n_paths; ++f)
        if (!paths[f]) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        const bool timing = issl::timing_wanted();
        const double t0 = issl::now_ms();
        std::vector<std::string> inputs;
        if (int rc = issl::expand_guide_inputs(paths, n_paths, inputs)) return rc;
        std::string text;
        std::vector<issl::FastaRecord> records;
        std::unordered_set<std::string> recorded;
        std::vector<char> buf;
        std::vector<uint64_t> file_starts;
        for (const auto &path : inputs) {
            file_starts.push_back(text.size());
            if (int rc = issl::read_whole_file(path.c_str(), buf)) return rc;
            if (int rc = issl::append_guide_records(buf.data(), buf.size(), "'" + path + "'", recorded, text, records)) return rc;
        }
        buf = std::vector<char>();
        return issl::extract_guides(text, records, file_starts, device, timing, issl::now_ms() - t0, out);
    });
}

int issl_guides_info(const issl_guide_set *g, uint64_t *n_guides, uint64_t *n_unique, uint64_t *n_matches, uint64_t *n_records)
{
    if (!g || !n_guides || !n_unique || !n_matches || !n_records) return issl::fail(ISSL_E_ARG, "null argument");
    *n_guides = g->n_guides;
    *n_unique = g->n_unique;
    *n_matches = g->n_matches;
    *n_records = g->records.size();
    return ISSL_OK;
}

int issl_guides_record(const issl_guide_set *g, uint64_t r, const char **name, size_t *name_len, uint64_t *length)
{
    if (!g || !name || !name_len || !length) return issl::fail(ISSL_E_ARG, "null argument");
    if (r >= g->records.size()) {
        issl::set_error("record out of range");
        return ISSL_E_ARG;
    }
    *name = g->records[r].name.data();
    *name_len = g->records[r].name.size();
    *length = g->records[r].length;
    return ISSL_OK;
}

int issl_guides_files(const issl_guide_set *g, uint64_t *n_files)
{
    if (!g || !n_files) return issl::fail(ISSL_E_ARG, "null argument");
    *n_files = g->file_counts.size() / 4;
    return ISSL_OK;
}

int issl_guides_file_counts(const issl_guide_set *g, uint64_t file, issl_guides_file *out)
{
    if (!g || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (file >= g->file_counts.size() / 4) {
        issl::set_error("input " + std::to_string(file) + " of " + std::to_string(g->file_counts.size() / 4));
        return ISSL_E_ARG;
    }
    const uint32_t *c = g->file_counts.data() + 4 * file;
    *out = issl_guides_file{c[0], c[1], c[2], c[3]};
    return ISSL_OK;
}

int issl_guides_copy(const issl_guide_set *g, issl_guide *out, size_t cap)
{
    if (!g || (!out && g->n_guides)) return issl::fail(ISSL_E_ARG, "null argument");
    if (cap < g->n_guides) {
        issl::set_error("room for " + std::to_string(cap) + " guides, the set has " + std::to_string(g->n_guides));
        return ISSL_E_ARG;
    }
    if (g->n_guides == 0) return ISSL_OK;
    return issl::abi_call([&] { return issl::copy_guides(g, out); });
}

int issl_guides_device(const issl_guide_set *g, const issl_guide **d_guides, const uint64_t **d_sigs)
{
    if (!g || !d_guides || !d_sigs) return issl::fail(ISSL_E_ARG, "null argument");
    *d_guides = static_cast<const issl_guide *>(g->guides.p);
    *d_sigs = static_cast<const uint64_t *>(g->sigs.p);
    return ISSL_OK;
}

int issl_guides_close(issl_guide_set *g)
{
    if (!g) return ISSL_OK;
    if (g->device >= 0) (void)hipSetDevice(g->device);
    delete g;
    return ISSL_OK;
}

} // extern "C"
