// Off-target site extraction on the GPU: the step that feeds the index builder.
// Counterpart of /root/reference/src/crackling/utils/extractOfftargets.py:
//   :23-24   forward pattern [ACG][ACGT]{19}[ACGT][AG]G, reverse pattern C[CT][ACGT][ACGT]{19}[TGC], both as lookaheads
//            (every position is tried, matches overlap)
//   :97-110  a match contributes the first 20 characters of its 23 -- as they are (forward) or reverse-complemented
//            (reverse pattern; Helpers.py:7-10)
//   :112-191 all sites, one per line, sorted as text, duplicates kept
//
// Host: FASTA records -> one upper-cased byte string with '\n' between records (no match can span a separator).
// Device: k_match_count / k_match_emit find the matches and write each site as a 40-bit key whose numeric order is
// the text order (base 0 in the two most significant bits); an LSD radix sort (5 passes of 8 bits) orders the keys;
// k_keys_to_text expands them to "<20 chars>\n".
//
// Genome -> index (issl_index_build_from_fasta): the sorted keys never leave the device.  k_run_heads counts the heads of
// the runs of equal keys per 4096-key block, launch_scan turns the counts into the rank of every block's first head, and
// k_run_sites writes, per run, the site's ISSL signature (isslCreateIndex.cpp:39-47,183-200: the 20 two-bit groups of the
// key in reverse order, base 0 in the least significant bits) and its occurrence count.  Those two arrays go to the
// device-side builder (issl_index_build_from_device_sites) as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "issl_host.hpp"
#include "issl_index.hpp"
#include "issl_match.hpp"
#include "issl_radix.hpp"

namespace issl {

namespace {

__global__ __launch_bounds__(256) void k_match_count(const uint8_t *__restrict__ s, uint64_t len,
                                                     unsigned long long *__restrict__ total)
{
    __shared__ uint32_t wave_cnt[4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    uint32_t cnt = 0;
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a, b;
        const uint32_t m = match_at(s, base + k, len, a, b);
        cnt += (m & 1u) + (m >> 1);
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (t) atomicAdd(total, static_cast<unsigned long long>(t));
    }
}

// Second pass: every workgroup reserves room for its matches with ONE atomic, then its threads write keys at
// wave-prefix offsets (the order of the keys is irrelevant, they are sorted afterwards).
__global__ __launch_bounds__(256) void k_match_emit(const uint8_t *__restrict__ s, uint64_t len,
                                                    unsigned long long *__restrict__ cursor, uint64_t *__restrict__ keys,
                                                    uint64_t cap)
{
    __shared__ uint32_t wave_cnt[4];
    __shared__ unsigned long long block_base;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kPosPerBlock;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt = 0;
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a, b;
        const uint32_t m = match_at(s, base + k, len, a, b);
        cnt += (m & 1u) + (m >> 1);
    }
    uint32_t incl = cnt; // inclusive scan inside the wave
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        block_base = t ? atomicAdd(cursor, static_cast<unsigned long long>(t)) : 0ull;
    }
    __syncthreads();
    uint64_t at = block_base + (incl - cnt);
    for (uint32_t w = 0; w < wave; ++w) at += wave_cnt[w];
    for (uint32_t k = threadIdx.x; k < kPosPerBlock; k += 256) {
        uint64_t a = 0, b = 0;
        const uint32_t m = match_at(s, base + k, len, a, b);
        if ((m & 1u) && at < cap) keys[at++] = a;
        if ((m & 2u) && at < cap) keys[at++] = b;
    }
}

__global__ __launch_bounds__(256) void k_keys_to_text(const uint64_t *__restrict__ keys, uint64_t n, char *__restrict__ text)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    char *dst = text + i * 21;
#pragma unroll
    for (int p = 0; p < 20; ++p) dst[p] = "ACGT"[(key >> (2 * (19 - p))) & 3u];
    dst[20] = '\n';
}

// ---- collapse of the sorted keys into the site table (runs of equal keys -> one site each) -------------------------
// No thread walks a run: a repeat gives 10^5 identical keys and more.  Every key is looked at by one thread, which
// compares it with its two neighbours; a run's count is its tail's index + 1 minus its head's index.
constexpr uint32_t kRunRounds = 16;                 // keys per thread in the collapse kernels
constexpr uint32_t kRunBlockKeys = 256 * kRunRounds; // keys per 256-thread workgroup

__global__ __launch_bounds__(256) void k_run_heads(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_cnt[4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kRunBlockKeys;
    uint32_t c = 0;
    for (uint32_t r = 0; r < kRunRounds; ++r) {
        const uint64_t i = base + r * 256 + threadIdx.x;
        if (i < n && (i == 0 || keys[i] != keys[i - 1])) ++c;
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// first[b]: heads before block b (exclusive scan of k_run_heads' counts).  occ[] is zeroed before the launch: the head
// and the tail of a run of two keys or more add -head and tail + 1 to the run's count, in whichever order they come.
__global__ __launch_bounds__(256) void k_run_sites(const uint64_t *__restrict__ keys, uint64_t n, const uint32_t *__restrict__ first,
                                                   uint64_t *__restrict__ sigs, uint32_t *__restrict__ occ)
{
    __shared__ uint32_t wave_cnt[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kRunBlockKeys;
    uint32_t before = first[blockIdx.x]; // heads ahead of this round
    for (uint32_t r = 0; r < kRunRounds; ++r) {
        const uint64_t i = base + r * 256 + threadIdx.x;
        const bool valid = i < n;
        const uint64_t key = valid ? keys[i] : 0ull;
        const bool head = valid && (i == 0 || keys[i - 1] != key);
        const bool tail = valid && (i + 1 == n || keys[i + 1] != key);
        const uint64_t heads = __ballot(head);
        if (lane == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(heads));
        __syncthreads();
        uint32_t rank = before + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(heads >> 32),
                                                           __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(heads), 0u));
        for (uint32_t w = 0; w < wave; ++w) rank += wave_cnt[w];
        // rank: heads before i, i.e. the id of the site i opens, or one past the id of the site i belongs to
        if (head) {
            uint64_t sig = 0;
#pragma unroll
            for (int p = 0; p < 20; ++p) sig |= ((key >> (2 * (19 - p))) & 3ull) << (2 * p);
            sigs[rank] = sig;
        }
        const uint32_t at = static_cast<uint32_t>(i); // n <= 2^32 - 1: exact, and the sums below are exact mod 2^32
        if (head && tail) occ[rank] = 1u;
        else if (head) atomicAdd(&occ[rank], 0u - at);
        else if (tail) atomicAdd(&occ[rank - 1], at + 1u);
        before += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
}

// FASTA bytes -> upper-cased sequence text with '\n' after every record.  The reference (extractOfftargets.py) reads
// its inputs in Python's text mode -- "\n", "\r\n" and a lone "\r" each end a line -- and has two sets of rules:
//   one input (:209-222, explodeMultiFastaFile :26-62): every line is stripped; a stripped line that starts with '>'
//     opens a record;
//   several inputs (processingNode :74-90 on each file as it is): a line is a header when its first raw character is
//     '>'; other lines lose their trailing blanks only, so leading blanks are sequence text; the records of one file are
//     keyed by the header line, and a repeated header empties the record before it (:83-85).
// Where the reference raises on one input -- a blank line (IndexError, :36), sequence before the first header
// (AttributeError, :56) -- the blank line is skipped and the sequence is a record of its own.

// What str.strip() removes from ASCII text: C's isspace() and the separators FS GS RS US.
static inline bool py_blank(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

// A header line: its text behind '>' in the file, whether the line has a line end (text mode makes every line end
// "\n"; the last line of a file may have none, and is then another key of the per-file rules), and where its record's
// sequence starts in the piece's text.
struct HeaderMark {
    size_t hdr, hdr_len;
    bool ended;
    size_t at;
};

struct Piece {
    std::string text;              // explode rules: records closed by '\n'; per-file rules: no separators, see marks
    std::vector<HeaderMark> marks; // the join of the per-file rules needs them, the record table of either rules
};

// Lines [begin, end) of one piece of a file; `begin` is a line start, `end` the end of the file or behind a '\n'.
static void parse_fasta_lines(const char *fasta, size_t begin, size_t end, bool per_file, Piece &out)
{
    std::string &seq = out.text;
    size_t p = begin;
    while (p < end) {
        size_t e = p;
        while (e < end && fasta[e] != '\n' && fasta[e] != '\r') ++e;
        size_t next = e < end ? e + 1 : end;
        if (e + 1 < end && fasta[e] == '\r' && fasta[e + 1] == '\n') ++next;
        size_t a = p, b = e;
        if (!per_file)
            while (a < b && py_blank(fasta[a])) ++a;
        while (b > a && py_blank(fasta[b - 1])) --b;
        if (per_file && fasta[p] == '>') {
            out.marks.push_back({p + 1, e - p - 1, e < end, seq.size()});
        } else if (!per_file && b > a && fasta[a] == '>') {
            if (seq.empty() || seq.back() != '\n') seq.push_back('\n'); // (a piece's leading separator is settled when it is joined)
            out.marks.push_back({a + 1, e - a - 1, e < end, seq.size()});
        } else {
            for (size_t k = a; k < b; ++k) seq.push_back(static_cast<char>(std::toupper(static_cast<unsigned char>(fasta[k]))));
        }
        p = next;
    }
}

// Per-file rules: the pieces' records in file order, those dropped whose header line comes again later in the file (in
// whichever piece), the others appended to seq with a '\n' behind each.  A piece's text ahead of its first header
// continues the record open at the end of the piece before it.  records: every record that is not dropped gets an entry
// when its first span comes by -- a header without sequence too, the lines ahead of the first header only when they
// hold text.
static void join_file_records(const char *fasta, const std::vector<Piece> &piece, std::string &seq, std::vector<FastaRecord> *records)
{
    struct Span { uint32_t rec; const std::string *text; size_t from, to; };
    struct Key { std::string_view hdr; bool ended; };
    std::vector<Span> spans;
    std::vector<Key> keys(1);  // record 0: the lines before the first header (keyed by the path in the reference)
    for (const auto &pc : piece) {
        size_t from = 0;
        for (const auto &m : pc.marks) {
            spans.push_back({static_cast<uint32_t>(keys.size() - 1), &pc.text, from, m.at});
            keys.push_back({std::string_view(fasta + m.hdr, m.hdr_len), m.ended});
            from = m.at;
        }
        spans.push_back({static_cast<uint32_t>(keys.size() - 1), &pc.text, from, pc.text.size()});
    }
    std::unordered_map<std::string_view, std::array<uint32_t, 2>> last; // header text -> last record, by `ended`
    for (uint32_t r = 1; r < keys.size(); ++r) last[keys[r].hdr][keys[r].ended] = r;
    uint32_t open = 0;
    bool listed = false; // the record of the span before this one has its entry
    uint32_t listed_rec = 0;
    for (const auto &sp : spans) {
        const bool dropped = sp.rec && last[keys[sp.rec].hdr][keys[sp.rec].ended] != sp.rec;
        if (records && !dropped && (sp.from != sp.to || sp.rec) && !(listed && listed_rec == sp.rec)) {
            records->push_back({seq.size(), 0, std::string(keys[sp.rec].hdr)});
            listed = true;
            listed_rec = sp.rec;
        }
        if (sp.from == sp.to || dropped) continue;
        if (sp.rec != open && !seq.empty() && seq.back() != '\n') seq.push_back('\n');
        open = sp.rec;
        if (records && records->back().length == 0) records->back().start = seq.size(); // behind its separator
        seq.append(*sp.text, sp.from, sp.to - sp.from);
        if (records) records->back().length += sp.to - sp.from;
    }
}

// The one host pass of the extraction, on up to 16 threads: the file is cut at line starts, every piece is parsed on
// its own, and the pieces are joined with the sequential rule for record separators (none at the very start, never two
// in a row), so the result is byte-for-byte what one thread produces.  per_file: the rules for several inputs.  (One
// thread manages ~0.3 GB/s: 10 s for a human genome, against ~0.3 s for everything that follows on the GPU.)
// records: the table of the records appended, by the same sequential rules (a header's record starts where the text
// stands once its separator is settled; under the explode rules a record ends one short of the next one's start).
} // namespace

void append_records(const char *fasta, size_t len, bool per_file, std::string &seq, std::vector<FastaRecord> *records)
{
    const size_t want = std::min<size_t>({16, std::max(1u, std::thread::hardware_concurrency()), len / (size_t(4) << 20) + 1});
    std::vector<size_t> cut(want + 1, len);
    cut[0] = 0;
    for (size_t t = 1; t < want; ++t) {
        size_t at = std::max(cut[t - 1], len / want * t);
        while (at < len && fasta[at] != '\n') ++at;  // the piece starts behind the next line end
        cut[t] = at < len ? at + 1 : len;
    }
    std::vector<Piece> piece(want);
    {
        issl::ThreadGroup pool;
        for (size_t t = 1; t < want; ++t)
            pool.add([&, t] { piece[t].text.reserve(cut[t + 1] - cut[t]); parse_fasta_lines(fasta, cut[t], cut[t + 1], per_file, piece[t]); });
        piece[0].text.reserve(cut[1] - cut[0]);
        parse_fasta_lines(fasta, cut[0], cut[1], per_file, piece[0]);
        pool.join();
    }
    size_t total = seq.size() + 1;
    for (const auto &pc : piece) total += pc.text.size() + (per_file ? pc.marks.size() : 0);
    seq.reserve(total);
    const size_t seq0 = seq.size(), rec0 = records ? records->size() : 0;
    if (per_file) {
        join_file_records(fasta, piece, seq, records);
    } else {
        for (const auto &pc : piece) {
            size_t from = 0;
            if (!pc.text.empty() && pc.text[0] == '\n' && (seq.empty() || seq.back() == '\n')) from = 1;
            if (records)
                for (const auto &m : pc.marks) records->push_back({seq.size() + m.at - from, 0, std::string(fasta + m.hdr, m.hdr_len)});
            seq.append(pc.text, from, std::string::npos);
        }
    }
    if (!seq.empty() && seq.back() != '\n') seq.push_back('\n');
    if (records && !per_file) {
        const uint64_t first = records->size() > rec0 ? (*records)[rec0].start : seq.size();
        if (first > seq0) records->insert(records->begin() + rec0, FastaRecord{seq0, 0, std::string()}); // text ahead of the first header
        for (size_t r = rec0; r < records->size(); ++r) {
            const uint64_t next = r + 1 < records->size() ? (*records)[r + 1].start : seq.size();
            (*records)[r].length = next > (*records)[r].start ? next - (*records)[r].start - 1 : 0;
        }
    }
}

namespace {

// seq (host) -> sorted site keys in the memory of the current device: keys.p holds *n_sites of them (null when there
// are none).  Peak: the sequence, then 16 B per site (keys + sort scratch).
int extract_sorted_keys(const std::string &seq, DevBuf &keys, uint64_t *n_sites, StageTimer *clock)
{
    *n_sites = 0;
    const uint64_t len = seq.size();
    if (len < 23) return ISSL_OK;
    DevBuf seq_buf, ctr_buf, tmp_buf;
    HIP_TRY(hipMalloc(&seq_buf.p, len));
    HIP_TRY(hipMalloc(&ctr_buf.p, 16));
    uint8_t *d_seq = static_cast<uint8_t *>(seq_buf.p);
    unsigned long long *d_ctr = static_cast<unsigned long long *>(ctr_buf.p);
    HIP_TRY(hipMemcpy(d_seq, seq.data(), len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_ctr, 0, 16));
    if (clock) clock->note("upload");
    const uint32_t blocks = static_cast<uint32_t>((len + kPosPerBlock - 1) / kPosPerBlock);
    hipLaunchKernelGGL(k_match_count, dim3(blocks), dim3(256), 0, nullptr, d_seq, len, d_ctr);
    unsigned long long total = 0;
    HIP_TRY(hipMemcpy(&total, d_ctr, 8, hipMemcpyDeviceToHost));
    if (total > 0xFFFFFFFFull) { // the radix passes count and place with 32-bit offsets (issl_radix.hpp)
        set_error("more than 2^32 - 1 sites in one extraction (" + std::to_string(total) + "): split the input");
        return ISSL_E_UNSUPPORTED;
    }
    if (total == 0) return ISSL_OK;
    HIP_TRY(hipMalloc(&keys.p, 8 * total));
    HIP_TRY(hipMalloc(&tmp_buf.p, 8 * total));
    uint64_t *d_keys = static_cast<uint64_t *>(keys.p), *d_tmp = static_cast<uint64_t *>(tmp_buf.p);
    hipLaunchKernelGGL(k_match_emit, dim3(blocks), dim3(256), 0, nullptr, d_seq, len, d_ctr + 1, d_keys, total);
    HIP_TRY(hipDeviceSynchronize());
    seq_buf.release();
    if (clock) clock->note("match");
    int rc = radix_sort(d_keys, d_tmp, total, 40);
    tmp_buf.release();
    if (rc) return rc;
    if (clock) clock->note("sort");
    *n_sites = total;
    return ISSL_OK;
}

// seq (host) -> sorted site text (host, malloc'd).
int extract_sorted_text(const std::string &seq, int device, char **out_text, size_t *out_len, uint64_t *n_sites)
{
    if (int rc = select_device(device, "the extraction")) return rc;
    *out_text = nullptr;
    *out_len = 0;
    *n_sites = 0;
    DevBuf keys_buf, text_buf;
    uint64_t total = 0;
    if (int rc = extract_sorted_keys(seq, keys_buf, &total, nullptr)) return rc;
    if (total == 0) {
        *out_text = static_cast<char *>(std::malloc(1));
        return ISSL_OK;
    }
    const uint64_t *d_keys = static_cast<const uint64_t *>(keys_buf.p);
    HIP_TRY(hipMalloc(&text_buf.p, 21 * total));
    char *d_text = static_cast<char *>(text_buf.p);
    hipLaunchKernelGGL(k_keys_to_text, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, nullptr, d_keys,
                       total, d_text);
    char *host = static_cast<char *>(std::malloc(21 * total));
    if (!host) {
        set_error("out of memory");
        return ISSL_E_NOMEM;
    }
    hipError_t e = hipMemcpy(host, d_text, 21 * total, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        std::free(host);
        set_error(std::string("HIP error: ") + hipGetErrorString(e));
        return ISSL_E_DEVICE;
    }
    *out_text = host;
    *out_len = 21 * total;
    *n_sites = total;
    return ISSL_OK;
}

// seq (host) -> uploaded index, the site table built and handed over in HBM.  Same result and same errors as
// extract_sorted_text followed by HostIndex::build_from_text(text, n_sites, 20, slice_width) (the text is sorted, so
// its runs of equal lines are the runs of equal keys), for the widths the device builder takes (checked by the caller).
// Peak of the collapse: 8 B per raw site (keys) + 12 B per distinct site; keys are gone before the image build starts.
int build_index_from_seq(const std::string &seq, size_t slice_width, int device, const char *options, StageTimer &clock,
                         issl_index **out)
{
    if (int rc = select_device(device, "the extraction")) return rc;
    {
        Tuning probe = Tuning::from_env(); // a typo in the options fails here, not after the extraction
        if (int rc = probe.set_list(options)) return rc;
    }
    DevBuf keys_buf, first_buf, sigs_buf, occ_buf;
    uint64_t n = 0;
    if (int rc = extract_sorted_keys(seq, keys_buf, &n, &clock)) return rc;
    if (n == 0) {
        set_error("site list is empty");
        return ISSL_E_ARG;
    }
    const uint64_t *d_keys = static_cast<const uint64_t *>(keys_buf.p);
    const uint32_t n_blocks = static_cast<uint32_t>((n + kRunBlockKeys - 1) / kRunBlockKeys);
    HIP_TRY(hipMalloc(&first_buf.p, 4 * scan_words(n_blocks + 1ull)));
    uint32_t *d_first = static_cast<uint32_t *>(first_buf.p);
    HIP_TRY(hipMemset(d_first + n_blocks, 0, 4));
    hipLaunchKernelGGL(k_run_heads, dim3(n_blocks), dim3(256), 0, nullptr, d_keys, n, d_first);
    launch_scan(d_first, n_blocks + 1ull, nullptr);
    uint32_t n_distinct = 0;
    HIP_TRY(hipMemcpy(&n_distinct, d_first + n_blocks, 4, hipMemcpyDeviceToHost));
    if (n_distinct == 0 || n_distinct > n) {
        set_error("site collapse on the device: " + std::to_string(n_distinct) + " distinct of " + std::to_string(n) + " sites");
        return ISSL_E_DEVICE;
    }
    HIP_TRY(hipMalloc(&sigs_buf.p, 8ull * n_distinct));
    HIP_TRY(hipMalloc(&occ_buf.p, 4ull * n_distinct));
    uint64_t *d_sigs = static_cast<uint64_t *>(sigs_buf.p);
    uint32_t *d_occ = static_cast<uint32_t *>(occ_buf.p);
    HIP_TRY(hipMemset(d_occ, 0, 4ull * n_distinct));
    hipLaunchKernelGGL(k_run_sites, dim3(n_blocks), dim3(256), 0, nullptr, d_keys, n, d_first, d_sigs, d_occ);
    HIP_TRY(hipDeviceSynchronize());
    keys_buf.release();
    first_buf.release();
    clock.note("collapse");
    issl_index *ix = nullptr;
    if (int rc = build_from_device_sites(d_sigs, d_occ, n_distinct, n, 20, slice_width, device, options, &ix)) return rc;
    clock.note("build");
    *out = ix;
    return ISSL_OK;
}

} // namespace

// The FASTA files at paths[0..n) -> seq: the explode rules for one input, the per-file rules for several.
int read_fasta_files(const char *const *paths, int n, std::string &seq, std::vector<FastaRecord> *records)
{
    for (int f = 0; f < n; ++f) {
        std::vector<char> buf; // one file's bytes at a time: released before the next is read
        if (int rc = read_whole_file(paths[f], buf)) return rc;
        append_records(buf.data(), buf.size(), n > 1, seq, records);
    }
    return ISSL_OK;
}

namespace {

bool fasta_index_width(size_t slice_width)
{
    if (slice_width == 8 || slice_width == 4 || slice_width == 2) return true;
    set_error("slice width " + std::to_string(slice_width) + " for an index built from FASTA: 8, 4 or 2 bits (the scorer's geometries)");
    return false;
}

} // namespace

} // namespace issl

extern "C" {

int issl_extract_from_memory(const char *const *files, const size_t *lens, int n_files, int device, char **out_text,
                             size_t *out_len, uint64_t *n_sites)
{
    if (!files || !lens || n_files <= 0 || !out_text || !out_len || !n_sites) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        std::string seq;
        for (int f = 0; f < n_files; ++f) issl::append_records(files[f], lens[f], n_files > 1, seq);
        return issl::extract_sorted_text(seq, device, out_text, out_len, n_sites);
    });
}

int issl_extract_offtargets(const char *const *inputs, int n_inputs, const char *output_path, int device,
                            uint64_t *n_sites)
{
    if (!inputs || n_inputs <= 0 || !output_path || !n_sites) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        std::string seq;
        if (int rc = issl::read_fasta_files(inputs, n_inputs, seq)) return rc;
        char *text = nullptr;
        size_t len = 0;
        int rc = issl::extract_sorted_text(seq, device, &text, &len, n_sites);
        if (rc) return rc;
        FILE *out = std::fopen(output_path, "wb");
        if (!out) {
            std::free(text);
            issl::set_error(std::string("cannot write '") + output_path + "'");
            return ISSL_E_IO;
        }
        const bool ok = (len == 0 || std::fwrite(text, 1, len, out) == len);
        const bool closed = std::fclose(out) == 0;
        std::free(text);
        if (!ok || !closed) {
            issl::set_error(std::string("short write to '") + output_path + "'");
            return ISSL_E_IO;
        }
        return ISSL_OK;
    });
}

int issl_index_build_from_fasta(const char *const *files, const size_t *lens, int n_files, size_t slice_width, int device,
                                const char *options, issl_index **out)
{
    if (!issl::fasta_index_width(slice_width)) return ISSL_E_ARG;
    if (!files || !lens || n_files <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] {
        issl::StageTimer clock(issl::Tuning::from_env().upload_timing, "[issl genome]"); // ISSL_UPLOAD_TIMING=1: one stderr line per stage
        std::string seq;
        for (int f = 0; f < n_files; ++f) issl::append_records(files[f], lens[f], n_files > 1, seq);
        clock.note("parse");
        return issl::build_index_from_seq(seq, slice_width, device, options, clock, out);
    });
}

int issl_index_build_from_fasta_files(const char *const *paths, int n_paths, size_t slice_width, int device,
                                      const char *options, issl_index **out)
{
    if (!issl::fasta_index_width(slice_width)) return ISSL_E_ARG;
    if (!paths || n_paths <= 0 || !out) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&]() -> int {
        issl::StageTimer clock(issl::Tuning::from_env().upload_timing, "[issl genome]"); // ISSL_UPLOAD_TIMING=1: one stderr line per stage
        std::string seq;
        if (int rc = issl::read_fasta_files(paths, n_paths, seq)) return rc;
        clock.note("parse");
        return issl::build_index_from_seq(seq, slice_width, device, options, clock, out);
    });
}

} // extern "C"
