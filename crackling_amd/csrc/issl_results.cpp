// The result table, host side (issl_results_*, include/issl_hip.h): the argument checks, the text pool the kernels of
// issl_results.hip copy their free-text fields from (issl_results_text.hpp), the launches and the way out to host memory
// and to a file.  The host waits once while a table is built, for the text's length.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_folds.hpp"
#include "issl_folds_text.hpp"
#include "issl_genome_handle.hpp"
#include "issl_guides.hpp"
#include "issl_host.hpp"
#include "issl_results.hpp"
#include "issl_results_text.hpp"

struct issl_results {
    int device = -1;
    uint64_t n_rows = 0, n_bytes = 0;
    issl::DevBuf text, offsets; // n_bytes characters (padded to 16), n_rows + 1 offsets
    float ms_measure = 0, ms_scan = 0, ms_emit = 0; // the three launches by HIP events on their stream
};

namespace issl {
namespace {

struct Inputs {
    const issl_guide_set *gs;
    const issl_consensus_row *d_rows;
    const uint32_t *d_fold, *d_selected;
    uint64_t n_fold, n_selected;
    const char *ss_text;
    size_t ss_len;
    const issl_text_span *ss_spans;
    const issl_folds *folds;      // in place of the three above: the spans and their text where issl_folds_read left them
    const issl_occurrence *d_bowtie;
    const issl_genome *genome;
    const uint32_t *d_scored;
    const double *d_mit, *d_cfd;
    size_t n_scored;
    const issl_results_config *cfg;
    uint64_t first_row, n_rows; // the rows of the set the text holds
};

} // namespace

// The method as the scorer matches it (exactly) and as the caller reads it (stripped, lower case): issl_verdicts.
void method_rules(const char *method, ResultArgs &a)
{
    const int printed = method_from_string(method);
    a.print_mit = printed == ISSL_METHOD_MIT || printed == ISSL_METHOD_AND || printed == ISSL_METHOD_OR || printed == ISSL_METHOD_AVG;
    a.print_cfd = printed == ISSL_METHOD_CFD || printed == ISSL_METHOD_AND || printed == ISSL_METHOD_OR || printed == ISSL_METHOD_AVG;
    std::string m(method);
    const char *ws = " \t\n\r\f\v";
    const size_t b = m.find_first_not_of(ws);
    m = b == std::string::npos ? std::string() : m.substr(b, m.find_last_not_of(ws) - b + 1);
    for (char &c : m) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
    switch (method_from_string(m.c_str())) {
    case ISSL_METHOD_MIT: a.rule = kRuleMit; break;
    case ISSL_METHOD_CFD: a.rule = kRuleCfd; break;
    case ISSL_METHOD_AND: a.rule = kRuleAnd; break;
    case ISSL_METHOD_OR: a.rule = kRuleOr; break;
    case ISSL_METHOD_AVG: a.rule = kRuleAvg; break;
    default: a.rule = kRuleNone; break;
    }
}

namespace {

// Host text -> pool and span tables.  No device call.
int prepare_text(const Inputs &in, ResultPool &pool, std::vector<issl_text_span> &headers, std::vector<issl_text_span> &ss,
                 std::vector<issl_text_span> &chr)
{
    const char d = in.cfg->delimiter;
    pool.fixed_len = in.ss_spans ? in.ss_len : 0;
    if (in.ss_spans) {
        size_t bad = 0;
        if (!results_ss_spans(in.ss_text, in.ss_len, in.ss_spans, 3 * in.n_fold, d, pool, ss, &bad)) {
            set_error("span " + std::to_string(bad % 3) + " of fold " + std::to_string(bad / 3) + " does not lie in the " +
                      std::to_string(in.ss_len) + " bytes of text");
            return ISSL_E_ARG;
        }
    }
    headers.resize(in.gs->records.size());
    for (size_t r = 0; r < headers.size(); ++r) {
        const std::string &name = in.gs->records[r].name;
        if (!pool.add(name.data(), name.size(), d, headers[r])) {
            set_error("the header of record " + std::to_string(r) + " is longer than a field can be");
            return ISSL_E_UNSUPPORTED;
        }
    }
    if (in.d_bowtie) {
        chr.resize(in.genome->records.size());
        for (size_t r = 0; r < chr.size(); ++r) {
            const std::string &name = in.genome->records[r].name;
            size_t begin, n;
            first_word(name.data(), name.size(), begin, n);
            if (!pool.add(name.data() + begin, n, d, chr[r])) {
                set_error("the name of genome record " + std::to_string(r) + " is longer than a field can be");
                return ISSL_E_UNSUPPORTED;
            }
        }
    }
    return ISSL_OK;
}

template <class T> int upload(DevBuf &buf, const std::vector<T> &v, hipStream_t stream)
{
    if (v.empty()) return ISSL_OK;
    HIP_TRY(hipMalloc(&buf.p, sizeof(T) * v.size()));
    HIP_TRY(hipMemcpyAsync(buf.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, stream));
    return ISSL_OK;
}

int invert(DevBuf &buf, const uint32_t *d_list, uint64_t n_list, uint32_t n, hipStream_t stream)
{
    HIP_TRY(hipMalloc(&buf.p, 4ull * n));
    HIP_TRY(hipMemsetAsync(buf.p, 0xFF, 4ull * n, stream));
    launch_results_invert(d_list, static_cast<uint32_t>(n_list), static_cast<uint32_t *>(buf.p), n, stream);
    HIP_TRY(hipGetLastError());
    return ISSL_OK;
}

int results_build(const Inputs &in, issl_results **out)
{
    ResultPool pool;
    std::vector<issl_text_span> headers, ss, chr;
    if (int rc = prepare_text(in, pool, headers, ss, chr)) return rc;
    const std::string header_row = (in.cfg->flags & ISSL_RESULTS_NO_HEADER) ? std::string() : results_header_row(in.cfg->delimiter);

    if (int rc = select_device(in.gs->device, "the extraction")) return rc;
    std::unique_ptr<issl_results> r(new issl_results());
    r->device = in.gs->device;
    r->n_rows = in.n_rows;
    const uint32_t n_set = static_cast<uint32_t>(in.gs->n_guides); // (a set has at most 2^32 - 1 matches)
    const uint32_t n = static_cast<uint32_t>(in.n_rows);           // the rows of the text: [first_row, first_row + n) of the set
    hipStream_t stream = nullptr; // the null stream: behind whatever the caller's streams have enqueued for the inputs
    HIP_TRY(hipMalloc(&r->offsets.p, 8ull * (n + 1ull)));
    if (n == 0) {
        r->n_bytes = header_row.size();
        const uint64_t first = header_row.size();
        HIP_TRY(hipMalloc(&r->text.p, ((r->n_bytes + 15) & ~15ull) + 16));
        if (!header_row.empty()) HIP_TRY(hipMemcpy(r->text.p, header_row.data(), header_row.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(r->offsets.p, &first, 8, hipMemcpyHostToDevice));
        *out = r.release();
        return ISSL_OK;
    }

    DevBuf d_pool, d_headers, d_ss, d_chr, fold_of, sel_of, score_of, sums;
    const uint64_t pool_bytes = pool.fixed_len + pool.extra.size();
    if (pool_bytes) {
        HIP_TRY(hipMalloc(&d_pool.p, pool_bytes));
        if (pool.fixed_len)
            HIP_TRY(hipMemcpyAsync(d_pool.p, in.ss_text, pool.fixed_len, hipMemcpyHostToDevice, stream));
        if (!pool.extra.empty())
            HIP_TRY(hipMemcpyAsync(static_cast<char *>(d_pool.p) + pool.fixed_len, pool.extra.data(), pool.extra.size(),
                                      hipMemcpyHostToDevice, stream));
    }
    if (int rc = upload(d_headers, headers, stream)) return rc;
    if (int rc = upload(d_ss, ss, stream)) return rc;
    if (int rc = upload(d_chr, chr, stream)) return rc;

    ResultArgs a{};
    a.guides = static_cast<const issl_guide *>(in.gs->guides.p);
    a.rows = in.d_rows;
    a.first = static_cast<uint32_t>(in.first_row);
    a.n = n;
    a.headers = static_cast<const issl_text_span *>(d_headers.p);
    a.n_headers = static_cast<uint32_t>(headers.size());
    if ((in.ss_spans || in.folds) && in.n_fold) {
        if (int rc = invert(fold_of, in.d_fold, in.n_fold, n_set, stream)) return rc;
        a.fold_of = static_cast<const uint32_t *>(fold_of.p);
        a.ss = in.folds ? static_cast<const issl_text_span *>(in.folds->spans.p) : static_cast<const issl_text_span *>(d_ss.p);
        a.fold_text = in.folds ? static_cast<const char *>(in.folds->text.p) : nullptr; // (null before any read: every span is '?')
        a.fold_quote = folds_text::quote_bit(static_cast<uint8_t>(in.cfg->delimiter)) | folds_text::quote_bit('"');
        a.n_fold = static_cast<uint32_t>(in.n_fold);
    }
    if (in.d_bowtie && in.n_selected) {
        if (int rc = invert(sel_of, in.d_selected, in.n_selected, n_set, stream)) return rc;
        a.sel_of = static_cast<const uint32_t *>(sel_of.p);
        a.occ = in.d_bowtie;
        a.n_sel = static_cast<uint32_t>(in.n_selected);
        a.chr = static_cast<const issl_text_span *>(d_chr.p);
        a.n_chr = static_cast<uint32_t>(chr.size());
    }
    if (in.d_scored && in.n_scored) {
        if (int rc = invert(score_of, in.d_scored, in.n_scored, n_set, stream)) return rc;
        a.score_of = static_cast<const uint32_t *>(score_of.p);
        a.mit = in.d_mit;
        a.cfd = in.d_cfd;
        a.n_scored = static_cast<uint32_t>(in.n_scored);
    }
    a.pool = static_cast<const char *>(d_pool.p);
    a.threshold = in.cfg->threshold;
    method_rules(in.cfg->method, a);
    a.no_sgrna = (in.cfg->flags & ISSL_RESULTS_NO_SGRNA) ? 1u : 0u;
    a.delimiter = in.cfg->delimiter;

    const uint32_t groups = result_groups(n);
    uint64_t *offsets = static_cast<uint64_t *>(r->offsets.p);
    HIP_TRY(hipMalloc(&sums.p, 8ull * (groups + 1ull)));
    Events<5> ev;
    if (int rc = ev.create()) return rc;
    HIP_TRY(hipEventRecord(ev.e[0], stream));
    launch_results_measure(a, offsets, static_cast<uint64_t *>(sums.p), stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], stream));
    launch_results_scan(static_cast<uint64_t *>(sums.p), groups, header_row.size(), offsets, n, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[2], stream));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, static_cast<uint64_t *>(sums.p) + groups, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total < header_row.size() + 49ull * n) { // (a row is at least the 23-mer, 25 delimiters and the line end)
        set_error("the rows measure " + std::to_string(total) + " bytes for " + std::to_string(n) + " guides");
        return ISSL_E_DEVICE;
    }
    r->n_bytes = total;
    HIP_TRY(hipMalloc(&r->text.p, (total + 15) & ~15ull));
    if (!header_row.empty())
        HIP_TRY(hipMemcpyAsync(r->text.p, header_row.data(), header_row.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ev.e[3], stream));
    launch_results_emit(a, offsets, static_cast<const uint64_t *>(sums.p), static_cast<char *>(r->text.p),
                        (in.cfg->flags & ISSL_RESULTS_DIRECT) != 0, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[4], stream));
    HIP_TRY(hipStreamSynchronize(stream)); // (the tables above go with this scope)
    HIP_TRY(hipEventElapsedTime(&r->ms_measure, ev.e[0], ev.e[1]));
    HIP_TRY(hipEventElapsedTime(&r->ms_scan, ev.e[1], ev.e[2]));
    HIP_TRY(hipEventElapsedTime(&r->ms_emit, ev.e[3], ev.e[4]));
    *out = r.release();
    return ISSL_OK;
}

int results_copy(const issl_results *r, char *out)
{
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpy(out, r->text.p, r->n_bytes, hipMemcpyDeviceToHost));
    return ISSL_OK;
}

int results_write(const issl_results *r, const char *path, int append)
{
    std::unique_ptr<char[]> host(new char[r->n_bytes ? r->n_bytes : 1]);
    if (int rc = results_copy(r, host.get())) return rc;
    FILE *fp = std::fopen(path, append ? "ab" : "wb");
    if (!fp) {
        set_error(std::string("cannot open ") + path + ": " + std::strerror(errno));
        return ISSL_E_IO;
    }
    const size_t wrote = std::fwrite(host.get(), 1, r->n_bytes, fp);
    const int closed = std::fclose(fp);
    if (wrote != r->n_bytes || closed != 0) {
        set_error(std::string("cannot write ") + path + ": " + std::strerror(errno));
        return ISSL_E_IO;
    }
    return ISSL_OK;
}

} // namespace
} // namespace issl

extern "C" {

static int build_range(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                                    const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                                    const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                                    size_t n_scored, const uint64_t *range, const issl_results_config *cfg, issl_results **out,
                                    const issl_folds *folds = nullptr);

int issl_results_build(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                       const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                       const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                       size_t n_scored, const issl_results_config *cfg, issl_results **out)
{
    return build_range(gs, c, ss_text, ss_len, ss_spans, n_folds, d_bowtie, n_bowtie, genome, d_scored, d_mit, d_cfd,
                                    n_scored, nullptr, cfg, out);
}

int issl_results_build_rows(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                            const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                            const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                            size_t n_scored, uint64_t first_row, uint64_t n_rows, const issl_results_config *cfg,
                            issl_results **out)
{
    const uint64_t range[2] = {first_row, n_rows};
    return build_range(gs, c, ss_text, ss_len, ss_spans, n_folds, d_bowtie, n_bowtie, genome, d_scored, d_mit, d_cfd,
                                    n_scored, range, cfg, out);
}

int issl_results_build_rows_folds(const issl_guide_set *gs, const issl_consensus *c, const issl_folds *f,
                                  const issl_occurrence *d_bowtie, size_t n_bowtie, const issl_genome *genome,
                                  const uint32_t *d_scored, const double *d_mit, const double *d_cfd, size_t n_scored,
                                  uint64_t first_row, uint64_t n_rows, const issl_results_config *cfg, issl_results **out)
{
    if (out) *out = nullptr;
    if (!f) return issl::fail(ISSL_E_ARG, "null argument");
    const uint64_t range[2] = {first_row, n_rows};
    return build_range(gs, c, nullptr, 0, nullptr, 0, d_bowtie, n_bowtie, genome, d_scored, d_mit, d_cfd, n_scored, range, cfg, out, f);
}

/* range: {first row, rows}, or NULL for the whole set.  The checks in the order of the header's list, every one of them
   ahead of any device call. */
static int build_range(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                                    const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                                    const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                                    size_t n_scored, const uint64_t *range, const issl_results_config *cfg, issl_results **out,
                                    const issl_folds *folds)
{
    if (out) *out = nullptr;
    if (!gs || !c || !cfg || !out || !cfg->method) return issl::fail(ISSL_E_ARG, "null argument");
    if (!issl::results_delimiter_ok(cfg->delimiter))
        return issl::fail(ISSL_E_UNSUPPORTED, "delimiter: one of ',', TAB, ';', '|' and ' '");
    issl::Inputs in{};
    in.gs = gs;
    in.cfg = cfg;
    in.first_row = range ? range[0] : 0;
    in.n_rows = range ? range[1] : gs->n_guides;
    if (in.first_row > gs->n_guides || in.n_rows > gs->n_guides - in.first_row) {
        issl::set_error("rows " + std::to_string(in.first_row) + " and the " + std::to_string(in.n_rows) + " behind it of a set of " +
                        std::to_string(gs->n_guides) + " guides");
        return ISSL_E_ARG;
    }
    if (int rc = issl_consensus_device(c, &in.d_rows, &in.d_selected, &in.n_selected)) return rc; // (ISSL_E_STATE: not finished)
    if (int rc = issl_consensus_fold_list(c, &in.d_fold, &in.n_fold)) return rc;
    if (folds) {
        if (folds->consensus != c) return issl::fail(ISSL_E_ARG, "the folds belong to another consensus");
        in.folds = folds;
    }
    if (ss_spans) {
        if (!ss_text && ss_len) return issl::fail(ISSL_E_ARG, "null argument");
        if (n_folds != in.n_fold) {
            issl::set_error("spans for " + std::to_string(n_folds) + " folds, the fold list has " + std::to_string(in.n_fold));
            return ISSL_E_ARG;
        }
        in.ss_text = ss_text ? ss_text : "";
        in.ss_len = ss_len;
        in.ss_spans = ss_spans;
    }
    if (d_bowtie) {
        if (!genome) return issl::fail(ISSL_E_ARG, "Bowtie rows without the genome that names their records");
        if (genome->device != gs->device) return issl::fail(ISSL_E_ARG, "the genome is on another device than the guide set");
        if (n_bowtie != in.n_selected) {
            issl::set_error(std::to_string(n_bowtie) + " Bowtie rows, the selection has " + std::to_string(in.n_selected));
            return ISSL_E_ARG;
        }
        in.d_bowtie = d_bowtie;
        in.genome = genome;
    }
    if (d_scored) {
        if (!d_mit || !d_cfd) return issl::fail(ISSL_E_ARG, "scored rows without both scores");
        if (n_scored > gs->n_guides) {
            issl::set_error(std::to_string(n_scored) + " scored rows, the set has " + std::to_string(gs->n_guides) + " guides");
            return ISSL_E_ARG;
        }
        in.d_scored = d_scored;
        in.d_mit = d_mit;
        in.d_cfd = d_cfd;
        in.n_scored = n_scored;
    }
    return issl::abi_call([&] { return issl::results_build(in, out); });
}

int issl_results_info(const issl_results *r, uint64_t *n_rows, uint64_t *n_bytes, uint32_t *rows_per_group)
{
    if (!r) return issl::fail(ISSL_E_ARG, "null argument");
    if (n_rows) *n_rows = r->n_rows;
    if (n_bytes) *n_bytes = r->n_bytes;
    if (rows_per_group) *rows_per_group = issl::kResultRows;
    return ISSL_OK;
}

int issl_results_times(const issl_results *r, double *ms_measure, double *ms_scan, double *ms_emit)
{
    if (!r) return issl::fail(ISSL_E_ARG, "null argument");
    if (ms_measure) *ms_measure = r->ms_measure;
    if (ms_scan) *ms_scan = r->ms_scan;
    if (ms_emit) *ms_emit = r->ms_emit;
    return ISSL_OK;
}

int issl_results_device(const issl_results *r, const char **d_text, const uint64_t **d_offsets)
{
    if (!r || !d_text || !d_offsets) return issl::fail(ISSL_E_ARG, "null argument");
    *d_text = static_cast<const char *>(r->text.p);
    *d_offsets = static_cast<const uint64_t *>(r->offsets.p);
    return ISSL_OK;
}

int issl_results_copy(const issl_results *r, char *out, size_t cap)
{
    if (!r || !out) return issl::fail(ISSL_E_ARG, "null argument");
    if (cap < r->n_bytes) {
        issl::set_error("room for " + std::to_string(cap) + " bytes, the text has " + std::to_string(r->n_bytes));
        return ISSL_E_ARG;
    }
    return issl::abi_call([&] { return issl::results_copy(r, out); });
}

int issl_results_write(const issl_results *r, const char *path, int append)
{
    if (!r || !path) return issl::fail(ISSL_E_ARG, "null argument");
    return issl::abi_call([&] { return issl::results_write(r, path, append); });
}

int issl_results_close(issl_results *r)
{
    if (!r) return ISSL_OK;
    if (r->device >= 0) (void)hipSetDevice(r->device);
    delete r;
    return ISSL_OK;
}

int issl_repr_f64_device(const double *d_values, size_t n, char *d_text, uint32_t *d_len, void *stream)
{
    if (n && (!d_values || !d_text || !d_len)) return issl::fail(ISSL_E_ARG, "null argument");
    if (n > (size_t(1) << 39)) return issl::fail(ISSL_E_ARG, "at most 2^39 values per call"); // (2^31 - 1 workgroups of 256)
    if (n == 0) return ISSL_OK;
    return issl::abi_call([&]() -> int {
        int count = 0;
        if (int rc = issl::count_devices("the formatter", &count)) return rc;
        issl::launch_repr(d_values, n, d_text, d_len, stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            issl::set_error(std::string("HIP error: ") + hipGetErrorString(e) + " at the launch of the formatter");
            return ISSL_E_DEVICE;
        }
        return ISSL_OK;
    });
}

} // extern "C"
