/*
 * issl_hip.h -- C ABI of libissl_hip.so, the MI355X (gfx950) ISSL off-target scorer.
 *
 * Drop-in scope: the `isslScoreOfftargets` step of Crackling (reference paths relative to
 * /root/reference).  The reference has no in-process API for this step -- its boundary is the
 * process `isslScoreOfftargets <issl> <query> <maxDist> <threshold> <method>` launched from
 * src/crackling/Crackling.py:767-778 -- so every entry point below names the block of
 * src/ISSL/isslScoreOfftargets.cpp (or isslCreateIndex.cpp) whose work it takes over.
 * bin/isslScoreOfftargets (crackling_amd/csrc/cli_score.cpp) is the shipped caller.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * ISSL_E_* code, never throws and never calls exit() (memory or a thread that cannot be had is ISSL_E_NOMEM);
 * issl_last_error() holds the message of the last failure on the calling thread.  One issl_index is used by one thread at a time.
 * Scoring needs a HIP device: there is NO CPU fallback, calls fail with ISSL_E_DEVICE.
 */
#ifndef ISSL_HIP_H
#define ISSL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISSL_ABI_VERSION 6

enum {
    ISSL_OK = 0,
    ISSL_E_ARG = -1,      /* bad argument */
    ISSL_E_IO = -2,       /* file cannot be opened / read / written */
    ISSL_E_FORMAT = -3,   /* .issl or query file malformed (reference: "Error reading index", exit 1) */
    ISSL_E_UNSUPPORTED = -4, /* geometry the kernels do not implement */
    ISSL_E_DEVICE = -5,   /* HIP error or no device */
    ISSL_E_NOMEM = -6,
    ISSL_E_STATE = -7,    /* call order (e.g. score before upload) */
    ISSL_E_RETRY = -8     /* issl_score_finish: a batch ran out of scratch space (buffers grown) or needs the whole pipeline: enqueue it again */
};

/* Score methods, isslScoreOfftargets.cpp:44,121-143. */
enum {
    ISSL_METHOD_UNKNOWN = 0, /* neither score computed; the CLI prints -1 -1 */
    ISSL_METHOD_MIT = 1,
    ISSL_METHOD_CFD = 2,
    ISSL_METHOD_AND = 3,
    ISSL_METHOD_OR = 4,
    ISSL_METHOD_AVG = 5
};

typedef struct issl_index issl_index; /* opaque */

/* Header of an .issl file, isslScoreOfftargets.cpp:162-174 / isslCreateIndex.cpp:257-263. */
typedef struct {
    uint64_t n_sites;     /* offtargetsCount: distinct sites */
    uint64_t seq_len;     /* seqLength */
    uint64_t n_lines;     /* seqCount: input lines including duplicates */
    uint64_t slice_width; /* bits per slice */
    uint64_t n_slices;    /* sliceCount */
    uint64_t n_scores;    /* scoresCount: {mask, local MIT score} pairs in the file */
} issl_header;

/* One scored off-target (the reference keeps these only implicitly, :382-463). */
typedef struct {
    uint32_t guide; /* index into the guide batch */
    uint32_t slice; /* slice whose bucket produced it (first matching slice) */
    uint32_t pos;   /* position j inside that bucket, :344 */
    uint32_t id;    /* site id = low 32 bits of the bucket entry, :347 */
    uint32_t dist;  /* mismatches, :380 */
    uint32_t occ;   /* occurrences = high 32 bits of the entry, :348 */
} issl_hit;

/* Timings and counters of the last issl_score* call on an index (milliseconds).  ms_scan is always measured (mean over
 * the batches since the last finish) by the scan kernel itself: first workgroup in to last workgroup out on the 100 MHz
 * constant clock (s_memrealtime), i.e. the launch's own duration; the other stage times (GPU events) and ms_total are filled by the
 * synchronous entry points, and by issl_score_device_async only when the stage_timing option is set (every event
 * record costs ~4 us of stream time, which back-to-back batches should not pay). */
typedef struct {
    uint64_t n_guides;
    uint64_t candidates;    /* (guide, candidate) comparisons the scan kernel COUNTED while making them: real
                               candidates of every tile it fetched x real guides it ran past it.  Full scan: equals
                               reference_comparisons.  Pruned scan: far fewer (only the successor-byte groups of a
                               bucket that can hold a hit are fetched), and >= planned_comparisons because a group's
                               first and last tile also hold neighbours' candidates */
    uint64_t hits;          /* candidates within max_dist, first matching slice only */
    uint64_t scan_tiles;    /* candidate tiles x guide groups processed by the scan kernel */
    double ms_bin;          /* guide binning kernels */
    double ms_scan;         /* XOR/popcount scan kernel (the roofline kernel) */
    double ms_verify;       /* exact re-test of the candidates the scan noted, first-matching-slice rule */
    double ms_group;        /* hit grouping (count/scan/scatter) */
    double ms_replay;       /* ordered MIT/CFD accumulation */
    double ms_total;        /* first kernel to last kernel */
    uint64_t scan_launches; /* >1 when a hit buffer had to grow and the scan was repeated */
    uint64_t raw_records;   /* upper bound of candidates noted by the scan (chunks handed out x chunk size) */
    uint64_t n_batches;     /* batches covered by these statistics (ms_scan is their mean) */
    uint64_t planned_comparisons; /* what the planning kernel expected the scan to compare: guides x lengths of the
                                     buckets (full scan) or successor-byte groups (pruned scan) they visit */
    uint64_t reference_comparisons; /* sum over guides of their five bucket lengths = iterations of the reference's
                                       loop :344 without early exit (host equivalent: issl_count_candidates) */
    uint64_t pruned;              /* 0: full scan; 1 / 2 / 3: pruned scan over the successor-byte groups equal to / within
                                     one / within two mismatches of the guide's own (max_dist <= 2 / <= 4 / = 5, sorted image) */
    double ms_scan_events;        /* the scan launches by the HIP event pair recorded around them on their stream (mean over
                                     the batches that recorded one: scan_events option); equals ms_scan for batches on one
                                     lane, includes the wait for wave slots when a second lane shares the device (lanes) */
} issl_stats;

const char *issl_last_error(void);
int issl_abi_version(void);

/* ---- index: host side (A1, isslScoreOfftargets.cpp:152-270) ------------------------------ */

/* Map and validate an .issl file.  Errors the reference reports (:164-167,201-204,223-226,237-240)
 * and the ones it leaves undefined (missing file, truncated sections, ids out of range). */
int issl_index_open(const char *path, issl_index **out);

/* Same from a memory image of the file (copied). */
int issl_index_from_memory(const void *image, size_t len, issl_index **out);

/* isslCreateIndex.cpp:132-289 counterpart: build an index from the text of a SORTED site list,
 * n_lines lines of seq_len characters + '\n'.  issl_index_write() then emits the same bytes as
 * the reference builder. */
int issl_index_build_from_text(const char *text, size_t n_lines, size_t seq_len,
                               size_t slice_width, issl_index **out);

/* Build from already packed, de-duplicated signatures in id order (isslCreateIndex.cpp:199-200
 * state after the counting loop): sigs[i] occurs occ[i] times; n_lines = sum(occ). */
int issl_index_build_from_sites(const uint64_t *sigs, const uint32_t *occ, size_t n_sites,
                                size_t n_lines, size_t seq_len, size_t slice_width,
                                issl_index **out);

/* Same inputs, but the slice lists (isslCreateIndex.cpp:218-234) are built on `device`: the signatures are
 * copied into the HBM image and one stable radix pass per slice writes the lists next to them.  The result is
 * uploaded and ready to score; the host keeps only the geometry, the MIT table and the bucket sizes (12 B/site of
 * input instead of 48 B/site of host arrays), so indexes up to the format's 2^32-1 sites fit a 288 GB GPU.
 * issl_index_write() streams the arrays back out of the image (same bytes as the host builder);
 * issl_index_upload() to another device is refused -- replicate with issl_index_image/attach_image.
 * 20 bp; slices of 8, 4 or 2 bits (the scorer's geometries). */
int issl_index_build_on_device(const uint64_t *sigs, const uint32_t *occ, size_t n_sites,
                               size_t n_lines, size_t seq_len, size_t slice_width, int device,
                               issl_index **out);
/* The same with layout options for the image it makes, as issl_index_set_option would set them on a handle before
 * issl_index_upload: `options` = "key=value,key=value" (e.g. "compact=1,host_cold=1") or NULL.  (ABI 4) */
int issl_index_build_on_device_opt(const uint64_t *sigs, const uint32_t *occ, size_t n_sites,
                                   size_t n_lines, size_t seq_len, size_t slice_width, int device,
                                   const char *options, issl_index **out);

/* The same for a site table that is ALREADY in the memory of `device` (d_sigs, d_occ: device pointers; e.g. the sorted,
 * de-duplicated sites issl_index_build_from_fasta collapses there, or sites generated on the GPU): bucket lengths are counted on the
 * device, nothing of the size of the index ever exists in host memory.  The inputs are copied into the image and may be
 * freed when the call returns.  isslCreateIndex.cpp:199-234 from its state after the counting loop on.  (ABI 5)
 * Checked on the device: no signature carries bits above 2 * seq_len (ISSL_E_ARG).  NOT checked, as in the host-side
 * builders and in the reference (which collapses only CONSECUTIVE equal lines, isslCreateIndex.cpp:189-193): that the
 * signatures are distinct -- a signature listed twice is two sites, found and scored twice, exactly as the reference scores
 * an index built from unsorted text. */
int issl_index_build_from_device_sites(const uint64_t *d_sigs, const uint32_t *d_occ, size_t n_sites,
                                       size_t n_lines, size_t seq_len, size_t slice_width, int device,
                                       const char *options, issl_index **out);

/* Genome FASTA in, uploaded index out, the site table never in host memory: the extraction below (issl_extract_*) sorts
 * the sites on `device`, the runs of equal sites are collapsed there into signatures and occurrence counts (ids in text
 * order, n_lines = the raw site count), and those go to issl_index_build_from_device_sites with `options`.  The handle and
 * its issl_index_write bytes, scores and errors are those of issl_extract_from_memory(files) followed by
 * issl_index_build_from_text(text, n_lines, 20, slice_width): "site list is empty" (ISSL_E_ARG) for a genome without a
 * site, ISSL_E_UNSUPPORTED above 2^32 - 1 raw sites, ISSL_E_DEVICE without a device (no CPU fallback).  slice_width must be
 * 8, 4 or 2 (ISSL_E_ARG before any work otherwise); an unknown option fails once the device is selected, before the
 * extraction.  Peak HBM: the extraction's 16 B per raw site, then 8 B per raw site + 12 B per distinct site for the
 * collapse, then the image build with its 12 B per distinct site of inputs.  ISSL_UPLOAD_TIMING=1 prints one stderr line
 * per stage.  files[i]/lens[i]: the bytes of FASTA / multi-FASTA files. */
int issl_index_build_from_fasta(const char *const *files, const size_t *lens, int n_files, size_t slice_width,
                                int device, const char *options, issl_index **out);
/* Same from files on disk (what bin/isslIndexFromFasta calls). */
int issl_index_build_from_fasta_files(const char *const *paths, int n_paths, size_t slice_width,
                                      int device, const char *options, issl_index **out);

/* Write the .issl bytes (isslCreateIndex.cpp:256-289). */
int issl_index_write(const issl_index *idx, const char *path);

int issl_index_header(const issl_index *idx, issl_header *out);

/* Bucket lengths, slice-major (isslScoreOfftargets.cpp:221-226): n_slices << slice_width values. */
int issl_index_bucket_sizes(const issl_index *idx, uint64_t *out, size_t n);

int issl_index_close(issl_index *idx);

/* ---- index: HBM image ----------------------------------------------------------------- */

/* Bytes of the device image (sites + bucket entries + packed scan stream + tables). */
int issl_index_device_bytes(const issl_index *idx, size_t *out);

/* Free and total memory of `device` in bytes (hipMemGetInfo): what a resident server weighs an upload against.  (ABI 4) */
int issl_device_memory(int device, size_t *free_bytes, size_t *total_bytes);

/* Allocate the image on `device` (hipMalloc), copy and transform.  Owned by the index. */
int issl_index_upload(issl_index *idx, int device);

/* Same into caller-owned device memory (e.g. a torch uint8 tensor) of at least
 * issl_index_device_bytes() bytes, 256-byte aligned.  The caller keeps it alive until close. */
int issl_index_upload_into(issl_index *idx, int device, void *dev_buf, size_t bytes);

/* Adopt an image that some other rank produced and that arrived in `dev_buf` through an RCCL
 * broadcast: no file is needed on this rank.  Creates a new index handle. */
int issl_index_attach_image(int device, void *dev_buf, size_t bytes, issl_index **out);

/* Device pointer/size of the current image (for the broadcast on the producing rank). */
int issl_index_image(const issl_index *idx, void **dev_ptr, size_t *bytes);

/* Copy the image into caller-owned device memory of the same device (256-byte aligned, >= issl_index_image bytes):
 * how an index that was built on the device gets into the tensor a framework broadcasts. */
int issl_index_copy_image_to(const issl_index *idx, void *dev_dst, size_t bytes);

/* Image layouts, and indexes larger than the free HBM (BASELINE configs[4]; the format's 32-bit ids,
 * isslScoreOfftargets.cpp:347, allow 4.29 G sites).  Only the scan stream (20 B/site) is read by the scan; everything else
 * is touched for the ~2e-5 of the comparisons that come within max_dist.  issl_index_upload / issl_index_build_on_device
 * try, in this order, until one fits the free HBM:
 *   sorted        every bucket ordered by the byte of the next slice (what the pruned scan needs) + 16-byte stream records,
 *                 site table, counts, slice lists: 152 B/site
 *   compact       the same order with 4-byte site ids per stream position: 92 B/site, or 52 B/site WITHOUT the slice lists
 *                 (ABI 5; the automatic fallback): scoring never reads them, and on a sorted layout they are a function of
 *                 site table and counts (every list ascends by site id, isslCreateIndex.cpp:218-234), which
 *                 issl_index_write and issl_dump_hits redo on the device when asked.  An index at the format's limit of
 *                 4.29 G sites takes 223 GB of a 288 GB GPU (3 G lines: 152 GB, measured), nothing in host memory, and
 *                 the image still moves as one broadcast.  While a sorted image is built it needs 8 B per site beyond its
 *                 own size (keys and slice list of the slice being ordered borrow the image's scan section, which is packed
 *                 last): 60 B/site = 258 GB at the format's limit from a file or host arrays (+ a 2 - 9 GB working reserve);
 *                 issl_index_build_from_device_sites has the caller's 12 B/site beside it (~3.8 G sites on 288 GB).  On request (host_cold=1) the lists are kept in pinned,
 *                 mapped HOST memory instead (40 B/site there)
 *   list order    (indexes whose lists do not ascend by site id, or whose five lists disagree about a site's count: no
 *                 builder writes such, the reference does not care; no pruned scan then) with / without in-list
 *                 signatures 108 / 68 B/site, or with site table and lists in host memory 25 B/site (the kernels rebuild
 *                 signatures from the scan stream and read host memory only for counts >= 255 and for issl_dump_hits)
 * Indexes with ten 4-bit or twenty 2-bit slices take every layout but the last (the sorted ones order a bucket by the byte
 * of the next two / four slices; per site the slice lists then cost 80 / 160 B instead of 40).
 * Options sorted_layout / compact / inline_sigs / host_cold force a choice (or the upload fails); results are identical
 * in every layout.  An index with a site in a bucket its signature does not select, or twice in one slice, is refused
 * (ISSL_E_FORMAT).  issl_index_cold() returns the host buffer of an image with host-resident sections (NULL / 0 when
 * everything is in HBM); another device of the same process adopts a copy of the hot image plus the SAME host buffer
 * with issl_index_attach_image_cold (issl_node does this).  Such images cannot be attached in another process. */
int issl_index_cold(const issl_index *idx, void **host_ptr, size_t *bytes);
int issl_index_attach_image_cold(int device, void *dev_buf, size_t bytes, void *cold_host, size_t cold_bytes,
                                 issl_index **out);

/* Tuning knobs.  Every knob has an environment variable that is read ONCE, when the handle is created (open / build /
 * attach), never inside a scoring call; afterwards this call changes it (no batches may be in flight).  Keys (env):
 *   scan_blocks (ISSL_SCAN_BLOCKS) workgroups of the scan launch      item_guides (ISSL_ITEM_GUIDES) guides per scan item
 *   scan_generic (ISSL_SCAN_GENERIC) 0|1 runtime-threshold scan       stage_timing (ISSL_STAGE_TIMING) 0|1 events at every stage
 *   scan_events (ISSL_SCAN_EVENTS) 0|1|2: the HIP event pair around the scan of an asynchronous batch (issl_stats::ms_scan_events):
 *     1 every batch, 2 (default) the first batch after a finish, 0 never -- an event record is ~5 us of stream time, and
 *     ms_scan (the kernel's own clock stamps) times every launch without them
 *   raw_chunks (ISSL_RAW_CHUNKS) initial raw-record buffer
 *   sorted_layout (ISSL_SORTED_LAYOUT), compact (ISSL_COMPACT), inline_sigs (ISSL_INLINE_SIGS), host_cold
 *     (ISSL_FORCE_HOST_COLD), keep_lists (ISSL_KEEP_LISTS), each -1|0|1: image layout, read at upload (see above; -1 =
 *     automatic).  compact=1 with host_cold=1: the compact sorted image with its slice lists in host memory; host_cold=1
 *     alone: the list-order image with site table and lists in host memory; keep_lists=0: the compact sorted image
 *     without slice lists (52 B/site), keep_lists=1: never drop them
 *   tail_shapes (ISSL_TAIL_SHAPES) 0|1 (default 1): the short last unit of a successor-byte group runs 2 / 4 guides per
 *     pass on 16 / 8 candidates per lane
 *   hit_slots (ISSL_HIT_SLOTS) 0|1|2 (default 1): the first 512 hits of every guide go straight from the exact test to a
 *     32-byte record of their own (1.6 GB of scratch per 100 000 guides of a batch; batches beyond 512 k guides, a
 *     device short of memory and issl_dump_hits go without; a handle whose batches show many guides beyond 512 hits
 *     widens its slots to 2048 by itself); 0: every hit passes through the grouping pass; 2: slots for 2048 hits per
 *     guide from the first batch on (tests and A/B: the results do not depend on the width)
 *   lean_tail (ISSL_LEAN_TAIL) 0|1 (default 1): a handle whose finished batches met no guide beyond its hit slots
 *     enqueues the next ones without the grouping pass and the three many-hit replays (five dependent launches that
 *     would find nothing to do: 25 us of every batch); a batch that does meet such a guide is run again in full
 *   small_bin (ISSL_SMALL_BIN) 0|1 (default 1): batches of up to 512 (guide, slice) pairs (102 guides of five slices), max_dist
 *     <= 4, sorted image, are binned in two launches instead of seven -- every placement a group of its own (a matter of
 *     latency only: 64 guides against 300 M sites 0.110 -> 0.079 ms); fine_items (ISSL_FINE_ITEMS): initial capacity of the
 *     pruned plan's item list instead of the size derived from the index (tests of the list's two overflow paths)
 *   expect_guides (ISSL_EXPECT_GUIDES) n: a batch of about n guides follows the upload at once (the one-shot scorer knows its
 *     page): the scoring workspace's streams, events and small buffers are set up on a thread of their own beside the upload --
 *     20 ms less in front of the first kernel; 0 (default): nothing is prepared
 *   upload_chunk_kib, upload_ring_min_kib, upload_threads (ISSL_UPLOAD_CHUNK_KIB, ISSL_UPLOAD_RING_MIN_KIB,
 *     ISSL_UPLOAD_THREADS): the ring of pinned chunks a file-mapped index is uploaded through (eight threads pread the
 *     file into two slots each, every slot leaves with its own asynchronous copy: the PCIe link's rate, where hipMemcpy
 *     from the fresh mapping moves a fifth of it; the sections are queued one behind the other, every reader pins its
 *     slots when it first needs them, and the ring is given back at the end of the upload, before it returns): KiB per
 *     slot (default 16384), the section size from which the ring is used (default 65536), readers (1..32, default 8)
 *   scan_threads (ISSL_SCAN_THREADS) 64..1024: threads per scan workgroup (default 1024 = 8 waves per SIMD; an occupancy
 *     experiment)
 *   prune (ISSL_PRUNE) -1|0|1: scan only the successor-byte groups of a bucket that can hold a site within max_dist (13
 *     of 256 for max_dist <= 4, 1 of 256 for <= 2, 67 of 256 for max_dist 5; same hits and scores as the reference's scan
 *     of the whole bucket, isslScoreOfftargets.cpp:344): -1 = a planning kernel decides per batch from the two plans'
 *     estimated times, 0 = never, 1 = whenever the image is sorted and max_dist <= 5
 *   lanes (ISSL_LANES) 1|2|3: workspaces that the batches of issl_score_device_async alternate between (default 1).  With
 *     2 the batches form a software pipeline: scans one after the other, verify / group / replay of a batch on a
 *     high-priority stream beside the next batch's scan; with 3 only the BINNING of a batch (its short, latency-bound
 *     launches) runs beside the batch before it, the scan waits for that batch's replay.  Outputs of two consecutive
 *     batches must be different buffers with either
 *   scan_stamps (ISSL_SCAN_STAMPS) file for per-wave clocks (diagnostics)
 * Environment only (no key): ISSL_SCAN_VERIFY 0|1 (default: unset): behind the pruned plan on a sorted image a scan wave applies
 *   the exact test to the chunks of records it has filled itself, between two of its units, while the other waves of its
 *   SIMD go on comparing -- and, once it has filled a chunk, to its last one when its range is done; the verify kernel
 *   takes the rest.  1: every wave's last chunk too (tests: the tail on batches of a few records); 0: every record is the
 *   verify kernel's (A/B).  The results are the same with all three */
int issl_index_set_option(issl_index *idx, const char *key, const char *value);
/* Current value of an integer knob; also the read-only keys is_sorted, is_compact, cold_on_host, cold_sections (0, 1 =
 * slice lists, 3 = lists + site table in host memory), lists_absent, has_inline_sigs and dense_mit (layout of the uploaded image, -1
 * before an upload), and the read-only keys of the first lane's scoring workspace (0 before the first batch; set_option
 * refuses them with ISSL_E_ARG): ws_cap_guides (guides its arrays hold), ws_slot_width (hit slots per guide: 512 or 2048),
 * ws_fine_ways (placements per guide and bucket the pruned plan's arrays are sized for: 13 or 67), ws_cap_chunks (chunks of
 * the raw-record buffer), ws_cap_fitems (items of the pruned plan's list), ws_lean (1: the next batch is enqueued without
 * the grouping pass and the many-hit replays), ws_scan_verified (raw records of the lane's last finished batch that the scan's
 * own waves verified; the verify kernel took the others), and of the same batch which way its records went:
 * ws_scan_lds_buffers (buffers of records that the scan's waves verified from their LDS, which took no chunk: a lean batch on
 * the pruned plan, else 0), ws_scan_raw_top (one past the last chunk that such a batch copied a buffer to, where the verify
 * kernel stops; 0: no record left its wave) and ws_raw_chunks (chunks of the raw-record buffer handed out, the scan waves'
 * own included). */
int issl_index_get_option(const issl_index *idx, const char *key, long long *value);

/* ---- guides (A2, isslScoreOfftargets.cpp:63-71,82-89,275-305) ---------------------------- */

/* 2-bit pack n guides laid out as lines of `stride` bytes (seq_len chars then anything). */
int issl_encode_guides(const char *text, size_t n, size_t seq_len, size_t stride, uint64_t *out);
/* out must hold seq_len+1 bytes. */
int issl_decode_guide(uint64_t sig, size_t seq_len, char *out);
/* Query file rules of :275-294; *out is malloc'd (free with issl_free).  Large files are read and packed by several
 * threads. */
int issl_read_query_file(const char *path, size_t seq_len, uint64_t **out, size_t *n);

/* ---- output text (A12, isslScoreOfftargets.cpp:514-527) ------------------------------------- */
/* The scorer's stdout for n guides, in input order: "<seq>\t<MIT>\t<CFD>\n" with both scores as printf("%f") prints
 * them and "-1" for a score `method` (ISSL_METHOD_*) does not ask for (:517-525; ISSL_METHOD_UNKNOWN: "-1\t-1").  The text
 * comes in *n_spans consecutive pieces (formatted by up to `threads` threads, 0 = automatic; a million lines are
 * otherwise as long as their scoring): write them out one after the other, release with issl_free_spans.  The "%f" is
 * the library's own exact formatter (the binary value rounded to six decimals, ties to even: digit for digit glibc's
 * output), snprintf for negative, huge and non-finite values.  Host arithmetic only.  issl_free_spans hands the buffers
 * back to the library, which keeps up to 512 MB of them for the next call (a resident scorer formats page after page of the
 * same size, and a fresh buffer costs a page fault per 4 KiB when it is first written).  (ABI 6) */
typedef struct issl_span {
    char *data;
    size_t len;
} issl_span;
int issl_format_scores(const uint64_t *guides, const double *mit, const double *cfd, size_t n, size_t seq_len,
                       int method, int threads, issl_span **spans, size_t *n_spans);
void issl_free_spans(issl_span *spans, size_t n_spans);
void issl_free(void *p);

/* ---- scoring (A3-A11, isslScoreOfftargets.cpp:307-511) ------------------------------------ */

int issl_method_from_string(const char *s);

/* Score n guides held in host memory; mit/cfd receive 10000/(100+sum) per guide (:505-506).
 * Blocking.  Both outputs are always written (the reference prints -1 for a method that was not
 * requested, :517-525 -- that is the caller's business). */
int issl_score(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, double threshold,
               int method, double *mit, double *cfd);

/* Same with guides and outputs already in device memory of the index's device; asynchronous
 * on `stream` (a hipStream_t, may be NULL) except when the hit buffer must grow. */
int issl_score_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist,
                      double threshold, int method, double *d_mit, double *d_cfd, void *stream);

/* Enqueue one batch and return at once; any number of batches may be enqueued before issl_score_finish().
 * Batches run back to back on an internal stream of the index, independent of the caller's streams; use different
 * output buffers for batches whose results are consumed later.
 * `stream`: if not NULL the batch starts after the work enqueued on that stream so far (the producer of d_guides);
 * NULL means the inputs are ready now.  Results are valid after issl_score_finish(), or, on a stream, behind
 * issl_score_wait(idx, stream), which makes that stream wait for every batch enqueued so far (no host sync).
 * issl_score_finish() synchronises (internal streams and `stream`) and checks the batches: ISSL_E_RETRY means that a
 * batch needed more scratch space than was allocated (first large batch on an index; the buffers have been enlarged), or
 * that it was enqueued without the many-hit part of the pipeline (lean_tail option: a handle whose batches meet no guide
 * with more than 512 hits stops launching it) and did meet such a guide: the batches since the previous finish must be
 * enqueued again.  issl_last_stats() then describes the last
 * batch, with ms_scan averaged over all of them. */
int issl_score_device_async(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist,
                            double threshold, int method, double *d_mit, double *d_cfd, void *stream);
int issl_score_wait(issl_index *idx, void *stream);
int issl_score_finish(issl_index *idx, void *stream);

/* Parity helper: the scored off-targets of every guide in the reference's scoring order
 * (slice, then position in bucket), truncated by early exit exactly as :467-496.
 * *n_hits receives the total even when it exceeds cap. */
int issl_dump_hits(issl_index *idx, const uint64_t *guides, size_t n, int max_dist,
                   double threshold, int method, issl_hit *hits, size_t cap, size_t *n_hits);

/* ---- off-target report ---------------------------------------------------------------------- */
/* The off-targets of a guide are the candidates the reference scores at threshold 0 (maximum_sum = +inf, :326: the loops
 * of :330,344 never leave early): every site within max_dist (0..6), once, under its first matching slice.  Neither
 * operation takes a threshold or a method.  issl_dump_hits stays the early-exit-faithful parity view. */
#define ISSL_PROFILE_BINS 7 /* max_dist 0..6 */

/* One off-target with its score terms (40 bytes, no padding).  Records of a guide come in the reference's scoring order
 * (slice, then position in the bucket): adding a guide's mit (cfd) terms in record order in f64 and applying
 * 10000 / (100 + sum) gives the scores of issl_score at threshold 0.0, method "and", bit for bit. */
typedef struct {
    uint64_t site;  /* the site's packed signature (issl_decode_guide gives the 20-mer) */
    double mit;     /* addend of :392-396: local score of the mismatch mask x occ; 0.0 when dist == 0 */
    double cfd;     /* addend of :460: CFD product x occ; 1.0 x occ when dist == 0 */
    uint32_t guide; /* index into the guide batch */
    uint32_t id;    /* site id */
    uint32_t occ;   /* occurrences */
    uint16_t dist;  /* mismatches */
    uint16_t slice; /* first matching slice */
} issl_offtarget;

/* Per guide and distance d <= max_dist: the number of off-target sites and the sum of their occurrences; bins above
 * max_dist are zero. */
typedef struct {
    uint32_t sites[ISSL_PROFILE_BINS];
    uint32_t pad;
    uint64_t occurrences[ISSL_PROFILE_BINS];
} issl_profile;

/* Profiles of n guides in host memory (any n: cut into pieces like issl_score).  Runs the scoring pipeline with the
 * replay replaced by a kernel that bins every guide's verified hits by distance; no record is materialised.  Blocking. */
int issl_offtarget_profile(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, issl_profile *out);
/* Same with guides and profiles in device memory, one batch, on `stream` (may be NULL); returns when it is done. */
int issl_offtarget_profile_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist,
                                  issl_profile *d_out, void *stream);

/* Every off-target of n guides as a CSR list: guide i owns recs[offsets[i] .. offsets[i + 1]).  offsets (n + 1 words)
 * and *n_total are always complete; when *n_total > cap NO record is written and the call still returns ISSL_OK
 * (recs == NULL with cap == 0 is the counting call).  Any n: the batch is cut into pieces and at most one piece of
 * records is held on the device.  Blocking. */
int issl_offtargets(issl_index *idx, const uint64_t *guides, size_t n, int max_dist, uint64_t *offsets,
                    issl_offtarget *recs, size_t cap, size_t *n_total);
/* Same with guides, offsets and records in device memory, one batch, on `stream` (may be NULL); *n_total is host memory
 * and the call returns when the batch is done. */
int issl_offtargets_device(issl_index *idx, const uint64_t *d_guides, size_t n, int max_dist, uint64_t *d_offsets,
                           issl_offtarget *d_recs, size_t cap, size_t *n_total, void *stream);

int issl_last_stats(const issl_index *idx, issl_stats *out);

/* Sum over guides of the five bucket lengths (SURVEY 8d cross-check), host arithmetic only. */
int issl_count_candidates(const issl_index *idx, const uint64_t *guides, size_t n, uint64_t *out);

/* ---- caller-side thresholding (src/crackling/Crackling.py:780-835) ----------- */
/* What Crackling does with the scorer's stdout: the scores are read back from the "%f" text (6 decimals; -1 for a
 * score whose method was not requested, isslScoreOfftargets.cpp:517-525) and compared with the threshold under the
 * lower-cased, stripped method name (`mit`: MIT < t rejects; `cfd`; `and`: both below; `or`: either; `avg`: mean).
 * `method` is the string as configured: the scorer matches it exactly (:121-143) while the caller lower-cases it,
 * so "AND" prints -1/-1 and then rejects -- reproduced here.  accepted[i] = ISSL_VERDICT_REJECTED (0, CODE_REJECTED),
 * ISSL_VERDICT_ACCEPTED (1, CODE_ACCEPTED) or ISSL_VERDICT_NONE (the caller's if/elif chain matches no method and
 * leaves the guide untouched).  Host arithmetic only.  bin/isslScoreOfftargets writes "<20-mer>\t<0|1>\n" lines to
 * the file named by ISSL_VERDICTS when that variable is set (stdout is unchanged). */
enum { ISSL_VERDICT_REJECTED = 0, ISSL_VERDICT_ACCEPTED = 1, ISSL_VERDICT_NONE = 255 };
int issl_verdicts(const double *mit, const double *cfd, size_t n, double threshold, const char *method,
                  uint8_t *accepted);

/* ---- one process, several GPUs of the node ------------------------------------------------ */
/* The reference's outer loop is data-parallel over guides (isslScoreOfftargets.cpp:316-509 reads only the
 * index): a node replicates the HBM image on every listed device -- uploaded once on devices[0], then broadcast
 * with RCCL (ncclBroadcast over xGMI; peer copies when RCCL cannot be used, e.g. a device listed twice) -- and
 * scores every batch as a QUEUE OF CHUNKS (16 k - 256 k guides), one host thread per device taking the next chunk
 * when it has finished its last: the reference's static OpenMP split (:316) would leave the device that holds a
 * repeat-dense stretch of Crackling's genome-ordered guides working long after the others.  Scores land in input
 * order.  An image whose cold sections live in pinned host memory (issl_index_cold) is replicated hot part only, all
 * devices read the one host copy.  bin/isslScoreOfftargets uses a node when ISSL_DEVICES names several devices. */
typedef struct issl_node issl_node;

typedef struct {
    int n_devices;
    int used_rccl;         /* 1: image moved by ncclBroadcast, 0: hipMemcpyPeer */
    double ms_upload;      /* host -> devices[0] including the scan-stream transform */
    double ms_broadcast;   /* devices[0] -> all others */
    double ms_last_score;  /* wall time of the last issl_node_score call */
} issl_node_info;

/* idx has host arrays (opened from a file or built) or was built on devices[0] (issl_index_build_on_device); it stays
 * owned by the caller and must outlive the node.  devices may be NULL: then all visible devices are used. */
int issl_node_create(issl_index *idx, const int *devices, int n_devices, issl_node **out);
int issl_node_score(issl_node *node, const uint64_t *guides, size_t n, int max_dist, double threshold,
                    int method, double *mit, double *cfd);
int issl_node_get_info(const issl_node *node, issl_node_info *out);
/* Per device, for the last issl_node_score call: milliseconds spent scoring and guides scored (n >= n_devices). */
int issl_node_shard_times(const issl_node *node, double *busy_ms, uint64_t *guides, int n);
int issl_node_close(issl_node *node);

/* ---- off-target site extraction (the step before the index builder) ------------------------------ */
/* Counterpart of src/crackling/utils/extractOfftargets.py: every N20 site next to a PAM on either strand
 * (patterns of :23-24, overlapping matches, first 20 characters of the match, reverse-complemented for the
 * reverse pattern), sorted as text, duplicates kept, one per line.  Runs on `device`; no CPU fallback.
 * files[i]/lens[i]: the bytes of FASTA / multi-FASTA files.  *out_text is malloc'd (issl_free).
 * n_files == 1: the reference's single-file rules (lines stripped, every record counts); n_files > 1: its per-file
 * rules ('>' must be the first character of a header line, leading blanks stay in the sequence, a header line that
 * comes again in the same file replaces the earlier record).  INTEGRATION.md, "Index preparation". */
int issl_extract_from_memory(const char *const *files, const size_t *lens, int n_files, int device,
                             char **out_text, size_t *out_len, uint64_t *n_sites);
/* Same from files on disk into `output_path` (what bin/extractOfftargets calls). */
int issl_extract_offtargets(const char *const *inputs, int n_inputs, const char *output_path, int device,
                            uint64_t *n_sites);

/* ---- where a site lies in the genome: record, position, strand ----------------------------------------------------- */
/* The .issl format holds no coordinates.  A genome handle keeps the text the extraction scans -- the records of the
 * inputs, upper-cased and joined by the rules of the extraction above (n_files == 1: the single-file rules, n_files > 1:
 * the per-file rules) -- resident in the memory of `device` at 1 B per base, with the table of record starts, and
 * answers where given sites occur.
 *   location  a match of the extraction: a start i in a record's sequence where the forward pattern (strand 0) or the
 *             reverse pattern (strand 1) of extractOfftargets.py:23-24 matches -- exactly the matches the extraction turns
 *             into site lines.  The site of a forward match is seq[i:i+20].  The site of a reverse match is the reverse
 *             complement of seq[i:i+20], the FIRST 20 OF THE 23 matched characters (the reference's rule,
 *             extractOfftargets.py:97-110) -- not the 20 characters behind the reverse PAM, so do not expect the
 *             protospacer's own span there.  One start can match both patterns: two locations, two sites
 *   pos       = i, 0-based inside the record, counted in the record's sequence as the extraction builds it: with one
 *             input lines are stripped and joined (the usual FASTA coordinate); with several inputs the per-file rules
 *             apply and the leading blanks that count as sequence there are counted too
 *   record    index among the surviving records in the order the extraction joins them.  A record dropped by the
 *             repeated-header rule has no index; a header without sequence is a record of length 0; text before the
 *             first header is a record with an empty name.  name = the header line without '>' and without its line
 *             end, as the bytes stand in the file (issl_genome_record; valid until the handle is closed, not terminated)
 *   sites     packed signatures, as in issl_offtarget.site and issl_encode_guides
 * Site k of the call owns locs[offsets[k] .. offsets[k + 1]), sorted by (record, pos, strand).  A site that does not
 * occur has an empty range; a site named twice gets the same list twice.  offsets (n + 1 words) and *n_total are always
 * complete; when *n_total > cap NO location is written and the call still returns ISSL_OK (locs == NULL with cap == 0 is
 * the counting call) -- the rules of issl_offtargets.  The output is deterministic: the same bytes on every run.  Any n:
 * the query is cut into pieces of 2^22 sites, each of which scans the text once.  More than 2^32 - 1 locations in one
 * call: ISSL_E_UNSUPPORTED, as the extraction refuses.  No device: ISSL_E_DEVICE (no CPU fallback); NULL arguments and
 * n_files <= 0: ISSL_E_ARG; *out is NULL after a failed open.  ISSL_LOCATE_TIMING=1 (read when the handle is made) prints
 * one stderr line per call with the stage times and the counters of the scan.  One handle is used by one thread at a time. */
typedef struct issl_genome issl_genome; /* opaque */
typedef struct {
    uint64_t pos;    /* 0-based start of the match inside the record */
    uint32_t record; /* index of the record */
    uint32_t strand; /* 0: forward pattern, 1: reverse pattern */
} issl_location;     /* 16 bytes, no padding */

int issl_genome_open(const char *const *files, const size_t *lens, int n_files, int device, issl_genome **out);
/* Same from files on disk; a lone directory stands for its non-hidden entries in sorted order, as for bin/extractOfftargets. */
int issl_genome_open_files(const char *const *paths, int n_paths, int device, issl_genome **out);
int issl_genome_info(const issl_genome *g, uint64_t *n_records, uint64_t *n_bases);
int issl_genome_record(const issl_genome *g, uint64_t r, const char **name, size_t *name_len, uint64_t *length);
/* Sites, offsets and locations in host memory.  Blocking. */
int issl_genome_locate(issl_genome *g, const uint64_t *sites, size_t n, uint64_t *offsets, issl_location *locs, size_t cap,
                       size_t *n_total);
/* Same with sites, offsets and locations in the memory of the handle's device, on `stream` (may be NULL); *n_total is host
 * memory and the call returns when it is done. */
int issl_genome_locate_device(issl_genome *g, const uint64_t *d_sites, size_t n, uint64_t *d_offsets, issl_location *d_locs,
                              size_t cap, size_t *n_total, void *stream);
int issl_genome_close(issl_genome *g);

/* ---- genome search: any PAM pattern, any guide length, up to k mismatches ---------------------------------------- */
/* An index-free answer on a genome handle: where does a query bind with at most max_dist mismatches, for a nuclease whose
 * PAM and guide length a pattern describes.  Nothing of the extraction's rules is built in: no 20-mer, no N[AG]G, no
 * exclusion of sites that start with T, and the minus strand gives the protospacer's own span.
 *   pattern   a string of length L, 1 <= L <= 32, in IUPAC codes A C G T R Y S W K M B D H V N, either letter case;
 *             position i allows the bases its code stands for
 *   query     a string of the same length L over A C G T N, either case; N: this position is not compared.  A query of
 *             only N is legal: it lists every window the pattern admits, each at distance 0
 *   window    w = seq[pos : pos + L] of ONE record of the handle's text (upper-cased, as the handle holds it), all L
 *             characters in ACGT; anything else, the record separator included, disqualifies the window, so no window
 *             spans two records
 *   strand    strand 0 reads t = w, strand 1 reads t = the reverse complement of w
 *   hit       strand s of the window at pos is a hit of query q when t[i] is allowed by pattern[i] for every i, and
 *             dist = #{ i : q[i] != 'N' and q[i] != t[i] } <= max_dist.  The pattern test and the comparison are
 *             independent of each other.  One window can be a hit on both strands: two rows
 *   pos       0-based start of w in the record, in forward coordinates FOR BOTH STRANDS: issl_location.pos's coordinate
 *   site      t packed as issl_encode_guides packs it: base i in bits 2i and 2i + 1, bits above 2L zero
 *   mism      bit i is set when q[i] != 'N' and q[i] != t[i]
 *   max_dist  0 <= max_dist <= L
 * Query k owns hits[offsets[k] .. offsets[k + 1]), sorted by (record, pos, strand); `query` is k.  The other rules are
 * those of issl_genome_locate: offsets (n + 1 words) and *n_total are always complete; when *n_total > cap NO row is
 * written and the call still returns ISSL_OK (hits == NULL with cap == 0 is the counting call); the bytes are the same on
 * every run and do not depend on how the call is cut into pieces; a query named twice gets the same list twice; n == 0:
 * ISSL_OK with offsets[0] = 0.  More than 2^32 - 1 hits in one call: ISSL_E_UNSUPPORTED.  No device: ISSL_E_DEVICE (no CPU
 * fallback).  NULL arguments, L outside 1..32, a character outside the two alphabets, max_dist outside 0..L, pattern bits
 * at or above L, a position that allows no base, and (host queries) query bits at or above 2L: ISSL_E_ARG before any device
 * work; the message names the offending position.  With the extraction's forward pattern VNNNNNNNNNNNNNNNNNNNNRG the
 * strand-0 hits of guide + "NNN" and the strand-1 hits of "NNN" + guide are the rows of issl_offtarget_landings.
 * ISSL_LOCATE_TIMING=1 prints one stderr line per piece of 2^22 queries with the stage times. */
typedef struct { uint32_t allow[4]; uint32_t length; uint32_t reserved[3]; } issl_search_pattern; /* 32 B; allow[b] bit i: base b (A,C,G,T) allowed at i */
typedef struct { uint64_t sig; uint64_t care; } issl_search_query;   /* 16 B; sig: N packs as 0; care: bits 2i,2i+1 set where compared */
typedef struct { uint64_t site; uint64_t pos; uint32_t record; uint32_t query; uint32_t mism;
                 uint8_t strand; uint8_t dist; uint8_t reserved[2]; } issl_search_hit;            /* 32 B, no padding, reserved = 0 */

/* Pattern text (NUL-terminated) and n query texts of its length, query k at queries + k * stride, into the structs the
 * search takes.  Host only, no device needed.  queries may be NULL when n == 0. */
int issl_search_prepare(const char *pattern, const char *queries, size_t n, size_t stride,
                        issl_search_pattern *pat, issl_search_query *out);
/* pat is host memory in every call.  Queries, offsets and hits in host memory.  Blocking. */
int issl_genome_search(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                       uint64_t *offsets, issl_search_hit *hits, size_t cap, size_t *n_total);
/* Same with queries, offsets and hits in the memory of the handle's device, on `stream` (may be NULL); *n_total is host
 * memory and the call returns when it is done.  The queries are not checked. */
int issl_genome_search_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n, int max_dist,
                              uint64_t *d_offsets, issl_search_hit *d_hits, size_t cap, size_t *n_total, void *stream);
/* counts[k * (max_dist + 1) + d]: hits of query k at distance d.  Reduced on the device: no row reaches the host, and
 * the limit of 2^32 - 1 hits does not apply. */
int issl_genome_search_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                               uint64_t *counts /* n * (max_dist + 1): hits of query k at distance d */);
int issl_genome_search_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                      int max_dist, uint64_t *d_counts, void *stream);

/* ---- genome search with DNA and RNA bulges beside the mismatches ------------------------------------------------------- */
/* Binding with a bulge: one to three bases of the DNA site that pair with nothing in the guide (a DNA bulge), or bases of
 * the guide that pair with nothing in the site (an RNA bulge).  A bulged hit is defined through issl_genome_search:
 *   pattern, query, window, strand, t, pos, site packing: as for issl_genome_search.  Pattern and queries have length L
 *   span      guide_start g0 and guide_length G: the pattern positions where the protospacer lies.  Given by the caller,
 *             never guessed (N * 21 + NNGRRT shows why).  2 <= G and g0 + G <= L
 *   limits    max_dna D and max_rna R, each 0..3, with L + D <= 32 and R <= G - 2.  When D + R > 0 the pattern must allow
 *             all four bases at positions g0 + 1 .. g0 + G - 2; the first and last position of the span, and everything
 *             outside it, may carry any code
 *   alignment (b, i), b signed, -R..D.  b = 0 has only i = 0: the pair (pattern, query) itself.  b = d > 0 is a DNA bulge
 *             of d bases, i = 1..G-1: the pair is P' = P[:g0+i] + 'N'*d + P[g0+i:], q' built likewise.  b = -r < 0 is an
 *             RNA bulge, i = 1..G-1-r: P' = P[:g0+i] + P[g0+i+r:], q' built likewise.  The window of alignment (b, i) has
 *             L + b bases; it hits when it is a hit of issl_genome_search for (P', q', max_dist), and dist(b, i) is that
 *             distance.  By the rule on the span's interior P' is the same for every i of one b
 *   row       one per (query, record, pos, strand, b) that has at least one hitting alignment.  dist is the minimum of
 *             dist(b, i) over i, `at` the smallest i that reaches it (0 for b = 0), `bulge` is b, `site` is t packed, L + b
 *             bases.  mism is in QUERY coordinates: bit j is set when query position j is paired in alignment (b, at), is
 *             not N, and differs from its partner.  The partner of j for b = d: t[j] for j < g0 + at, otherwise t[j + d];
 *             for b = -r: t[j] for j < g0 + at, none for g0 + at <= j < g0 + at + r (bit clear), t[j - r] above that
 *   NO FILTERING: a locus that matches at b = 0 also shows up in the shifted windows of the other b with a distance of
 *             about |b|.  These rows are listed, as Cas-OFFinder lists them
 *   order     query k owns hits[offsets[k] .. offsets[k + 1]), sorted by (record, pos, strand, bulge as a signed number)
 *   max_dist  0..L
 *   profile   counts[(k * (R + D + 1) + (b + R)) * (max_dist + 1) + dist]: the rows of query k with bulge b at that
 *             minimum distance.  Reduced on the device
 * The capacity rule, *n_total, the limit of 2^32 - 1 rows, n == 0, duplicated queries and "the bytes do not depend on the
 * cut into pieces" (here of 2^19 queries) are as for issl_genome_search.  ISSL_E_ARG before any device work, with a message
 * that names the offender: a span out of range, D or R above 3, L + D > 32, R > G - 2, a restricted pattern position that
 * is not N (the message names the position), and everything issl_genome_search refuses.  With D = R = 0 the rows are those
 * of issl_genome_search with bulge = at = 0. */
typedef struct { uint32_t guide_start, guide_length, max_dna, max_rna; } issl_search_bulges;       /* 16 B */
typedef struct { uint64_t site; uint64_t pos; uint32_t record; uint32_t query; uint32_t mism;
                 uint8_t strand; uint8_t dist; int8_t bulge; uint8_t at; } issl_bulge_hit;         /* 32 B, no padding */
/* pat and bulges are host memory in every call.  Queries, offsets and hits in host memory.  Blocking. */
int issl_genome_search_bulges(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                              const issl_search_query *queries, size_t n, int max_dist, uint64_t *offsets, issl_bulge_hit *hits,
                              size_t cap, size_t *n_total);
/* Same with queries, offsets and hits in the memory of the handle's device, on `stream` (may be NULL); *n_total is host
 * memory and the call returns when it is done.  The queries are not checked. */
int issl_genome_search_bulges_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                     const issl_search_query *d_queries, size_t n, int max_dist, uint64_t *d_offsets,
                                     issl_bulge_hit *d_hits, size_t cap, size_t *n_total, void *stream);
int issl_genome_search_bulges_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                      const issl_search_query *queries, size_t n, int max_dist,
                                      uint64_t *counts /* n * (R + D + 1) * (max_dist + 1) */);
int issl_genome_search_bulges_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                             const issl_search_query *d_queries, size_t n, int max_dist, uint64_t *d_counts,
                                             void *stream);

/* ---- variant-aware genome search: IUPAC codes in the text, SNPs from a VCF ------------------------------------------------ */
/* A reference assembly is one haplotype; a SNP can create an off-target, or a PAM, that it does not show.  This search
 * reads IUPAC ambiguity codes in the handle's text as sets of bases.  issl_genome_search_variants* is issl_genome_search*
 * with the differences below; everything not named is the plain search's rule: pattern, query alphabet, pos in forward
 * coordinates for both strands, the sort by (record, pos, strand), the capacity rule, *n_total, the limit of 2^32 - 1
 * rows, n == 0, duplicated queries, "the bytes do not depend on the cut into pieces", the argument errors and
 * ISSL_LOCATE_TIMING.
 *   window    w = seq[pos : pos + L] of ONE record, every character one of the 14 codes A C G T R Y S W K M B D H V.  N
 *             disqualifies the window, as does any other byte and the record separator: an assembly gap matches nothing.
 *             S(c) is the set of bases code c stands for; a position is AMBIGUOUS when S(c) has more than one base.  A
 *             window with more than max_variants ambiguous positions is disqualified (max_variants: 0..L)
 *   strand    strand 0 reads the sets T[i] = S(w[i]); strand 1 reads T[i] = comp(S(w[L-1-i])), comp mapping a set base by
 *             base, A<->T and C<->G: R<->Y, K<->M, B<->V, D<->H, S and W are their own complements
 *   hit       A[i] = T[i] intersected with the bases pattern[i] allows.  The window-strand is admitted when every A[i] is
 *             non-empty.  Position i MATCHES when q[i] is N or q[i] is in A[i]; dist is the number of positions that do not
 *             match, and dist <= max_dist is a hit.  Equivalently dist is the least distance of issl_genome_search over all
 *             the sequences the window stands for that the pattern admits: the positions are independent.  A base the
 *             text's set holds but the pattern forbids is a mismatch
 *   row       issl_variant_hit.  site[b] bit i is set when base b of A C G T is in T[i] -- the set the strand reads, NOT
 *             intersected with the pattern; the convention of issl_search_pattern.allow.  mism bit i: position i does not
 *             match.  n_var: the ambiguous positions of the window.  reserved = 0
 *   profile   counts[k * (max_dist + 1) + d], as for issl_genome_search_profile
 * max_variants outside 0..L: ISSL_E_ARG before any device work.  With max_variants = 0 on any text, and with any
 * max_variants on a text without ambiguity codes, the rows are those of issl_genome_search field by field, site re-encoded
 * one-hot and n_var = 0.  Bulges on such a text: issl_genome_search_bulges_variants*, below. */
typedef struct { uint64_t pos; uint32_t site[4]; uint32_t record; uint32_t query; uint32_t mism;
                 uint8_t strand; uint8_t dist; uint8_t n_var; uint8_t reserved; } issl_variant_hit; /* 40 B, no padding */
int issl_genome_search_variants(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                                int max_variants, uint64_t *offsets, issl_variant_hit *hits, size_t cap, size_t *n_total);
int issl_genome_search_variants_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                       int max_dist, int max_variants, uint64_t *d_offsets, issl_variant_hit *d_hits, size_t cap,
                                       size_t *n_total, void *stream);
int issl_genome_search_variants_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *queries, size_t n,
                                        int max_dist, int max_variants, uint64_t *counts /* n * (max_dist + 1) */);
int issl_genome_search_variants_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_query *d_queries,
                                               size_t n, int max_dist, int max_variants, uint64_t *d_counts, void *stream);

/* SNPs onto a resident genome.  An issl_snp names a place (record, 0-based pos inside it), its reference base `ref` (one
 * bit of A C G T = 1, 2, 4, 8) and a non-empty set `alt` of alternative bases (bits of the same).
 *
 * issl_vcf_snps reads them from the text of a VCF file (plain text, no gzip).  Host only, no device needed.  names,
 * name_lens and lengths describe the n_records records as issl_genome_record gives them.
 *   lines     end with "\n" or "\r\n"; empty lines and lines that begin with '#' are skipped.  Fields are tab-separated;
 *             CHROM POS REF ALT are fields 1, 2, 4, 5.  A line with fewer than five fields or a POS that is not all digits:
 *             ISSL_E_ARG, the message names the line (1-based)
 *   CHROM     is compared with a record's name up to its first blank (space, TAB, LF, VT, FF, CR), the first record of a
 *             name standing for it.  No such record: the line is skipped and counted in unknown_chrom
 *   POS       1-based.  0 or beyond the record: skipped and counted in beyond_record
 *   alleles   a line counts when REF is one base of ACGT (either case); of its comma-separated ALT alleles those that are
 *             one base of ACGT are taken and ORed into one issl_snp.  Every other allele -- an indel, `*`, `.`, a symbolic
 *             <...>, and every allele of a line whose REF is not one base -- is skipped and counted in alleles_skipped; a
 *             line without a usable allele is counted in no_allele
 * The checks are made in this order, and a skipped line is counted once.  out receives one entry per remaining line in file
 * order; *n is always complete, and when *n > cap nothing is written (out == NULL with cap == 0 is the counting call).
 * counts may be NULL.
 *
 * issl_genome_apply_snps writes them into the handle's text as ambiguity codes.  The host checks the ranges (record, pos,
 * ref one bit, alt 1..15), sorts by (record, pos) and merges the entries of one place: their ref must agree, their alt is
 * ORed.  On the device every place is checked first: the text byte must be one of the 14 codes and hold ref, and its set
 * united with alt must not be all four bases (that letter is N, which no window may hold).  If any check
 * fails the call returns ISSL_E_ARG, the message names the smallest failing input index, and the text is untouched.
 * Otherwise the byte becomes the letter of S(byte) united with alt.  *n_changed (may be NULL): the places whose byte changed;
 * applying the same list again changes nothing.  THE HANDLE'S TEXT IS CHANGED FOR EVERY LATER CALL: issl_genome_locate,
 * issl_genome_occurrences, issl_genome_search and issl_genome_search_bulges skip every window over an ambiguity code as
 * over any byte outside ACGT, in their host and _device forms.  So do the other entry points that scan the handle's text,
 * none of which keeps a copy of it or an index over it: issl_genome_occurrences_paged* (the pass of
 * issl_genome_occurrences with other page boundaries) and issl_offtarget_landings* / issl_offtarget_landing_profile* (locate's
 * scan: an off-target whose every place now holds a code is counted in `absent`, one that kept some of its places has fewer
 * landings than `occ`, which stays the index's count).  Only issl_genome_search_variants* and
 * issl_genome_search_bulges_variants* read a code as a set of bases.
 * issl_genome_apply_vcf chains the two with the handle's own records. */
typedef struct { uint64_t pos; uint32_t record; uint8_t ref; uint8_t alt; uint8_t reserved[2]; } issl_snp; /* 16 B */
typedef struct { uint64_t lines;           /* data lines read */
                 uint64_t snps;            /* entries they gave (*n) */
                 uint64_t alleles_skipped; uint64_t no_allele; uint64_t unknown_chrom; uint64_t beyond_record; } issl_vcf_counts; /* 48 B */
int issl_vcf_snps(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                  size_t n_records, issl_snp *out, size_t cap, size_t *n, issl_vcf_counts *counts);
int issl_genome_apply_snps(issl_genome *g, const issl_snp *snps, size_t n, uint64_t *n_changed);
int issl_genome_apply_vcf(issl_genome *g, const char *vcf, size_t len, issl_vcf_counts *counts, uint64_t *n_changed);

/* ---- genome search with bulges on a variant-aware text ------------------------------------------------------------------ */
/* Where a guide binds with mismatches and a bulge on any haplotype the text's ambiguity codes stand for: a SNP can create a
 * bulged off-target that the reference assembly does not show, as it can create a mismatch one.
 * issl_genome_search_bulges_variants* is issl_genome_search_bulges* with issl_genome_search_variants in the place where its
 * definition names issl_genome_search.  Everything not named below is the bulge search's rule: the span, the limits D and R
 * and their checks, the alignments (b, i) and the derived pairs P' and q', `at` as the smallest break point that reaches
 * the minimum, mism in query coordinates, NO FILTERING, the order (record, pos, strand, bulge as a signed number), the
 * capacity rule and *n_total, the limit of 2^32 - 1 rows, n == 0, duplicated queries, "the bytes do not depend on the cut
 * into pieces" (of 2^19 queries), and every ISSL_E_ARG of the bulge search.
 *   hit       alignment (b, i) hits at a window of L + b characters when that window is a hit of
 *             issl_genome_search_variants for (P', q', max_dist, max_variants); dist(b, i) is that distance
 *   window    every character is one of the 14 codes A C G T R Y S W K M B D H V; N, any other byte and a record end
 *             disqualify it.  The ambiguous positions are counted over all L + b characters, the unpaired bases of a DNA
 *             bulge included; more than max_variants of them disqualify the window for this b (and only for this b: the
 *             windows of the other b at the same pos have other characters)
 *   match     a position matches when the query's base is in the text's set cut by the pattern's; a base the text holds
 *             but the pattern forbids is a mismatch; a window-strand is admitted when every position's cut set is non-empty
 *   row       issl_bulge_variant_hit.  site: the sets the strand reads, NOT cut by the pattern, L + b positions, in
 *             issl_variant_hit.site's convention; n_var: the ambiguous positions of the window; reserved = 0
 *   profile   counts[(k * (R + D + 1) + (b + R)) * (max_dist + 1) + dist], as for issl_genome_search_bulges_profile
 * max_variants outside 0..L: ISSL_E_ARG before any device work.  With D = R = 0 the rows are those of
 * issl_genome_search_variants field by field, with bulge = at = 0.  With max_variants = 0 on any text, and with any
 * max_variants on a text without ambiguity codes, the rows are those of issl_genome_search_bulges field by field, site
 * re-encoded one-hot and n_var = 0.  ISSL_LOCATE_TIMING=1 prints one stderr line per piece, tagged [issl bulges+variants]. */
typedef struct { uint64_t pos; uint32_t site[4]; uint32_t record; uint32_t query; uint32_t mism;
                 uint8_t strand; uint8_t dist; uint8_t n_var; int8_t bulge; uint8_t at; uint8_t reserved[7]; } issl_bulge_variant_hit; /* 48 B, no padding */
int issl_genome_search_bulges_variants(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                       const issl_search_query *queries, size_t n, int max_dist, int max_variants, uint64_t *offsets,
                                       issl_bulge_variant_hit *hits, size_t cap, size_t *n_total);
int issl_genome_search_bulges_variants_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                              const issl_search_query *d_queries, size_t n, int max_dist, int max_variants,
                                              uint64_t *d_offsets, issl_bulge_variant_hit *d_hits, size_t cap, size_t *n_total,
                                              void *stream);
int issl_genome_search_bulges_variants_profile(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                               const issl_search_query *queries, size_t n, int max_dist, int max_variants,
                                               uint64_t *counts /* n * (R + D + 1) * (max_dist + 1) */);
int issl_genome_search_bulges_variants_profile_device(issl_genome *g, const issl_search_pattern *pat, const issl_search_bulges *bulges,
                                                      const issl_search_query *d_queries, size_t n, int max_dist, int max_variants,
                                                      uint64_t *d_counts, void *stream);

/* ---- the ALT haplotypes of indels ------------------------------------------------------------------------------------------ */
/* An insertion or a deletion moves a PAM against a protospacer: it creates and destroys off-targets that no substitution can,
 * and issl_vcf_snps skips every such allele.  Here the ALT haplotype of an indel is searched as TEXT: for one window length W
 * an indel becomes a STRIP -- the W - 1 bases ahead of the edit, the ALT allele, the W - 1 bases behind it, cut from the
 * resident text as it stands (with the ambiguity codes applied SNPs left there) -- and the strips, one per indel, are the
 * records of a second resident text that issl_genome_search_variants searches as it is.  A strip holds exactly the windows of
 * the ALT haplotype that overlap the edit, and none that the reference text shows at those coordinates.
 *
 * An issl_indel replaces ref_len >= 1 bases at (record, 0-based pos) by alt_len >= 1 bases, as a VCF line gives them with
 * the anchor base: deletions, insertions, multi-base substitutions and complex alleles are this one thing.  Its bases are
 * alleles[ref_at .. ref_at + ref_len) and alleles[alt_at .. alt_at + alt_len), a caller-owned buffer over ACGT in either
 * case (upper-cased on the way in); each length is at most ISSL_INDEL_MAX_ALLELE.
 *   trim      the common suffix of REF and ALT is removed first, then the common prefix of what is left: (p, REF', ALT') with
 *             p = pos + the prefix removed.  One of REF', ALT' is non-empty: an entry that changes nothing is refused
 *             (ISSL_E_ARG).  Nothing is re-aligned against the genome
 *
 * issl_vcf_indels reads them from a VCF's text.  Host only.  Lines, fields, CHROM, the two malformed-line errors,
 * unknown_chrom and beyond_record (POS) are issl_vcf_snps's.  Then, in this order: a REF that is empty or not all ACGT --
 * every ALT allele of the line is counted in alleles_skipped and the line in no_allele; a REF that runs past the record's
 * end -- beyond_record; then per ALT allele, left to right, the allele is taken when it is one or more bases of ACGT, differs
 * from REF ignoring case, and REF and ALT are not both one base long (a SNP: issl_vcf_snps's share).  A taken allele whose REF
 * or ALT is longer than ISSL_INDEL_MAX_ALLELE is counted in too_long instead; every other allele in alleles_skipped; a line
 * that gave nothing in no_allele.  out receives one issl_indel per taken allele in file order, and its REF bytes, then its ALT
 * bytes, as they stand in the file, are appended to `alleles`.  *n and *alleles_len are always complete; nothing is written
 * to either buffer when one of them exceeds its capacity (NULL with capacity 0 is the counting call).  counts may be NULL.
 *
 * issl_haplotypes_open builds the strips for ONE window length `window` (1..32, never guessed) on g's device.  The host
 * checks every entry (ISSL_E_ARG, the message names it): record in range, pos + ref_len within the record, the lengths
 * 1..ISSL_INDEL_MAX_ALLELE, the offsets inside `alleles`, every byte one of ACGT, not a no-op.  With
 *   left = min(window - 1, p),  right = min(window - 1, length - p - |REF'|)
 * strip k is the `left` text bytes ahead of p, ALT', the `right` text bytes from p + |REF'| on, and a separator; strips lie in
 * input order.  On the device every base of the UNTRIMMED REF must lie in the set of its text byte (so a SNP applied there
 * earlier is fine); if any entry fails the call returns ISSL_E_ARG, the message names the smallest failing input index, and
 * no handle is made.  Then the strips are gathered.  THE STRIPS ARE A SNAPSHOT: SNPs applied to g after the open do not
 * reach them, and g may be closed before h.  n == 0 gives a handle without strips.  A strip text of 2^41 bytes or more, or
 * more than 2^32 - 1 entries: ISSL_E_UNSUPPORTED.  Memory: about 2 * window + |ALT'| + 33 bytes per indel (text, an 8-byte
 * start and a 32-byte table entry), plus 40 bytes per row of scratch during a search call.
 * issl_haplotypes_open_vcf chains issl_vcf_indels and issl_haplotypes_open with the handle's own records.
 *
 * issl_haplotypes_search* have the signatures of issl_genome_search_variants* with h in the place of g.
 * pat->length != window: ISSL_E_ARG before any device work.
 *   hit       a hit of issl_genome_search_variants on the ALT haplotype of ONE indel, taken alone on the text as it stood at
 *             the open, at a window that overlaps the edit: with ALT' non-empty the window holds at least one base of ALT';
 *             with ALT' empty it holds both the base ahead of the junction and the base behind it
 *   row       issl_haplotype_hit.  site, mism, dist, n_var, strand, query: the variant search's.  indel: the input index;
 *             record: the reference record.  With s the window's start in its strip, edit_at = left - s: the window index
 *             of the first ALT' base, or of the first base behind a deletion's junction; negative when the window starts
 *             inside ALT'.  pos is the reference position of the window's first base: p - left + s for s < left; p for
 *             left <= s < left + |ALT'|; p + |REF'| + (s - left - |ALT'|) behind that.  reserved = 0
 *   NO FILTERING: in a repeat such a window can spell what the reference text spells too; it is listed.  ONE INDEL AT A
 *             TIME: two indels closer than a window are never combined, and an indel given twice gives its rows twice.
 *             No bulges: the strips serve one window length
 *   order     query k owns hits[offsets[k] .. offsets[k + 1]), sorted by (indel, s, strand)
 *   profile   counts[k * (max_dist + 1) + d], the variant profile of the strips
 * Everything else is the variant search's rule: the capacity rule, *n_total, n == 0, duplicated queries, pieces, the
 * argument errors, max_variants. */
#define ISSL_INDEL_MAX_ALLELE 65535
typedef struct { uint64_t pos;        /* 0-based inside the record, of the first REF base */
                 uint32_t record, ref_len, alt_len;
                 uint32_t ref_at, alt_at;   /* where the REF / ALT bases start in the allele text */
                 uint32_t reserved; } issl_indel;                          /* 32 B */
typedef struct { uint64_t lines, indels, alleles_skipped, no_allele, unknown_chrom, beyond_record, too_long; } issl_vcf_indel_counts; /* 56 B */
typedef struct { uint64_t pos; uint32_t site[4]; uint32_t record; uint32_t query; uint32_t mism;
                 uint8_t strand, dist, n_var, reserved; uint32_t indel; int32_t edit_at; } issl_haplotype_hit; /* 48 B, no padding */
typedef struct issl_haplotypes issl_haplotypes; /* opaque; owns device memory */
int issl_vcf_indels(const char *vcf, size_t len, const char *const *names, const size_t *name_lens, const uint64_t *lengths,
                    size_t n_records, issl_indel *out, size_t cap, size_t *n, char *alleles, size_t alleles_cap, size_t *alleles_len,
                    issl_vcf_indel_counts *counts);
int issl_haplotypes_open(issl_genome *g, const issl_indel *indels, size_t n, const char *alleles, size_t alleles_len, int window,
                         issl_haplotypes **out);
int issl_haplotypes_open_vcf(issl_genome *g, const char *vcf, size_t len, int window, issl_vcf_indel_counts *counts,
                             issl_haplotypes **out);
int issl_haplotypes_info(const issl_haplotypes *h, uint64_t *n_indels, uint64_t *text_bytes, uint32_t *window);
int issl_haplotypes_close(issl_haplotypes *h);
int issl_haplotypes_search(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *queries, size_t n, int max_dist,
                           int max_variants, uint64_t *offsets, issl_haplotype_hit *hits, size_t cap, size_t *n_total);
int issl_haplotypes_search_device(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *d_queries, size_t n,
                                  int max_dist, int max_variants, uint64_t *d_offsets, issl_haplotype_hit *d_hits, size_t cap,
                                  size_t *n_total, void *stream);
int issl_haplotypes_search_profile(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *queries, size_t n,
                                   int max_dist, int max_variants, uint64_t *counts /* n * (max_dist + 1) */);
int issl_haplotypes_search_profile_device(issl_haplotypes *h, const issl_search_pattern *pat, const issl_search_query *d_queries,
                                          size_t n, int max_dist, int max_variants, uint64_t *d_counts, void *stream);

/* ---- the Bowtie step: exact occurrences of a guide's eight reads ----------------------------------------------------- */
/* Counterpart of src/crackling/Crackling.py:600-725 on a genome handle.  For every guide the reference aligns eight reads,
 * the guide's 20-mer followed by AGG, CGG, GGG, TGG, AAG, CAG, GAG, TAG (variants 0..7), and counts the reads that align
 * without a mismatch (XM:i:0), once more when a second such alignment exists (XS:i:0).  Here the same figures are exact
 * counts over the text:
 *   occurrence  of read r: (record, pos, strand) with seq[pos:pos+23] == r (strand 0) or == the reverse complement of r
 *               (strand 1); pos is 0-based in the record's sequence as for issl_location, the window lies inside one record
 *               and holds A, C, G, T only.  One start can be an occurrence on both strands (of different reads)
 *   sites       n packed 20-mer signatures (issl_encode_guides), duplicates allowed
 *   page_length the reference works through its guides in pages of this many (Paginator.py; 0: one page); sites are the
 *               guides in that order
 *   verdicts    the reference reads Bowtie's output in groups of eight lines, one group per guide, and files the reads of
 *               a page under their text.  The guide a group speaks about is looked up under the sequence its first line
 *               prints -- read 0, reverse-complemented when it aligned to strand 1 -- and then under that sequence's
 *               reverse complement.  So a group names the LAST site of its page with its own 20-mer, except when its
 *               read 0 first occurs on strand 1 and the 20 characters that start that occurrence (C, C, T and the guide's
 *               bases 19..3 complemented) are the 20-mer of a site of the page and the last three one of the eight PAMs
 *               (the guide starts with C and C or T): then it names the last site of the page with THAT 20-mer.  The
 *               window CCT N{18} NGG, a guide on both strands, is the common case: the group of the strand-1 guide sets
 *               the verdict of the strand-0 guide.  The named site receives the group's verdict (its nb > 1 rejects),
 *               chromosome and position; of several groups that name one site the last wins; a site that no group names
 *               stays untested.  This is kept as the reference does it
 * rows[k] answers sites[k].  The output is deterministic: the same bytes on every run, and no row depends on how the
 * call is cut into pieces (of 2^22 sites, each of which scans the text once).  n == 0: ISSL_OK, nothing is written.  NULL
 * arguments and a signature with bits above its 20 bases: ISSL_E_ARG, checked before any row is written.  More than
 * 2^32 - 2 sites in one call: ISSL_E_UNSUPPORTED.  No device: ISSL_E_DEVICE (no CPU fallback).  ISSL_LOCATE_TIMING=1
 * prints one stderr line per piece with the stage times and the counters of the scan, and one for the verdicts.
 * What a real Bowtie2 run can answer differently: it may miss a second perfect alignment within its effort limits; for a
 * read 0 without a perfect occurrence it reports its best inexact alignment where record is 0xFFFFFFFF here; among equal
 * alignments it picks at random where this step reports the least (record, pos, strand). */
typedef struct {
    uint64_t pos;          /* first occurrence of read 0 of the source's 20-mer in (record, pos, strand) order -- the site's own
                              when no group names it: 0-based start; 0 when there is none */
    uint32_t record;       /* its record; 0xFFFFFFFF when there is none */
    uint32_t n_perfect;    /* occurrences of all eight reads of the site's 20-mer, saturating */
    uint8_t aligned;       /* bit v: read v of the site's 20-mer has at least one occurrence */
    uint8_t repeated;      /* bit v: read v has at least two */
    uint8_t nb;            /* popcount(aligned) + popcount(repeated): the reference's nb_occurences of the site's own group */
    uint8_t strand;        /* of the occurrence pos and record name; 0 when there is none */
    uint8_t owner;         /* 1: a group names this site (source is valid) */
    uint8_t code;          /* passedBowtie: 2 (untested, '?') when owner == 0; else 0 (rejected) when the source's nb > 1, else 1 */
    uint8_t reserved[2];   /* 0 */
    uint32_t source;       /* the site whose group set this verdict: the last one that names this site; 0xFFFFFFFF when none.
                              source == k, or another site with the same 20-mer, unless the rule above applies */
    uint32_t reserved2;    /* 0 */
} issl_occurrence;         /* 32 bytes, no padding */

/* Sites and rows in host memory.  Blocking. */
int issl_genome_occurrences(issl_genome *g, const uint64_t *sites, size_t n, size_t page_length, issl_occurrence *rows);
/* Same with sites and rows in the memory of the handle's device, on `stream` (may be NULL); the sites are not copied to
 * the host and not changed, and the call returns when the rows are written. */
int issl_genome_occurrences_device(issl_genome *g, const uint64_t *d_sites, size_t n, size_t page_length, issl_occurrence *d_rows,
                                   void *stream);
/* The same two calls for pages that are not all of one length: the pages of a run in batches ([input] batch-size) start
 * again with every batch (issl_consensus_selection_pages makes them).  page_starts has n_pages + 1 entries, page p is sites
 * [page_starts[p], page_starts[p + 1]): page_starts[0] == 0, page_starts[n_pages] == n, no entry below the one before it;
 * equal neighbours are an empty page.  The boundaries are checked on the device before any row is written: ISSL_E_ARG
 * otherwise, as for a NULL page_starts unless n and n_pages are both 0, which is ISSL_OK.  The boundaries of a uniform
 * page_length give the bytes of the calls above; pieces and pages still change no row but through `source` and what
 * comes from it.  page_starts is host memory in the first call and device memory in the second. */
int issl_genome_occurrences_paged(issl_genome *g, const uint64_t *sites, size_t n, const uint64_t *page_starts, size_t n_pages,
                                  issl_occurrence *rows);
int issl_genome_occurrences_paged_device(issl_genome *g, const uint64_t *d_sites, size_t n, const uint64_t *d_page_starts,
                                         size_t n_pages, issl_occurrence *d_rows, void *stream);
/* The same rows, byte for byte, and beside them the figure the reference's log prints for the step (:709-717, `failed`):
 * d_page_events[p], n_pages words of device memory, = the groups of page p that reject the site they name while that site is
 * not rejected.  The groups of a page are walked in the order of its sites, and several can name one site -- sites of a page
 * that share a 20-mer name the last of them, and a strand-1 guide can name the strand-0 guide of its window (above) -- so this
 * is a count of events, not of rows: a site named reject, accept counts once and ends accepted; named reject, accept, reject
 * it counts twice; the rows know the last group only.  The figure of a batch is the sum over its pages.  A NULL
 * d_page_events with n_pages above 0: ISSL_E_ARG. */
int issl_genome_occurrences_paged_events_device(issl_genome *g, const uint64_t *d_sites, size_t n, const uint64_t *d_page_starts,
                                                size_t n_pages, issl_occurrence *d_rows, uint32_t *d_page_events, void *stream);

/* ---- candidate guides from FASTA: Crackling's extraction step ------------------------------------------------------- */
/* Counterpart of src/crackling/Crackling.py:151-305: the candidate 23-mers of the inputs, on `device`; no CPU fallback.
 *   inputs    files[i]/lens[i]: the bytes of FASTA files, taken in the order given.  Lines end at "\n", "\r\n" or a lone
 *             "\r" and are stripped of blanks (Python's str.strip() on ASCII); a stripped line that starts with '>' is a
 *             header, its name the rest of the line; other lines are joined WITHOUT a change of case.  A line that is empty
 *             after the strip stops the reference with an IndexError: ISSL_E_FORMAT here, the message names the input and
 *             the line
 *   records   a record is finished by the next header and counts when no record of that name was finished before, in this
 *             input or an earlier one, or when it has no name but a sequence; the last record of every input counts
 *             whatever its name, and its name is not remembered.  Text ahead of the first header is a record with an
 *             empty name.  A record that does not count has no index; a header without sequence is a record of length 0.
 *             name = the stripped header line without '>', as the bytes stand in the file (issl_guides_record; valid until
 *             the set is closed, not terminated)
 *   match     forward, strand 0: seq[i..i+21) all in ACGT -- upper case only, soft-masked bases never match -- and
 *             seq[i+21] == seq[i+22] == 'G'; the guide is seq[i:i+23].  Reverse, strand 1: seq[i] == seq[i+1] == 'C' and
 *             seq[i+2..i+23) all in ACGT; the guide is the reverse complement of seq[i:i+23].  Overlapping matches all
 *             count, one start can match both ways, nothing straddles a record.  start = i for both strands, 0-based in the
 *             record's joined sequence; the reference's `end` is start + 23
 *   order     the reference meets the matches input by input, record by record, and in a record all forward matches by
 *             position, then all reverse matches by position
 *   guide set the distinct guides in the order they are first met; each with the record, start and strand of its first
 *             occurrence and `seen`, the number of its occurrences in the whole input.  seen == 1 is the reference's
 *             isUnique; a guide seen more often is the row the reference keeps with blanked coordinates and never scores
 *   guide23   base p of the guide at bits [2p, 2p + 2), A C G T = 0..3 (issl_encode_guides with seq_len 23).  The signature
 *             array beside the guides holds guide23 & (2^40 - 1), the packed guide[0:20]: what Crackling.py:747-752 sends to
 *             the scorer, ready for issl_score_device
 * Input without any match is an empty set (n_guides == 0, device pointers NULL), not an error.  More than 2^32 - 1 matches
 * in one call: ISSL_E_UNSUPPORTED, as the extraction refuses.  No device: ISSL_E_DEVICE (no CPU fallback); NULL arguments
 * and n_files <= 0: ISSL_E_ARG; *out is NULL after a failure.  The output is deterministic: the same bytes on every run.
 * ISSL_GUIDES_TIMING=1 (read when the call starts) prints one stderr line with the stage times and the counts.  One set is
 * used by one thread at a time. */
typedef struct issl_guide_set issl_guide_set; /* opaque; owns device and host memory */
typedef struct {
    uint64_t guide23;  /* packed 23-mer */
    uint64_t start;    /* 0-based start of the first occurrence inside its record */
    uint32_t record;   /* index of that record */
    uint32_t strand;   /* 0: forward pattern, 1: reverse pattern */
    uint32_t seen;     /* occurrences in the whole input */
    uint32_t reserved; /* 0 */
} issl_guide;          /* 32 bytes, no padding */

int issl_guides_extract(const char *const *files, const size_t *lens, int n_files, int device, issl_guide_set **out);
/* Same from files on disk, in the order given; a lone directory stands for the files in it, top level only, in REVERSE
 * sorted name order (ConfigManager.py:181-184).  A file that cannot be read: ISSL_E_IO. */
int issl_guides_extract_files(const char *const *paths, int n_paths, int device, issl_guide_set **out);
/* n_matches: all occurrences (the sum of `seen`); n_unique: guides with seen == 1. */
int issl_guides_info(const issl_guide_set *g, uint64_t *n_guides, uint64_t *n_unique, uint64_t *n_matches, uint64_t *n_records);
int issl_guides_record(const issl_guide_set *g, uint64_t r, const char **name, size_t *name_len, uint64_t *length);
/* What the reference's log prints per input (Crackling.py:254-258), counted during the extraction, where the sorted runs
 * of equal guides still exist: input `file` in the order the inputs were read (a directory's files as they were expanded).
 * The running figures of the log are sums over the inputs so far: distinct guides = the sum of first_seen, guides that are
 * not unique (seen twice or more) = the sum of second_seen.  An input beyond the last: ISSL_E_ARG. */
typedef struct {
    uint32_t identified;  /* matches of this input */
    uint32_t duplicates;  /* those of them that met a guide seen before, in this input or an earlier one */
    uint32_t second_seen; /* guides whose second occurrence lies in this input */
    uint32_t first_seen;  /* guides whose first occurrence lies in this input */
} issl_guides_file;       /* 16 bytes */
int issl_guides_file_counts(const issl_guide_set *g, uint64_t file, issl_guides_file *out);
/* The number of inputs the set was extracted from (a directory counts by its files). */
int issl_guides_files(const issl_guide_set *g, uint64_t *n_files);
/* The guides to host memory, first-seen order; cap < n_guides: ISSL_E_ARG. */
int issl_guides_copy(const issl_guide_set *g, issl_guide *out, size_t cap);
/* The guides and their signatures in the memory of the set's device, n_guides each, valid until the set is closed. */
int issl_guides_device(const issl_guide_set *g, const issl_guide **d_guides, const uint64_t **d_sigs);
int issl_guides_close(issl_guide_set *g);

/* ---- efficiency consensus: G20, the mm10db filters, sgRNAScorer2 ------------------------------------------------------ */
/* Counterpart of src/crackling/Crackling.py:306-598 with the filter of :36-149, on the rows of a guide set, in place on the
 * set's device; no guide is copied to the host and there is no CPU fallback.  The set must stay open while the consensus is.
 *   filter    every step looks only at the guides filterCandidateGuides yields at that point, for the optimisation level,
 *             n and the tool flags given; passedBowtie is untested here and rejects nothing
 *   begin     G20 (:310-323), leading T (:328-343), AT percent (:348-366) and TTTT (:371-384), in that order; at =
 *             100.0 * count / 20.0 in double over guide[0:20]; the fold list = the rows the reference would write to
 *             RNAfold's input (:406-422), ascending.  Without mm10db the list is empty
 *   folds     RNAfold is not part of this library.  The caller folds "G" + guide[1:20] + the scaffold of :395 for every row of
 *             the list and hands back, per row and in the list's order, the energy, whether the structure matches the pattern
 *             of :396, and present = 0 where RNAfold's output has no entry under the key guide[1:20] (the reference looks the
 *             entry up by that key, the last one wins: :439-470)
 *   finish    once: ss by :476-498 -- error for a guide that starts with T, which the filter lets through only at ultralow and
 *             low; with the scaffold matched rejected when energy < low_energy, otherwise rejected when energy <=
 *             high_energy; present == 0 leaves it untested -- then for all rows the mm10db verdict (:518-530: an untested or
 *             erred sub-test rejects), the sgRNAScorer2 score and verdict for the rows the filter yields (:541-577), the
 *             count (:586-591) and the selection: the rows the filter yields for the specificity stage, ascending -- what
 *             goes to issl_score_device
 *   score     exact.  onehot sets for position p the bits 4p .. 4p + 3 of the reference's encoding, string index 0 first:
 *             A 0001, C 0010, T 0100, G 1000.  k_i = popcount(sv_i & onehot); score = -((((0.0 + coef[0] * k_0) + coef[1] * k_1)
 *             ... + coef[n_sv - 1] * k_(n_sv - 1)) + intercept), every product and sum rounded to double on its own: libsvm's
 *             sum for a linear kernel over 0 / 1 support vectors and sklearn's change of sign.  Rejected when score <
 *             sgrna_threshold
 * Errors: ISSL_E_ARG for a NULL pointer, optimisation > 3, sgrnascorer2 != 0 with n_sv == 0, n_folds that differs from the
 * fold list and cap below what is copied; ISSL_E_UNSUPPORTED for a support-vector entry other than 0 or 1; ISSL_E_STATE for a
 * second finish and for copy / device ahead of finish.  An empty set gives empty results.  The output is deterministic:
 * the same bytes on every run.  One consensus is used by one thread at a time. */
typedef struct issl_consensus issl_consensus; /* opaque; owns device memory */
typedef struct {
    uint32_t optimisation;                   /* 0 ultralow, 1 low, 2 medium, 3 high ([general] optimisation) */
    uint32_t n;                              /* [consensus] n */
    uint32_t mm10db, chopchop, sgrnascorer2; /* 0 / 1: the tools in the consensus */
    uint32_t n_sv;                           /* support vectors of the sgRNAScorer2 model */
    const uint8_t *sv;                       /* n_sv x 80, row-major, every entry 0 or 1 */
    const double *coef;                      /* n_sv: sklearn's _dual_coef_[0] */
    double intercept;                        /* sklearn's _intercept_[0] */
    double sgrna_threshold;                  /* [sgrnascorer2] score-threshold */
    double low_energy, high_energy;          /* [rnafold] low_energy_threshold, high_energy_threshold */
} issl_consensus_config;
typedef struct {
    double energy;     /* the number in the last parentheses of RNAfold's structure line */
    uint32_t scaffold; /* 1: the structure matches the pattern of :396 */
    uint32_t present;  /* 0: no entry for this guide */
} issl_fold;           /* 16 bytes */
typedef struct {
    double sgrna_score, at, ss_energy; /* NaN where the reference leaves '?' */
    uint8_t g20, lead_t, at_pct, tttt, ss, mm10db, sgrna; /* 0 rejected, 1 accepted, 2 untested '?', 3 error '!' */
    uint8_t count;                     /* consensusCount, 0..3 */
} issl_consensus_row;                  /* 32 bytes, no padding */

int issl_consensus_begin(const issl_guide_set *gs, const issl_consensus_config *cfg, issl_consensus **out);
/* The fold list in the memory of the set's device (NULL when it is empty), valid until the consensus is closed. */
int issl_consensus_fold_list(const issl_consensus *c, const uint32_t **d_rows, uint64_t *n_fold);
/* The fold list to host memory; cap below its length: ISSL_E_ARG. */
int issl_consensus_fold_copy(const issl_consensus *c, uint32_t *rows, size_t cap);
/* folds: host memory, n_folds = the length of the fold list, fold i belongs to row i of the list; NULL with 0. */
int issl_consensus_finish(issl_consensus *c, const issl_fold *folds, size_t n_folds);
/* The rows of all guides of the set to host memory; cap below their number: ISSL_E_ARG. */
int issl_consensus_copy(const issl_consensus *c, issl_consensus_row *out, size_t cap);
/* Rows and selection in the memory of the set's device (NULL where empty), valid until the consensus is closed. */
int issl_consensus_device(const issl_consensus *c, const issl_consensus_row **d_rows, const uint32_t **d_selected,
                          uint64_t *n_selected);
/* The reference's pages of the Bowtie step for a run in batches, made on the device from the selection where it lies: a
 * batch is batch_size consecutive rows of the set ([input] batch-size; Batchinator.py records every distinct guide once, in
 * first-seen order; 0: one batch), and every batch cuts its selected rows into pages of page_length ([bowtie2] page-length;
 * 0: one page per batch that has a selected row).  *d_page_starts: *n_pages + 1 boundaries in positions of the selection,
 * for issl_genome_occurrences_paged_device: device memory owned by the consensus, valid until the next such call or close.
 * No page is empty; an empty selection gives 0 pages and the one boundary 0.  ISSL_E_STATE before finish.  The host waits
 * once, for *n_pages. */
int issl_consensus_selection_pages(issl_consensus *c, uint64_t batch_size, uint64_t page_length, const uint64_t **d_page_starts,
                                   uint64_t *n_pages);
int issl_consensus_close(issl_consensus *c);

/* ---- transcript hit counts: how many transcripts of its gene a located guide cuts ------------------------------------ */
/* Counterpart of src/crackling/utils/countHitTranscripts.py (loadAnnotation :45-146, countTranscripts :148-193, process
 * :197-243): a GFF3 annotation is parsed on the host and resolved on `device` into one answer per elementary segment of
 * every sequence; a query is then a binary search.  No CPU fallback.  The reference's rules, quirks included:
 *   lines       end at "\n", "\r\n" or a lone "\r"; a line is split on TAB and every field stripped (Python's str.strip() on
 *               ASCII; bytes above 127 pass through as they stand, where Python decodes them first).  A line that does not
 *               give exactly 9 fields is skipped: comments and blank lines among them
 *   names       every '.' of the sequence name becomes '_'; the name a QUERY gives is not changed
 *   attributes  split on ';'; key = the text ahead of the first '=', value = the text between the first and the second;
 *               keys are not stripped, a later key overrides an earlier one.  An attribute without '=' -- a trailing ';'
 *               or an empty column is one -- stops the reference on a line of any type: ISSL_E_FORMAT
 *   counted     a line counts when it has both ID and Parent and its type is gene, mRNA or exon (a usual gene line has no
 *               Parent and is skipped).  Sequences are listed in the order they first appear on a counted line
 *   transcripts of a sequence, in the order they first appear on it: an mRNA line (its ID) or an exon line (its Parent).  The
 *               same ID on two sequences is two transcripts.  A transcript's ordinal counts first appearances over the whole
 *               file, so the transcripts of one sequence keep the reference's order
 *   genes       a transcript's gene is the Parent of the FIRST mRNA line anywhere in the file with its ID; a gene's total
 *               counts every mRNA line with that Parent, duplicates included
 *   exons       an exon adds (int(start), int(end)) to its transcript: an optional sign and ASCII digits within int64 here,
 *               anything else is ISSL_E_FORMAT (Python's int() also takes blanks, underscores, other digits and any size).
 *               start > end contains nothing
 *   query       (sequence, start): a transcript is hit when one of its exons has start <= q <= end, and counts once.  No
 *               hit, a sequence the annotation lacks ('*' is a name like any other) and a negative start: 0/0.  When the hit
 *               transcripts that have a gene name more than one, the reference raises: '?/?' (status 2).  Otherwise the
 *               gene is that of the FIRST hit transcript in the sequence's order; when that one never had an mRNA line the
 *               reference gets a KeyError: '?/?' (status 3).  Otherwise hit / the gene's total, hit counting the transcripts
 *               without an mRNA line too: 2/1 is possible
 * Bounds: exon coordinates that can contain a position >= 0 lie in [0, 2^40 - 2] after a negative start is raised to 0 and
 * an exon that ends below 0 is dropped; fewer than 2^24 sequences; at most 2^32 - 1 (segment, transcript) pairs while the
 * answers are built.  Beyond: ISSL_E_UNSUPPORTED.  The reference writes <annotation>.p beside the GFF; nothing is written here.
 * Errors: parsing comes before any device call, so a malformed file is ISSL_E_FORMAT with or without a GPU; then no device:
 * ISSL_E_DEVICE.  NULL arguments: ISSL_E_ARG; n == 0: ISSL_OK, nothing is written; *out is NULL after a failed open.  An
 * annotation without a counted line is valid and answers 0/0 everywhere.  The output is deterministic: the same bytes on
 * every run.  One annotation is used by one thread at a time. */
typedef struct issl_annotation issl_annotation; /* opaque; owns device and host memory */
typedef struct { uint32_t hit, total, status, first; } issl_transcript_hits; /* 16 bytes */
/* status 0: hit/total as counted (0/0 included); 1: untested row ('?/?'); 2: more than one gene ('?/?');
   3: first hit transcript has no mRNA line ('?/?').  first: ordinal of the first hit transcript among all
   transcripts of the annotation, 0xFFFFFFFF when none.  hit is filled for status 2 and 3 too; total is 0 there. */
int issl_annotation_open(const char *gff, size_t len, int device, issl_annotation **out);
/* Same from a file on disk; a file that cannot be read: ISSL_E_IO. */
int issl_annotation_open_file(const char *path, int device, issl_annotation **out);
/* n_exons: exon lines counted; n_segments: the stretches between neighbouring breakpoints of a sequence, summed over the
 * sequences -- a breakpoint is a start or an end + 1 of a transcript's exons, joined first where they overlap. */
int issl_annotation_info(const issl_annotation *a, uint64_t *n_seqs, uint64_t *n_transcripts, uint64_t *n_genes,
                         uint64_t *n_exons, uint64_t *n_segments);
/* Name of sequence k, '.' already replaced; valid until the annotation is closed, not terminated. */
int issl_annotation_seq(const issl_annotation *a, uint64_t k, const char **name, size_t *name_len);
int issl_annotation_lookup(const issl_annotation *a, const char *name, size_t name_len, uint32_t *seq); /* 0xFFFFFFFF: absent; the name is NOT '.'->'_' translated */
/* seq[i]: index from issl_annotation_lookup (0xFFFFFFFF or any index the annotation lacks: 0/0); start[i]: bowtieStart.
 * Host memory.  Blocking. */
int issl_annotation_hits(issl_annotation *a, const uint32_t *seq, const int64_t *start, size_t n, issl_transcript_hits *out);
/* Same with all arrays in the memory of the annotation's device, enqueued on `stream` (may be NULL); the call does not wait. */
int issl_annotation_hits_device(issl_annotation *a, const uint32_t *d_seq, const int64_t *d_start, size_t n,
                                issl_transcript_hits *d_out, void *stream);
/* The rows of issl_genome_occurrences_device as they lie in device memory: code == 2 is an untested row (status 1).
 * Otherwise the row is asked as the reference prints it: a record's name up to the first blank, as Bowtie2 names it, with
 * start = pos + 1; for record 0xFFFFFFFF -- the guide's read 0 does not occur -- the name '*' with start 0 ('*', 0, 22 in
 * Crackling's output), which hits only when the annotation has a sequence called '*'.  The genome must be on the
 * annotation's device.  Returns when the answers are written.
 * ISSL_ANNOTATION_TIMING=1 (read by issl_annotation_open*): one stderr line per open with the host clock around the parse,
 * the interval merge and the device build, which ends in a synchronise. */
int issl_annotation_hits_occurrences_device(issl_annotation *a, const issl_genome *g, const issl_occurrence *d_rows,
                                            size_t n, issl_transcript_hits *d_out, void *stream);
int issl_annotation_close(issl_annotation *a);

/* ---- off-target landings: where a guide's off-targets lie, and what they cut ------------------------------------------- */
/* The off-target report, the genome handle and the annotation joined on the device.  A LANDING is one occurrence in the
 * genome of one off-target of one guide: an issl_offtarget record of the guide, one issl_location of that record's site,
 * and the transcript answer at that location -- exactly what issl_annotation_hits returns for (name, pos + 1), name being
 * the record's header from its first non-blank character up to the next blank (the rule of
 * issl_annotation_hits_occurrences_device; not '.'->'_' translated).  Without an annotation (NULL) the answer is
 * {0, 0, 1, 0xFFFFFFFF}: status 1, untested.
 *   order     guides in batch order; inside a guide its off-targets in record order (the reference's scoring order, as
 *             issl_offtargets lists them); inside an off-target its landings sorted by (record, pos, strand), as
 *             issl_genome_locate lists them.  A site named by several records gets its list under each of them.  An
 *             off-target that does not occur in this genome (index and genome from different inputs) has no landing
 *   capacity  guide i owns out[offsets[i] .. offsets[i + 1]).  offsets (n + 1 words) and *n_total are always complete; when
 *             *n_total > cap NO row is written and the call still returns ISSL_OK (out == NULL with cap == 0 is the
 *             counting call) -- the rules of issl_offtargets and issl_genome_locate
 *   pieces    the host calls take any n and cut the batch as issl_offtargets does; a piece of more than 2^22 records is
 *             located in pieces of 2^22 sites.  At most one piece of records and landings is on the device at a time.  The
 *             device calls take one batch
 *   errors    NULL arguments: ISSL_E_ARG.  max_dist outside 0..6: ISSL_E_ARG.  An index that is not uploaded:
 *             ISSL_E_STATE, as issl_offtargets.  The handles not on one device: ISSL_E_ARG, the message names the devices.
 *             More than 2^32 - 1 landings in a call: ISSL_E_UNSUPPORTED.  No device: ISSL_E_DEVICE.  n == 0: ISSL_OK with
 *             offsets[0] = 0
 * The output is deterministic: the same bytes on every run.  The handles are used by one thread at a time. */
typedef struct {
    uint64_t site;              /* the off-target's packed signature */
    uint64_t pos;               /* issl_location.pos */
    uint32_t record, strand;    /* issl_location.record / .strand */
    uint32_t guide;             /* index into the guide batch */
    uint32_t rank;              /* index of the off-target among the guide's records: recs[offsets[guide] + rank] of issl_offtargets */
    uint32_t id, occ;           /* issl_offtarget.id / .occ */
    uint16_t dist, slice;
    uint32_t pad;               /* 0 */
    issl_transcript_hits hits;
} issl_landing;                 /* 64 bytes, no padding */

/* Per guide and distance d <= max_dist; bins above max_dist are zero.  For the genome an index was built from,
 * located[d] == issl_profile.occurrences[d] and absent[d] == 0. */
typedef struct {
    uint64_t located[ISSL_PROFILE_BINS]; /* landings of off-targets at distance d */
    uint64_t in_exon[ISSL_PROFILE_BINS]; /* of them, those with hits.hit > 0 (any status); 0 without an annotation */
    uint32_t absent[ISSL_PROFILE_BINS];  /* off-target sites at distance d without a landing */
    uint32_t pad;                        /* 0 */
} issl_landing_profile;                  /* 144 bytes */

/* Guides, offsets and rows in host memory.  Blocking. */
int issl_offtarget_landings(issl_index *idx, issl_genome *g, issl_annotation *a /* may be NULL */, const uint64_t *guides, size_t n,
                            int max_dist, uint64_t *offsets /* n + 1 */, issl_landing *out, size_t cap, size_t *n_total);
/* Same with guides, offsets and rows in device memory, one batch, on `stream` (may be NULL); *n_total is host memory and
 * the call returns when the batch is done. */
int issl_offtarget_landings_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n,
                                   int max_dist, uint64_t *d_offsets, issl_landing *d_out, size_t cap, size_t *n_total, void *stream);
/* One profile per guide; no landing is materialised, on the host or on the device: every guide's landings are reduced
 * where the join would write them.  Blocking. */
int issl_offtarget_landing_profile(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *guides, size_t n,
                                   int max_dist, issl_landing_profile *out);
/* Same with guides and profiles in device memory, one batch, on `stream`; returns when it is done. */
int issl_offtarget_landing_profile_device(issl_index *idx, issl_genome *g, issl_annotation *a, const uint64_t *d_guides, size_t n,
                                          int max_dist, issl_landing_profile *d_out, void *stream);

/* ---- the result table: Crackling's output file from the resident stages ---------------------------------------------- */
/* Counterpart of src/crackling/Crackling.py:263-268 (the header row) and :842-852 (one CSV row of the 26 columns of
 * Constants.py:42-70 per candidate guide, csv.writer with dialect 'unix', QUOTE_MINIMAL, quote character '"'): the text is
 * written on the set's device -- every row measured, the lengths summed, every workgroup's rows assembled in LDS and stored as
 * one span -- and stays there; no CPU fallback.  The reference works through the guides in batches of [input] batch-size and
 * appends every batch's rows to the file.  A row's text does not know its batch: what a batch changes are the pages of the
 * Bowtie step and of RNAfold, which start again with every batch, and both come in through the arguments -- d_bowtie from
 * issl_genome_occurrences_paged_device over issl_consensus_selection_pages, the folds and ss spans read page by page
 * (crackling_amd.pipeline).  With [rnafold] page-length = 0 the reference tests no guide (Paginator.py:29-30 hands out the
 * filter's generator, Crackling.py:420 consumes it, :458 sees nothing): folds with present == 0 and spans without text say
 * that.  issl_results_build_rows writes a run of rows, so that the text can leave the device a batch at a time.  Not
 * modelled: the RNAfold and Bowtie2 programs themselves, delimiters beyond the five, a CPU fallback.
 *   rows       those of the guide set, in its order, behind the header row; lines end in "\n"
 *   seq .. isUnique   the 23-mer; for seen == 1 the record's header line (issl_guides_record), start, start + 23, '+' / '-'
 *              and 1, otherwise '-' four times and 0 (:292-303)
 *   codes      of issl_consensus_row: 0, 1, ? (untested), ! (error); consensusCount is the row's count; AT and
 *              sgrnascorer2score are '?' for NaN, otherwise the double as Python's repr prints it: the shortest decimal that
 *              reads back as the same double, fixed notation for 1e-4 <= |x| < 1e16 with at least one digit behind the point,
 *              otherwise d[.ddd]e+XX / e-XX with at least two exponent digits; -0.0, inf, -inf, nan
 *   ssL1, ssStructure, ssEnergy   text, not numbers (:469-474): three spans of `ss_text` per row of the consensus' fold list,
 *              in its order; length UINT32_MAX leaves '?'; ss_spans == NULL leaves '?' everywhere
 *   bowtie     passedBowtie, bowtieChr, bowtieStart, bowtieEnd from issl_occurrence rows aligned with the consensus'
 *              selection: '?' four times for a row outside it, for code 2 and when d_bowtie is NULL; the code, '*', 0, 22
 *              without a record; otherwise the code, the genome record's name up to its first blank (space, TAB, LF, VT, FF,
 *              CR), pos + 1, pos + 23
 *   scores     mitOfftargetscore, cfdOfftargetscore, passedOffTargetScore for the rows d_scored lists (ascending row
 *              indices of the set), '?' for the others and when d_scored is NULL.  A score goes through the scorer's text as
 *              in the reference (:785-786): R = float("%f" % x), exactly (round(x * 10^6) ties to even on the binary value,
 *              one IEEE division by 10^6; x in [0, 2^32), anything else is taken as it is), printed as repr(R); a score
 *              `method` does not ask for is -1.0 (matched exactly as the scorer does: "AND" prints -1.0 twice); the verdict
 *              applies :794-835 to R under the lower-cased, stripped method, and stays '?' when that names no rule
 *   quoting    header, bowtieChr and the three ss columns are quoted when they contain the delimiter, '"', LF or CR, an
 *              embedded '"' doubled.  Delimiters: ',', TAB, ';', '|' and ' ' -- none of which a number or a code contains;
 *              any other: ISSL_E_UNSUPPORTED
 * Errors: ISSL_E_ARG for NULL pointers, spans outside ss_text, n_folds / n_bowtie that differ from the fold list / the
 * selection, n_scored above the number of guides, d_bowtie without a genome (or one on another device) and d_scored without both
 * scores, all before any device call; ISSL_E_STATE for an unfinished consensus; ISSL_E_DEVICE without a device.  An empty set
 * gives the header row only.  The output is deterministic: the same bytes on every run.  The guide set, the consensus and the
 * arrays are read while the call runs and not kept. */
typedef struct issl_results issl_results; /* opaque; owns device memory */
typedef struct {
    uint64_t offset;   /* into ss_text */
    uint32_t length;   /* bytes; 0xFFFFFFFF: no text, the column keeps '?' */
    uint32_t reserved; /* 0 */
} issl_text_span;      /* 16 bytes */
enum {
    ISSL_RESULTS_DIRECT = 1,  /* every row is stored straight to global memory by its thread (the path rows larger than the
                                 staging buffer take); same bytes.  Tests and A/B */
    ISSL_RESULTS_NO_SGRNA = 2, /* sgrnascorer2score is '?' in every row: the A/B that prices its repr (tools/bench_results.py) */
    ISSL_RESULTS_NO_HEADER = 4 /* the text starts with its first row: no header row, d_offsets[0] == 0 */
};
typedef struct {
    char delimiter;     /* [output] delimiter */
    uint32_t flags;     /* ISSL_RESULTS_* */
    const char *method; /* [offtargetscore] method as configured */
    double threshold;   /* [offtargetscore] score-threshold */
} issl_results_config;

int issl_results_build(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                       const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                       const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                       size_t n_scored, const issl_results_config *cfg, issl_results **out);
/* The same for rows [first_row, first_row + n_rows) of the set: the header row (unless ISSL_RESULTS_NO_HEADER) and these
 * rows.  Every other argument keeps its meaning for the WHOLE set: d_bowtie is aligned with the whole selection, d_scored
 * lists rows of the whole set, the spans belong to the whole fold list.  The header row, or a build with n_rows == 0, followed
 * by ISSL_RESULTS_NO_HEADER builds of consecutive ranges that cover the set is byte for byte the text of issl_results_build;
 * row k of the text is row first_row + k of the set (issl_results_info, issl_results_device).  A range that does not lie in
 * the set: ISSL_E_ARG.  An empty range gives the header row, or no byte with the flag. */
int issl_results_build_rows(const issl_guide_set *gs, const issl_consensus *c, const char *ss_text, size_t ss_len,
                            const issl_text_span *ss_spans, size_t n_folds, const issl_occurrence *d_bowtie, size_t n_bowtie,
                            const issl_genome *genome, const uint32_t *d_scored, const double *d_mit, const double *d_cfd,
                            size_t n_scored, uint64_t first_row, uint64_t n_rows, const issl_results_config *cfg,
                            issl_results **out);
/* n_rows: the guides (the header row is not counted); n_bytes: the whole text; rows_per_group: the rows one workgroup
 * assembles (a property of the build, for tests that place sizes around it).  Any output may be NULL. */
int issl_results_info(const issl_results *r, uint64_t *n_rows, uint64_t *n_bytes, uint32_t *rows_per_group);
/* Device time of the build's three launches in milliseconds, by HIP events on their stream (0 for an empty set): the
 * measuring kernel, the scan of the workgroups' sums, the emitting kernel.  Any output may be NULL. */
int issl_results_times(const issl_results *r, double *ms_measure, double *ms_scan, double *ms_emit);
/* The text and the n_rows + 1 row offsets in device memory, valid until close: row k is d_text[d_offsets[k] ..
 * d_offsets[k + 1]), d_offsets[0] is the length of the header row, d_offsets[n_rows] == n_bytes. */
int issl_results_device(const issl_results *r, const char **d_text, const uint64_t **d_offsets);
/* The text to host memory; cap below n_bytes: ISSL_E_ARG. */
int issl_results_copy(const issl_results *r, char *out, size_t cap);
/* The text into the file at `path`, appended when append != 0 (the reference opens its file "a+"); ISSL_E_IO. */
int issl_results_write(const issl_results *r, const char *path, int append);
int issl_results_close(issl_results *r);
/* repr() of n doubles in device memory: value i into d_text[32 i .. 32 i + d_len[i]), the rest of its 32 bytes zero (a repr
 * has at most 24 characters).  Enqueued on `stream` (may be NULL) on the current device; the call does not wait. */
int issl_repr_f64_device(const double *d_values, size_t n, char *d_text, uint32_t *d_len, void *stream);

/* ---- RNAfold's exchange: its input written, its answers read, on the device ------------------------------------------ */
/* Counterpart of src/crackling/Crackling.py:406-497 around the RNAfold program, which stays outside this library: the line
 * written per guide (:421), the dictionary of line pairs (:439-455), the lookup by guide[1:20] (:458-467), the three text
 * columns (:469-474), the two regular expressions of :396-397 and the number behind them (:481-497).  An issl_folds belongs
 * to one consensus and holds, for every row of its fold list, one issl_fold and the three spans ssL1, ssStructure, ssEnergy,
 * in device memory, where issl_consensus_finish_folds and issl_results_build_rows_folds read them.  A C caller runs
 *     issl_folds_input_write(f, first, n, "in");   RNAfold --noPS -jN -i in -o out;   issl_folds_read_file(f, first, n, "out");
 * once per page; RNAfold's two files are the only host-side text of a run.
 *   input     row r of the fold list is the 101 bytes 'G' + guide[1:20] + the 80 characters of the scaffold (:395) + LF
 *   pages     a page is a run [first, first + n) of the fold list read with its own text: the reference builds one dictionary
 *             per page (:439), so a pair that stands only in another page's text is not found.  Rows never read keep
 *             present == 0 and no text ([rnafold] page-length = 0 reads nothing).  Reading a row twice: ISSL_E_STATE.  A read
 *             that fails keeps nothing, and its rows can be read again
 *   lines     as the reference's text-mode file gives them: a line ends at LF, at CR LF (once) or at a lone CR, and at nothing
 *             else (str.splitlines(), which the package's Python helpers use, also splits at VT, FF and 0x1C-0x1E).  Empty
 *             lines count; a last line without terminator counts when it is not empty.  Lines 2p and 2p + 1 are pair p; a
 *             last line without partner is dropped.  A page may have any number of lines
 *   strip     rstrip() removes trailing bytes of {0x09-0x0D, 0x1C-0x1F, 0x20}; \s is the same set; bytes >= 0x80 are ordinary
 *   key       bytes [1, 20) of the stripped first line, U read as T; a key shorter than that or with a byte outside ACGT
 *             matches no guide.  Among pairs with one key the last one in the text wins
 *   texts     ssL1: the stripped first line.  ssStructure: the stripped second line up to its first 0x20.  ssEnergy: the
 *             word between the first and the second 0x20 (or the line's end) without its first and last byte, empty (length
 *             0, not '?') for a word of fewer than 3 bytes.  A second line without 0x20, for a pair a guide of the page
 *             looks up: ISSL_E_FORMAT (IndexError in the reference)
 *   :396      with z the last ')' of the stripped second line: the leftmost s with bytes [s + 28, s + 47) equal to
 *             "((((....))))...))))", [s + 68, s + 100) equal to "((((....))))(((((((...)))))))...", byte s + 100 in \s, byte
 *             s + 101 '(' and z >= s + 103; the number is [s + 102, z) and scaffold = 1
 *   :397      otherwise the leftmost p with byte p in \s, byte p + 1 '(' and z >= p + 3; the number is [p + 2, z).  With
 *             neither the row keeps present == 0 (all 16 bytes zero) and its three texts
 *   number    blanks and TABs around it, an optional sign, digits[.digits] or .digits with at least one digit; the value is
 *             the digit string as an integer divided by 10^(fraction digits), one IEEE division: correctly rounded for up to
 *             15 digits (leading zeros of the integer part not counted); more: ISSL_E_UNSUPPORTED.  Anything else -- an
 *             exponent, an underscore, inf, a blank behind the sign -- is ISSL_E_FORMAT.  Only pairs a guide of the page
 *             looks up are judged, as in the reference; the message names the lowest refused row of the fold list
 * Memory: the pages' text stays on the device until issl_folds_close, for the spans to point into: about 211 bytes per
 * folded guide (RNAfold's two lines), next to the 64 bytes of its fold and spans.  A line of 2^32 - 1 bytes or more in a
 * looked-up pair: ISSL_E_UNSUPPORTED.  ISSL_E_ARG for NULL pointers, a range outside the fold list, a cap that is too small
 * and folds of another consensus; ISSL_E_IO for a file.  The output is deterministic.  The consensus must outlive the
 * folds; one issl_folds is used by one thread at a time.  The host waits once per read. */
typedef struct issl_folds issl_folds; /* RNAfold's answers for the fold list of one consensus; owns device memory */
int issl_folds_open(const issl_consensus *c, issl_folds **out);
/* n_fold: rows of the fold list; n_read: rows read so far; text_bytes: bytes of the pages' text kept; bytes_per_group: the
 * bytes whose line ends one thread marks (for tests that place line ends around it).  Any output may be NULL. */
int issl_folds_info(const issl_folds *f, uint64_t *n_fold, uint64_t *n_read, uint64_t *text_bytes, uint32_t *bytes_per_group);
/* Device time of the last input and the last read in milliseconds, by HIP events on their stream. */
int issl_folds_times(const issl_folds *f, double *ms_input, double *ms_read);
/* RNAfold's input for rows [first, first + n) of the fold list (:421) in device memory, *n_bytes = 101 n; valid until the
 * next input call on this object or close. */
int issl_folds_input(issl_folds *f, uint64_t first, uint64_t n, const char **d_text, uint64_t *n_bytes);
int issl_folds_input_copy(issl_folds *f, uint64_t first, uint64_t n, char *out, size_t cap);
/* The same into the file at `path`, created or truncated (the reference opens it 'w+'). */
int issl_folds_input_write(issl_folds *f, uint64_t first, uint64_t n, const char *path);
/* One page: what RNAfold printed for (a superset of) rows [first, first + n), len bytes of host memory. */
int issl_folds_read(issl_folds *f, uint64_t first, uint64_t n, const char *text, size_t len);
int issl_folds_read_file(issl_folds *f, uint64_t first, uint64_t n, const char *path);
/* n_fold folds and 3 n_fold spans in device memory (NULL for an empty list), valid until close.  A span's offset counts
 * from *d_text of issl_folds_text_device, whose pointer is valid until the next read; its `reserved` word is the library's
 * own: which of ',' TAB ';' '|' ' ' (bits 0 .. 4) and of '"', CR, LF (bit 5) the text holds, for the table's quoting. */
int issl_folds_device(const issl_folds *f, const issl_fold **d_folds, const issl_text_span **d_spans);
int issl_folds_text_device(const issl_folds *f, const char **d_text, uint64_t *n_bytes);
/* To host memory; cap: rows there is room for; folds or spans may be NULL. */
int issl_folds_copy(const issl_folds *f, issl_fold *folds, issl_text_span *spans, size_t cap);
/* Column `which` (0 ssL1, 1 ssStructure, 2 ssEnergy) of one row to host memory: *len its bytes, (size_t)-1 for a column
 * without text.  For tests and small callers: one copy from the device per call. */
int issl_folds_text_copy(const issl_folds *f, uint64_t fold_row, int which, char *out, size_t cap, size_t *len);
int issl_folds_close(issl_folds *f);
/* issl_consensus_finish with the folds where they lie; ISSL_E_STATE as there. */
int issl_consensus_finish_folds(issl_consensus *c, const issl_folds *f);
/* issl_results_build_rows with the three ss columns from f's spans and text; the fields are quoted on the device, the same
 * bytes as issl_results_build_rows gives for the same texts. */
int issl_results_build_rows_folds(const issl_guide_set *gs, const issl_consensus *c, const issl_folds *f,
                                  const issl_occurrence *d_bowtie, size_t n_bowtie, const issl_genome *genome,
                                  const uint32_t *d_scored, const double *d_mit, const double *d_cfd, size_t n_scored,
                                  uint64_t first_row, uint64_t n_rows, const issl_results_config *cfg, issl_results **out);

/* ---- the run's log: what every batch's stages saw and failed ---------------------------------------------------------- */
/* Counterpart of the figures src/crackling/Crackling.py:305-598 and :727-837 print into the run's log, counted on the device
 * over the rows the stages left there; nothing per row crosses to the host and there is no CPU fallback.  (The name is not
 * issl_stats: that is the scorer's.)  A batch is batch_size consecutive rows of the guide set ([input] batch-size; 0, or a
 * size of at least the set: one batch); an empty set has no batch.  Per batch, with the codes of issl_consensus_row
 * (0 rejected, 1 accepted, 2 untested, 3 error):
 *   loaded      (:305) rows of the batch
 *   g20, lead_t, at, tttt   (:310-384) tested = rows whose code is 0 or 1, failed = code 0
 *   ss          (:390-507) over the batch's rows of the fold list: tested = code 0 or 1, failed = code 0, erred = code 3,
 *               not_found = rows without an answer: present == 0 in the folds, or code 2 when no folds are given (the
 *               consensus leaves exactly the rows with present == 0 untested).  The not-found rows of all batches, as
 *               positions in the fold list, ascending, are kept as well (the reference prints a line for each)
 *   mm10db      (:513-534) accepted = code 1, failed = every other row of the batch
 *   sgrna       (:541-577) tested = code 0 or 1, failed = code 0
 *   consensus   (:582-598) tested = rows of the batch, failed = count < [consensus] n
 *   positions   fold, selected, scored: the batch's share [first, end) of the fold list, of the selection and of d_scored
 *               -- all three ascending row lists -- from which the host derives every page's number of guides
 *   bowtie_rejected   rows of the batch's share of the selection whose issl_occurrence ends with code 0 (0 without d_bowtie).
 *               NOT the Bowtie step's `failed` figure (:709-717), which counts events, not rows
 *   pages       (:727-837) the batch's scored rows in pages of offtarget_page_length ([offtargetscore] page-length): pages
 *               [page_first, page_end) of the page array; page_failed[p] = rows of page p that `method` and `threshold`
 *               reject, by the rule of issl_verdicts on the scores read through the scorer's "%f" text.  A page length of 0
 *               is one page per batch, also for a batch without a scored row; above 0 a batch without one has no page
 *               (Paginator.py).  A method that names no rule rejects nothing
 * Every count is an integer sum: the result is the same on every run.  d_bowtie (aligned with the selection, may be NULL
 * with n_bowtie == 0), d_scored, d_mit, d_cfd (n_scored each; all NULL with 0) are device memory on the consensus' device
 * and must be complete when the call is made; the call returns when the counts are.  f may be NULL.
 * Errors: ISSL_E_ARG for NULL c, method or out, folds of another consensus, n_bowtie that differs from the selection,
 * d_scored without both scores and n_scored above the number of guides; ISSL_E_STATE for an unfinished consensus;
 * ISSL_E_DEVICE without a device; *out is NULL after a failure. */
typedef struct issl_runlog issl_runlog; /* opaque; owns device memory */
typedef struct {
    uint32_t loaded;
    uint32_t g20_tested, g20_failed, lead_t_tested, lead_t_failed, at_tested, at_failed, tttt_tested, tttt_failed;
    uint32_t ss_tested, ss_failed, ss_erred, ss_not_found;
    uint32_t mm10db_accepted, mm10db_failed;
    uint32_t sgrna_tested, sgrna_failed;
    uint32_t consensus_tested, consensus_failed;
    uint32_t fold_first, fold_end, selected_first, selected_end, scored_first, scored_end;
    uint32_t page_first, page_end;
    uint32_t bowtie_rejected;
} issl_runlog_batch; /* 112 bytes, no padding */

int issl_runlog_batches(const issl_consensus *c, const issl_folds *f, const issl_occurrence *d_bowtie, size_t n_bowtie,
                        const uint32_t *d_scored, const double *d_mit, const double *d_cfd, size_t n_scored, double threshold,
                        const char *method, uint64_t batch_size, uint64_t offtarget_page_length, issl_runlog **out);
/* n_batches; n_pages: the off-target pages of all batches; n_not_found: fold-list rows without an answer; ms: device time
 * of the counting launches by HIP events on their stream.  Any output may be NULL. */
int issl_runlog_info(const issl_runlog *r, uint64_t *n_batches, uint64_t *n_pages, uint64_t *n_not_found, double *ms);
/* To host memory: every array that is not NULL is copied whole; its cap below the number there is: ISSL_E_ARG. */
int issl_runlog_copy(const issl_runlog *r, issl_runlog_batch *batches, size_t cap_batches, uint32_t *page_failed,
                     size_t cap_pages, uint32_t *not_found, size_t cap_not_found);
int issl_runlog_close(issl_runlog *r);

#ifdef __cplusplus
}
#endif
#endif /* ISSL_HIP_H */
