// RNAfold's exchange (issl_folds_*, include/issl_hip.h) as its units see each other: issl_folds.cpp keeps the handle, the
// pages' text and the files; issl_folds.hip writes RNAfold's input and reads its answers; issl_consensus.hip and
// issl_results.cpp take the folds and the spans where they lie.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/issl_hip.h"
#include "issl_hiputil.hpp"

namespace issl {

constexpr uint32_t kFoldGroupBytes = 64;  // bytes of text whose line ends one thread marks: four 16-byte loads
constexpr uint32_t kFoldLineBytes = 101;  // 'G', guide[1:20], the 80 characters of the scaffold, LF
constexpr uint64_t kFoldNoError = ~0ull;  // the error word: fold row << 8 | kind, the lowest one wins

// What the consensus lends (issl_consensus.hip): the set's rows, the fold list.
struct FoldSource {
    int device;
    const ulonglong2 *guides; // issl_guide as two 16-byte halves
    uint32_t n_guides;
    const uint32_t *fold_list;
    uint64_t n_fold;
};
FoldSource consensus_fold_source(const issl_consensus *c);

// Rows [first, first + n) of the fold list as lines of kFoldLineBytes into text (16-byte aligned, n * 101 bytes and the
// rest of the last 16).
void launch_folds_input(const FoldSource &src, uint64_t first, uint64_t n, char *text, hipStream_t stream);
// folds[first .. first + n) = 0, their spans without text.
void launch_folds_clear(issl_fold *folds, issl_text_span *spans, uint64_t first, uint64_t n, hipStream_t stream);

// One page's answer.  text: len bytes at a 16-byte aligned address with room up to the next multiple of
// kFoldGroupBytes; base: where the text lies in the arena the spans count from; last_line: where its last line starts.
// work: folds_read_work(n, len) bytes.  Rows [first, first + n) of folds and spans are written; *error (device memory)
// becomes the lowest refused row << 8 | kind, or stays kFoldNoError.  No wait; -> the first HIP error of its memsets and launches.
struct FoldRead {
    const uint8_t *text;
    uint64_t len, base, last_line;
    uint64_t first, n;
    issl_fold *folds;
    issl_text_span *spans;
    uint64_t *error;
    void *work;
};
size_t folds_read_work(uint64_t n, uint64_t len);
hipError_t launch_folds_read(const FoldSource &src, const FoldRead &r, hipStream_t stream);

} // namespace issl

struct issl_folds {
    const issl_consensus *consensus = nullptr;
    issl::FoldSource src{};
    issl::OwnedStream stream;           // ahead of the buffers: they are released first
    issl::DevBuf folds, spans, error;   // n_fold rows, 3 n_fold spans, the error word
    issl::DevBuf text;                  // the pages' text, one behind the other, each at a multiple of 16
    uint64_t text_cap = 0, text_used = 0, text_bytes = 0; // bytes allocated / taken (padded) / of the pages' own text
    issl::DevBuf input;                 // the lines of the last issl_folds_input
    std::vector<std::pair<uint64_t, uint64_t>> read; // the runs [first, end) of the list that were read, ascending
    uint64_t n_read = 0;
    float ms_input = 0, ms_read = 0;    // the last input / read by HIP events on the stream
};
