// statmc_select_args.h -- what statmc_score_select and statmc_score_count_above (include/statmc.h) check and fill on the host, each
// rule stated once, the key of a score, the workspace layout and the argument blocks their kernels take (statmc_select.hip).  Pure
// functions of their arguments: no HIP call, no device, no global or thread-local state; nothing is read through a device pointer
// (the image pointers are compared as numbers; `ranks` and `thresholds` are host arrays and are read).  true: valid; false: the
// caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  Host-only and on its own:
// tests/cpp/test_select_args.cpp compiles this header with nothing but include/statmc.h, with and without sanitizers.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/statmc.h"

namespace statmc {

// ---- the key: integer arithmetic on the bit pattern alone.  NaN of either sign and everything with the sign bit are key 0; for
// the rest (+0, subnormals, normals, +inf) the order of the bit patterns is the order of the values.
constexpr uint32_t select_key(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u || (b >> 31) ? 0u : b; }
constexpr uint32_t kSelectLiveLo = 0x21800000u, kSelectLiveHi = 0x5D800000u;   // 2^-60 and 2^60: statmc_plan_samples' classes, on keys
static_assert(select_key(0x80000000u) == 0 && select_key(0xFF800000u) == 0 && select_key(0x7FC00000u) == 0 && select_key(0xFFC00000u) == 0 &&
                  select_key(0x80000001u) == 0 && select_key(0x7F800000u) == 0x7F800000u && select_key(1u) == 1u,
              "-0, -inf, both NaN signs and a negative subnormal are key 0; +inf and the smallest subnormal are their own bits");

// ---- the search of statmc_score_select: a most-significant-digit radix select, kSelectPasses digits of
// kSelectDigitBits bits.  Pass 0 is one histogram of the top digit over all pixels; pass q >= 1 holds one histogram per DISTINCT
// prefix (the top q digits) among the ranks -- slot i belongs to rank i if no rank j < i has the same prefix -- over the pixels
// under that prefix.
constexpr int kSelectDigitBits = 8;
constexpr int kSelectBins = 1 << kSelectDigitBits;
constexpr int kSelectPasses = 32 / kSelectDigitBits;
static_assert(kSelectPasses * kSelectDigitBits == 32, "the digits cover the key");
static_assert(STATMC_SELECT_MAX_RANKS == 8, "slots are indexed by 3 bits (statmc_select.hip: kSelectIndexBits)");

constexpr int kSelectBlock = 256;                // 4 waves; one thread per bin when the histograms are flushed
constexpr int kSelectQuad = 4;                   // consecutive pixels per lane and step
constexpr int kSelectChunk = kSelectBlock * kSelectQuad;   // pixels per workgroup and step
constexpr int kSelectMaxGrid = 768;              // workgroups of a pass, as statmc_plan_samples': they stride over the chunks

// the workspace, in 64-bit words: pass 0's histogram, STATMC_SELECT_MAX_RANKS histograms for each later pass, the class counts
constexpr int kSelectHistograms = 1 + (kSelectPasses - 1) * STATMC_SELECT_MAX_RANKS;
enum { kSelectWsHist = 0, kSelectWsLive = kSelectHistograms * kSelectBins, kSelectWsSaturated, kSelectWsWords = kSelectWsLive + 8 };
constexpr int select_hist_word(int pass, int slot) {
    return kSelectWsHist + (pass == 0 ? 0 : 1 + (pass - 1) * STATMC_SELECT_MAX_RANKS + slot) * kSelectBins;
}
inline size_t select_workspace_bytes() { return (size_t)kSelectWsWords * sizeof(int64_t); }

struct SelectArgs {
    const float *score;
    statmc_select_result *result;
    long long *ws;
    long long n_px, n_chunks;
    long long rank[STATMC_SELECT_MAX_RANKS];
    int n_ranks;
    int grid;                    // workgroups of a pass
    int vec;                     // score 16-byte aligned: a lane's full quad moves as dwordx4
};

struct CountAboveArgs {
    const float *score;
    long long *counts;
    long long n_px, n_chunks;
    uint32_t key[STATMC_SELECT_MAX_RANKS];   // of the thresholds
    int n_thresholds;
    int grid;
    int vec;
};

struct SelectMsg { char *buf; size_t len; };   // the caller's buffer
__attribute__((format(printf, 2, 3))) inline bool select_refuse(SelectMsg m, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m.buf, m.len, fmt, ap);
    va_end(ap);
    return false;
}
inline bool select_misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool select_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}
inline uint32_t select_float_bits(float f) {
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    return b;
}

// statmc_score_select, in this order: the film size, NULL pointers, alignment, n_ranks, the ranks, the workspace size, result over
// the score image or the workspace, the workspace over the score image.
inline bool check_select_call(uint16_t width, uint16_t height, const float *score, const int64_t *ranks, int n_ranks,
                              const statmc_select_result *result, const void *workspace, size_t workspace_bytes, SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!result) return select_refuse(m, "null result");
    if (!ranks) return select_refuse(m, "null ranks");
    if (!workspace) return select_refuse(m, "null workspace");
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    if (select_misaligned(result, 8)) return select_refuse(m, "result is not 8-byte aligned");
    if (select_misaligned(workspace, 8)) return select_refuse(m, "workspace is not 8-byte aligned");
    if (n_ranks < 1 || n_ranks > STATMC_SELECT_MAX_RANKS) return select_refuse(m, "n_ranks = %d: 1 to %d", n_ranks, STATMC_SELECT_MAX_RANKS);
    const long long n_px = (long long)width * height;
    for (int i = 0; i < n_ranks; i++)
        if (ranks[i] < 0 || ranks[i] >= n_px)
            return select_refuse(m, "ranks[%d] = %lld: outside the film's 0 .. %lld", i, (long long)ranks[i], n_px - 1);
    const size_t need = select_workspace_bytes();
    if (workspace_bytes < need)
        return select_refuse(m, "workspace_bytes = %zu: statmc_score_select_workspace asks for %zu", workspace_bytes, need);
    const size_t px = (size_t)n_px * 4;
    if (select_ranges_overlap(result, sizeof(statmc_select_result), score, px)) return select_refuse(m, "result overlaps score");
    if (select_ranges_overlap(result, sizeof(statmc_select_result), workspace, need)) return select_refuse(m, "result overlaps workspace");
    if (select_ranges_overlap(workspace, need, score, px)) return select_refuse(m, "workspace overlaps score");
    return true;
}

inline long long select_chunks(uint16_t width, uint16_t height) { return ((long long)width * height + kSelectChunk - 1) / kSelectChunk; }

// The kernels' argument block of a call that passed check_select_call.
inline void fill_select_args(SelectArgs &a, uint16_t width, uint16_t height, const float *score, const int64_t *ranks, int n_ranks,
                             statmc_select_result *result, void *workspace) {
    a = SelectArgs{};
    a.score = score, a.result = result;
    a.ws = static_cast<long long *>(workspace);
    a.n_px = (long long)width * height;
    a.n_chunks = select_chunks(width, height);
    for (int i = 0; i < n_ranks; i++) a.rank[i] = ranks[i];
    a.n_ranks = n_ranks;
    a.grid = (int)(a.n_chunks < kSelectMaxGrid ? a.n_chunks : kSelectMaxGrid);
    a.vec = !select_misaligned(score, 16);
}

// statmc_score_count_above, in this order: the film size, NULL pointers, alignment, n_thresholds, NaN thresholds, counts over the
// score image.
inline bool check_count_above_call(uint16_t width, uint16_t height, const float *score, const float *thresholds, int n_thresholds,
                                   const int64_t *counts, SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!counts) return select_refuse(m, "null counts");
    if (!thresholds) return select_refuse(m, "null thresholds");
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    if (select_misaligned(counts, 8)) return select_refuse(m, "counts is not 8-byte aligned");
    if (n_thresholds < 1 || n_thresholds > STATMC_SELECT_MAX_RANKS)
        return select_refuse(m, "n_thresholds = %d: 1 to %d", n_thresholds, STATMC_SELECT_MAX_RANKS);
    for (int i = 0; i < n_thresholds; i++)
        if ((select_float_bits(thresholds[i]) & 0x7FFFFFFFu) > 0x7F800000u) return select_refuse(m, "thresholds[%d] is NaN", i);
    if (select_ranges_overlap(counts, (size_t)n_thresholds * sizeof(int64_t), score, (size_t)width * height * 4))
        return select_refuse(m, "counts overlaps score");
    return true;
}

inline void fill_count_above_args(CountAboveArgs &a, uint16_t width, uint16_t height, const float *score, const float *thresholds,
                                  int n_thresholds, int64_t *counts) {
    a = CountAboveArgs{};
    a.score = score;
    a.counts = reinterpret_cast<long long *>(counts);
    a.n_px = (long long)width * height;
    a.n_chunks = select_chunks(width, height);
    for (int i = 0; i < n_thresholds; i++) a.key[i] = select_key(select_float_bits(thresholds[i]));
    a.n_thresholds = n_thresholds;
    a.grid = (int)(a.n_chunks < kSelectMaxGrid ? a.n_chunks : kSelectMaxGrid);
    a.vec = !select_misaligned(score, 16);
}

}  // namespace statmc
