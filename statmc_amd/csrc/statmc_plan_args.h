// statmc_plan_args.h -- what statmc_sample_scores and statmc_plan_samples (include/statmc.h) check and fill on the host, each rule
// stated once, and the argument blocks their kernels take (statmc_plan.hip).  Pure functions of their arguments: no HIP call, no
// device, no global or thread-local state; nothing is read through a pointer (the image pointers are compared as numbers).  true:
// valid; false: the caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  Host-only and on its own:
// tests/cpp/test_plan_args.cpp compiles this header with nothing but include/statmc.h, with and without sanitizers.
#pragma once

#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"

namespace statmc {

// ---- the search of statmc_plan_samples.  A pass evaluates T at kPlanCandidates levels.  Pass 0's candidates are
// U_LO + j * 2^24, j = 0 .. 63: both ends of [U_LO, U_HI] included (U_HI - U_LO = 63 * 2^24), so it settles status 1 and 2 and leaves
// an interval (lo, hi] of 2^24 bit patterns with T(lo) < budget <= T(hi).  Pass q = 1 .. 4 cuts (lo, hi] into 64 parts of
// 2^(24 - 6 q) patterns, candidate j = lo + (j + 1) * 2^(24 - 6 q); after pass 4 hi = u* and lo = u* - 1.
constexpr int kPlanCandidates = 64;
constexpr int kPlanPasses = 5;
constexpr uint32_t kPlanLevelLo = 0x20000000u, kPlanLevelHi = 0x5F000000u;   // 2^-63 and 2^63
static_assert(kPlanLevelHi - kPlanLevelLo == (kPlanCandidates - 1u) << 24, "pass 0 spans the level range with both ends");
static_assert(24 - 6 * (kPlanPasses - 1) == 0, "the last pass steps by one bit pattern");
constexpr int32_t kPlanMaxCount = 1 << 20;     // c_max's bound
constexpr int32_t kPlanMaxTarget = 1 << 30;    // N's and n's clamp

constexpr int kPlanBlock = 256;                // 4 waves
constexpr int kPlanQuad = 4;                   // consecutive pixels per lane and step
constexpr int kPlanChunk = kPlanBlock * kPlanQuad;   // pixels per workgroup and step; the scan's block
constexpr int kPlanMaxGrid = 768;              // workgroups of a search pass: 3 per compute unit of a 256-CU device, all resident at
                                               // the pass kernel's 3 waves per SIMD; they stride over the chunks

// the workspace, in 64-bit words: the passes' totals, the class counts, then one word per scan block
enum { kPlanWsTotals = 0, kPlanWsLive = kPlanPasses * kPlanCandidates, kPlanWsSaturated, kPlanWsBlocks = kPlanWsLive + 8 };

inline long long plan_scan_blocks(uint16_t width, uint16_t height) {
    return ((long long)width * height + kPlanChunk - 1) / kPlanChunk;
}
inline size_t plan_workspace_bytes(uint16_t width, uint16_t height) {
    return ((size_t)kPlanWsBlocks + (size_t)plan_scan_blocks(width, height)) * sizeof(int64_t);
}

struct PlanArgs {
    const float *score;
    const int32_t *n;            // NULL: 0 everywhere
    int32_t *counts;
    statmc_plan_result *result;
    long long *ws;
    long long n_px, n_chunks, budget;
    int c_min, c_max;
    int grid;                    // workgroups of a search pass
    int wide;                    // a lane's partial sums need 64 bits: pixels per lane x c_max >= 2^31
    int wide_wave;               // a wave's sums need 64 bits: 64 x pixels per lane x c_max >= 2^31
    int vec;                     // score, n and counts 16-byte aligned: a lane's full quad moves as dwordx4
};

struct ScoreArgs {
    const int32_t *n;
    const float *film_mean, *film_m2;
    float *score;
    long long n_px;
    float eps;
    int channels, metric;
    int vec;                     // all four planes 16-byte aligned
};

struct PlanMsg { char *buf; size_t len; };   // the caller's buffer
__attribute__((format(printf, 2, 3))) inline bool plan_refuse(PlanMsg m, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m.buf, m.len, fmt, ap);
    va_end(ap);
    return false;
}
inline bool plan_misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool plan_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

// statmc_sample_scores, in this order: the film size, channels, metric, eps (relative metric only), NULL images, alignment, score
// over an image it is computed from.
inline bool check_scores_call(uint16_t width, uint16_t height, int channels, int metric, float eps, const int32_t *n, const float *film_mean,
                              const float *film_m2, const float *score, PlanMsg m) {
    if (width == 0 || height == 0) return plan_refuse(m, "empty image: width and height must be positive");
    if (channels != 1 && channels != 3) return plan_refuse(m, "channels = %d: must be 1 or 3", channels);
    if (metric != STATMC_SCORE_ABSOLUTE && metric != STATMC_SCORE_RELATIVE)
        return plan_refuse(m, "metric = %d: STATMC_SCORE_ABSOLUTE (0) or STATMC_SCORE_RELATIVE (1)", metric);
    if (metric == STATMC_SCORE_RELATIVE && !(eps > 0.f && eps <= 3.402823466e+38f)) return plan_refuse(m, "eps must be positive and finite");
    if (!n) return plan_refuse(m, "null n");
    if (!film_mean) return plan_refuse(m, "null film_mean");
    if (!film_m2) return plan_refuse(m, "null film_m2");
    if (!score) return plan_refuse(m, "null score");
    if (plan_misaligned(n, 4)) return plan_refuse(m, "n is not 4-byte aligned");
    if (plan_misaligned(film_mean, 4)) return plan_refuse(m, "film_mean is not 4-byte aligned");
    if (plan_misaligned(film_m2, 4)) return plan_refuse(m, "film_m2 is not 4-byte aligned");
    if (plan_misaligned(score, 4)) return plan_refuse(m, "score is not 4-byte aligned");
    const size_t px = (size_t)width * height * 4, img = px * (size_t)channels;
    if (plan_ranges_overlap(score, px, n, px)) return plan_refuse(m, "score overlaps n");
    if (plan_ranges_overlap(score, px, film_mean, img)) return plan_refuse(m, "score overlaps film_mean");
    if (plan_ranges_overlap(score, px, film_m2, img)) return plan_refuse(m, "score overlaps film_m2");
    return true;
}

inline void fill_score_args(ScoreArgs &a, uint16_t width, uint16_t height, int channels, int metric, float eps, const int32_t *n,
                            const float *film_mean, const float *film_m2, float *score) {
    a = ScoreArgs{};
    a.n = n, a.film_mean = film_mean, a.film_m2 = film_m2, a.score = score;
    a.n_px = (long long)width * height;
    a.eps = eps, a.channels = channels, a.metric = metric;
    a.vec = !plan_misaligned(n, 16) && !plan_misaligned(film_mean, 16) && !plan_misaligned(film_m2, 16) && !plan_misaligned(score, 16);
}

// statmc_plan_samples, in this order: the film size, NULL pointers, alignment, the bounds, the budget, the workspace size,
// sample_counts over an image the call reads, the result or the workspace.
inline bool check_plan_call(uint16_t width, uint16_t height, const float *score, const int32_t *n, int64_t budget, int32_t c_min, int32_t c_max,
                            const int32_t *sample_counts, const statmc_plan_result *result, const void *workspace, size_t workspace_bytes,
                            PlanMsg m) {
    if (width == 0 || height == 0) return plan_refuse(m, "empty image: width and height must be positive");
    if (!score) return plan_refuse(m, "null score");
    if (!sample_counts) return plan_refuse(m, "null sample_counts");
    if (!result) return plan_refuse(m, "null result");
    if (!workspace) return plan_refuse(m, "null workspace");
    if (plan_misaligned(score, 4)) return plan_refuse(m, "score is not 4-byte aligned");
    if (plan_misaligned(n, 4)) return plan_refuse(m, "n is not 4-byte aligned");
    if (plan_misaligned(sample_counts, 4)) return plan_refuse(m, "sample_counts is not 4-byte aligned");
    if (plan_misaligned(result, 8)) return plan_refuse(m, "result is not 8-byte aligned");
    if (plan_misaligned(workspace, 8)) return plan_refuse(m, "workspace is not 8-byte aligned");
    if (c_min < 0 || c_min > c_max || c_max > kPlanMaxCount)
        return plan_refuse(m, "c_min = %d, c_max = %d: 0 <= c_min <= c_max <= %d", (int)c_min, (int)c_max, (int)kPlanMaxCount);
    if (budget < 0) return plan_refuse(m, "budget = %lld: must not be negative", (long long)budget);
    const size_t need = plan_workspace_bytes(width, height);
    if (workspace_bytes < need) return plan_refuse(m, "workspace_bytes = %zu: statmc_plan_samples_workspace asks for %zu", workspace_bytes, need);
    const size_t px = (size_t)width * height * 4;
    if (plan_ranges_overlap(sample_counts, px, score, px)) return plan_refuse(m, "sample_counts overlaps score");
    if (plan_ranges_overlap(sample_counts, px, n, px)) return plan_refuse(m, "sample_counts overlaps n");
    if (plan_ranges_overlap(sample_counts, px, result, sizeof(statmc_plan_result))) return plan_refuse(m, "sample_counts overlaps result");
    if (plan_ranges_overlap(sample_counts, px, workspace, need)) return plan_refuse(m, "sample_counts overlaps workspace");
    if (plan_ranges_overlap(result, sizeof(statmc_plan_result), workspace, need)) return plan_refuse(m, "result overlaps workspace");
    return true;
}

// The kernels' argument block of a call that passed check_plan_call.
inline void fill_plan_args(PlanArgs &a, uint16_t width, uint16_t height, const float *score, const int32_t *n, int64_t budget, int32_t c_min,
                           int32_t c_max, int32_t *sample_counts, statmc_plan_result *result, void *workspace) {
    a = PlanArgs{};
    a.score = score, a.n = n, a.counts = sample_counts, a.result = result;
    a.ws = static_cast<long long *>(workspace);
    a.n_px = (long long)width * height;
    a.n_chunks = plan_scan_blocks(width, height);
    a.budget = budget;
    a.c_min = c_min, a.c_max = c_max;
    a.grid = (int)(a.n_chunks < kPlanMaxGrid ? a.n_chunks : kPlanMaxGrid);
    const long long px_per_lane = (a.n_chunks + a.grid - 1) / a.grid * kPlanQuad;
    a.wide = px_per_lane * c_max >= (1ll << 31);
    a.wide_wave = 64 * px_per_lane * c_max >= (1ll << 31);
    a.vec = !plan_misaligned(score, 16) && !plan_misaligned(n, 16) && !plan_misaligned(sample_counts, 16);
}

}  // namespace statmc
