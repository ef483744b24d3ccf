// statmc_error_args.h -- what statmc_error_scores and statmc_plan_to_target (include/statmc.h) check and fill on the host, each rule
// stated once, and the argument blocks their kernels take (statmc_error.hip).  Pure functions of their arguments: no HIP call, no
// device, no global or thread-local state; nothing is read through a pointer (the image pointers are compared as numbers).  true:
// valid; false: the caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  Host-only and on its own:
// tests/cpp/test_error_args.cpp compiles this header with nothing but include/statmc.h, with and without sanitizers.
#pragma once

#include "statmc_plan_args.h"

namespace statmc {

constexpr int kErrorTables = 6;                  // alpha_index + 3 * sides, as statmc_set_t_quantiles numbers them
constexpr int kErrorDofMax = 4096;               // entries of a table: larger degrees of freedom read the last one
constexpr float kTargetLo = 0x1p-60f, kTargetHi = 0x1p60f;   // the live class of statmc_plan_samples: a target is a live error
constexpr int kTargetMaxGrid = 1024;             // workgroups of the one pass: 4 per compute unit of a 256-CU device; they stride over the chunks

struct ErrorArgs {
    const int32_t *n;
    const float *film_mean, *film_m2;
    const float *tq;             // the device's table `table`, 4096 entries; NULL: the standard error
    float *score;
    long long n_px;
    float eps;
    int channels, metric;
    int vec;                     // all four planes 16-byte aligned
};

struct TargetArgs {
    const float *error;
    const int32_t *n;
    int32_t *counts;
    statmc_target_result *result;
    long long n_px, n_chunks;
    float target;
    int c_min, c_max;
    int grid;
    int vec;                     // error, n and counts 16-byte aligned: a lane's full quad moves as dwordx4
};

// statmc_error_scores, in this order: the film size, channels, metric, table, eps (relative metric only), NULL images, alignment,
// score over an image it is computed from -- statmc_sample_scores' order with `table` right after `metric`.
inline bool check_error_scores_call(uint16_t width, uint16_t height, int channels, int metric, float eps, int table, const int32_t *n,
                                    const float *film_mean, const float *film_m2, const float *score, PlanMsg m) {
    if (width == 0 || height == 0) return plan_refuse(m, "empty image: width and height must be positive");
    if (channels != 1 && channels != 3) return plan_refuse(m, "channels = %d: must be 1 or 3", channels);
    if (metric != STATMC_SCORE_ABSOLUTE && metric != STATMC_SCORE_RELATIVE)
        return plan_refuse(m, "metric = %d: STATMC_SCORE_ABSOLUTE (0) or STATMC_SCORE_RELATIVE (1)", metric);
    if (table < STATMC_ERROR_NO_TABLE || table >= kErrorTables)
        return plan_refuse(m, "table = %d: STATMC_ERROR_NO_TABLE (-1) or 0..%d", table, kErrorTables - 1);
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

// tq: the device pointer of the table the call named, NULL with STATMC_ERROR_NO_TABLE.
inline void fill_error_args(ErrorArgs &a, uint16_t width, uint16_t height, int channels, int metric, float eps, const float *tq,
                            const int32_t *n, const float *film_mean, const float *film_m2, float *score) {
    a = ErrorArgs{};
    a.n = n, a.film_mean = film_mean, a.film_m2 = film_m2, a.tq = tq, a.score = score;
    a.n_px = (long long)width * height;
    a.eps = eps, a.channels = channels, a.metric = metric;
    a.vec = !plan_misaligned(n, 16) && !plan_misaligned(film_mean, 16) && !plan_misaligned(film_m2, 16) && !plan_misaligned(score, 16);
}

// statmc_plan_to_target, in this order: the film size, NULL pointers, alignment, the target, the bounds, sample_counts over an
// image the call reads or the result.
inline bool check_target_call(uint16_t width, uint16_t height, const float *error, const int32_t *n, float target, int32_t c_min, int32_t c_max,
                              const int32_t *sample_counts, const statmc_target_result *result, PlanMsg m) {
    if (width == 0 || height == 0) return plan_refuse(m, "empty image: width and height must be positive");
    if (!error) return plan_refuse(m, "null error");
    if (!n) return plan_refuse(m, "null n");
    if (!sample_counts) return plan_refuse(m, "null sample_counts");
    if (!result) return plan_refuse(m, "null result");
    if (plan_misaligned(error, 4)) return plan_refuse(m, "error is not 4-byte aligned");
    if (plan_misaligned(n, 4)) return plan_refuse(m, "n is not 4-byte aligned");
    if (plan_misaligned(sample_counts, 4)) return plan_refuse(m, "sample_counts is not 4-byte aligned");
    if (plan_misaligned(result, 8)) return plan_refuse(m, "result is not 8-byte aligned");
    if (!(target >= kTargetLo && target <= kTargetHi)) return plan_refuse(m, "target = %g: must lie in [2^-60, 2^60]", (double)target);
    if (c_min < 0 || c_min > c_max || c_max > kPlanMaxCount)
        return plan_refuse(m, "c_min = %d, c_max = %d: 0 <= c_min <= c_max <= %d", (int)c_min, (int)c_max, (int)kPlanMaxCount);
    const size_t px = (size_t)width * height * 4;
    if (plan_ranges_overlap(sample_counts, px, error, px)) return plan_refuse(m, "sample_counts overlaps error");
    if (plan_ranges_overlap(sample_counts, px, n, px)) return plan_refuse(m, "sample_counts overlaps n");
    if (plan_ranges_overlap(sample_counts, px, result, sizeof(statmc_target_result))) return plan_refuse(m, "sample_counts overlaps result");
    return true;
}

// The kernel's argument block of a call that passed check_target_call.
inline void fill_target_args(TargetArgs &a, uint16_t width, uint16_t height, const float *error, const int32_t *n, float target, int32_t c_min,
                             int32_t c_max, int32_t *sample_counts, statmc_target_result *result) {
    a = TargetArgs{};
    a.error = error, a.n = n, a.counts = sample_counts, a.result = result;
    a.n_px = (long long)width * height;
    a.n_chunks = plan_scan_blocks(width, height);
    a.target = target;
    a.c_min = c_min, a.c_max = c_max;
    a.grid = (int)(a.n_chunks < kTargetMaxGrid ? a.n_chunks : kTargetMaxGrid);
    a.vec = !plan_misaligned(error, 16) && !plan_misaligned(n, 16) && !plan_misaligned(sample_counts, 16);
}

}  // namespace statmc
