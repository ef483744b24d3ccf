// statmc_records_plan.h -- what statmc_accumulate_records_interleaved decides on the host: whether a record layout is valid and
// which kernel folds it.  Pure functions of their arguments: no HIP call, no device, no global or thread-local state, nothing but
// the C ABI's own structs -- tests/cpp/test_records_interleaved_plan.cpp compiles this header alone, with and without sanitizers.
// Also here, for the same reason: the chunk rule of the split entries (statmc_accumulate_records_split), the one definition the
// fold kernel and tests/cpp/test_records_split_plan.cpp share.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"

// What a function the device calls too is declared with.  A translation unit that calls records_split_chunk in a kernel defines
// this to the compiler's host-and-device attributes before the include (statmc_records.hip); everywhere else, and alone under
// g++, it is empty.
#ifndef STATMC_PLAN_HOST_DEVICE
#define STATMC_PLAN_HOST_DEVICE
#endif

namespace statmc {

constexpr int kRecordsMaxTypes = 16;      // statmc_record_layout's arrays (= kMaxStatTypes, statmc_device.h)
constexpr int kRecFusedTypes = 5;         // the fused fold: the radiance type, up to two mean-only RGB and two mean-only 1-channel types

// The limits and the layout rules of include/statmc.h, in the order the entry reports them.  true: valid.  false: `msg` names
// the argument.  Reads types[t].channels only (a field's length); the descriptors' other fields are the entry's to check.
inline bool check_records_interleaved(const statmc_stat_type *types, int n_types, const void *records, const statmc_record_layout *layout,
                                      int64_t n_records, char *msg, size_t msg_len) {
    if (n_types < 0 || n_types > kRecordsMaxTypes) {
        snprintf(msg, msg_len, "n_types must be in [0,%d]", kRecordsMaxTypes);
        return false;
    }
    if (n_records < 0 || n_records > (int64_t)INT32_MAX) {
        snprintf(msg, msg_len, "n_records must be in [0, 2^31)");
        return false;
    }
    if (layout == nullptr) {
        if (n_types == 0 && n_records == 0) return true;
        snprintf(msg, msg_len, "layout is NULL");
        return false;
    }
    if (layout->stride < 4 || layout->stride % 4 != 0) {
        snprintf(msg, msg_len, "layout->stride %d: a multiple of 4, at least 4", layout->stride);
        return false;
    }
    if (reinterpret_cast<uintptr_t>(records) % 4 != 0) {
        snprintf(msg, msg_len, "records must be 4-byte aligned");
        return false;
    }
    if (layout->pixel_offset < 0 || layout->pixel_offset % 4 != 0 || layout->pixel_offset > layout->stride - 4) {
        snprintf(msg, msg_len, "layout->pixel_offset %d: a multiple of 4 in [0, stride - 4 = %d]", layout->pixel_offset, layout->stride - 4);
        return false;
    }
    if (n_types > 0 && types == nullptr) {
        snprintf(msg, msg_len, "types is NULL");
        return false;
    }
    for (int t = 0; t < n_types; t++) {
        const int fmt = layout->sample_format[t], off = layout->sample_offset[t];
        if (fmt != STATMC_SAMPLES_F32 && fmt != STATMC_SAMPLES_F16) {
            snprintf(msg, msg_len, "layout->sample_format[%d] = %d: STATMC_SAMPLES_F32 or STATMC_SAMPLES_F16", t, fmt);
            return false;
        }
        if (types[t].channels != 1 && types[t].channels != 3) {
            snprintf(msg, msg_len, "types[%d].channels must be 1 or 3", t);
            return false;
        }
        const int elem = fmt == STATMC_SAMPLES_F16 ? 2 : 4;
        if (off < 0 || off % elem != 0 || (int64_t)off + (int64_t)elem * types[t].channels > layout->stride) {
            snprintf(msg, msg_len, "layout->sample_offset[%d] = %d: a multiple of %d with the field's %d bytes inside the stride (%d)", t, off, elem,
                     elem * types[t].channels, layout->stride);
            return false;
        }
    }
    return true;
}

// The fold's kernel.  kRecIlvGeneral serves every valid call: one lane per pixel and stat type, each reading its own field.
// kRecIlvFused: one lane per pixel holds every type's state and reads each record's fields once -- the type sets of the
// type-fused film-major walk (accumulate_fused_plan, statmc_pointwise.hip): exactly one RGB type with the transform and three
// moments, K <= 2 mean-only RGB types and M <= 2 mean-only 1-channel types without it, K + M >= 1; and its format classes: every
// field fp32 (fmt 0), every feature field half with the radiance field fp32 (1) or half (2).  Where the fields lie, whether they
// overlap and what the stride is play no part: both kernels take any valid layout.
enum { kRecIlvGeneral = 1, kRecIlvFused = 2 };
struct RecordsInterleavedPlan {
    int path;                       // kRecIlvGeneral | kRecIlvFused
    int K, M, fmt;                  // fused: the instantiation
    int order[kRecFusedTypes];      // fused: slot j (radiance, the K RGB types, the M 1-channel types) is types[order[j]]
};
// force: 0 = by the type set (fused wherever eligible: a record's line is then fetched by one lane instead of by one lane per type),
// 1 = general, 2 = fused where eligible (statmc_debug_accumulate_records_interleaved_path).  Expects a call that passed
// check_records_interleaved.
inline RecordsInterleavedPlan plan_records_interleaved(const statmc_stat_type *types, int n_types, const statmc_record_layout &layout, int force) {
    RecordsInterleavedPlan p{};
    p.path = kRecIlvGeneral;
    if (force == 1 || n_types < 2 || n_types > kRecFusedTypes) return p;
    int rad = -1, K = 0, M = 0, rgb[2] = {0, 0}, f1[2] = {0, 0};
    for (int i = 0; i < n_types; i++) {
        const statmc_stat_type &t = types[i];
        if (t.channels == 3 && t.transform && t.max_moment >= 3) {
            if (rad >= 0) return p;
            rad = i;
        } else if (!t.transform && t.max_moment == 1 && t.channels == 3) {
            if (K == 2) return p;
            rgb[K++] = i;
        } else if (!t.transform && t.max_moment == 1 && t.channels == 1) {
            if (M == 2) return p;
            f1[M++] = i;
        } else {
            return p;
        }
    }
    if (rad < 0 || K + M < 1) return p;
    bool features_half = true, features_f32 = true;
    for (int i = 0; i < n_types; i++) {
        if (i == rad) continue;
        const bool half = layout.sample_format[i] == STATMC_SAMPLES_F16;
        features_half = features_half && half;
        features_f32 = features_f32 && !half;
    }
    const bool rad_half = layout.sample_format[rad] == STATMC_SAMPLES_F16;
    if (features_f32 && !rad_half) p.fmt = 0;
    else if (features_half) p.fmt = rad_half ? 2 : 1;
    else return p;
    p.path = kRecIlvFused;
    p.K = K;
    p.M = M;
    p.order[0] = rad;
    for (int i = 0; i < K; i++) p.order[1 + i] = rgb[i];
    for (int i = 0; i < M; i++) p.order[1 + K + i] = f1[i];
    return p;
}

// ------------------------------------------------------------------ the split entries (statmc_accumulate_records_split, include/statmc.h)
constexpr int kRecSplitLanes = STATMC_RECORDS_SPLIT_LANES;   // the slots of a split pixel: the lanes of one wave

// split_above: a run of more than split_above records is split; anything below 1 is refused.  true: valid; false: `msg` names it.
inline bool check_records_split_above(int32_t split_above, char *msg, size_t msg_len) {
    if (split_above >= 1) return true;
    snprintf(msg, msg_len, "split_above %d: at least 1 (INT32_MAX: never split)", (int)split_above);
    return false;
}

// THE chunk rule.  A split pixel's run of cnt records -- positions [0, cnt) in ascending record index -- is cut into
// kRecSplitLanes contiguous chunks of L = ceil(cnt / kRecSplitLanes) records: slot j owns positions
// [min(j L, cnt), min((j + 1) L, cnt)) = [*begin, *begin + *len).  The chunks tile [0, cnt) in slot order; trailing slots may be
// empty (*len == 0, *begin == cnt).  cnt in [0, 2^31), slot in [0, kRecSplitLanes); 64-bit intermediates: (slot + 1) L passes
// 2^31 for the largest counts.
STATMC_PLAN_HOST_DEVICE inline void records_split_chunk(int cnt, int slot, int *begin, int *len) {
    const int64_t c = cnt;
    const int64_t L = (c + kRecSplitLanes - 1) / kRecSplitLanes;
    const int64_t lo = (int64_t)slot * L, hi = lo + L;
    const int64_t b = lo < c ? lo : c, e = hi < c ? hi : c;
    *begin = (int)b;
    *len = (int)(e - b);
}

}  // namespace statmc
