// statmc_compact_args.h -- what statmc_compact_offsets and statmc_compact_accumulate (include/statmc.h) check and fill on the host,
// each rule stated once, and the argument blocks their kernels take (statmc_compact.hip).  Pure functions of their arguments: no HIP
// call, no device, no global or thread-local state; nothing is read through a pointer but the descriptors and the formats (the
// image pointers are compared as numbers).  true: valid; false: the caller's buffer names the argument (the code is
// STATMC_ERR_INVALID throughout).  The rules the accumulation family already has -- the type limit, the format values, a type's own
// validation -- are statmc_accumulate_args.h's.  Also here, because the kernel and tests/cpp/test_compact_args.cpp share them: the
// run clamp and the map from a position in the arena to a byte offset, 64-bit throughout.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"
#include "statmc_accumulate_args.h"

namespace statmc {

// ---------------------------------------------------------------- positions
// Pixel p's run, from offsets[p] and offsets[p + 1]: start = clamp(o0, 0, n_samples), end = clamp(o1, start, n_samples).  The clamp
// comes before anything is derived from an offset: 0 <= *start <= *end <= n_samples whatever o0 and o1 hold.
__host__ __device__ inline void compact_run(int64_t o0, int64_t o1, int64_t n_samples, int64_t *start, int64_t *end) {
    const int64_t s = o0 < 0 ? 0 : o0 > n_samples ? n_samples : o0;
    const int64_t e = o1 < s ? s : o1 > n_samples ? n_samples : o1;
    *start = s;
    *end = e;
}
// Where sample `index` of a run that starts at position `offset` lies in a type's arena, in bytes from types[t].samples: the arena
// is sample-major [n_samples][channels], 4-byte (fp32) or 2-byte (half) elements.  (2^63 / 12 positions: no arena reaches that.)
__host__ __device__ inline int64_t compact_sample_byte(int64_t offset, int64_t index, int channels, bool half) {
    return (offset + index) * (int64_t)channels * (half ? 2 : 4);
}
// A run's length as the folds count it: they stay below 2^24 by contract, and wrong offsets -- clamped already -- may claim the
// whole arena for one pixel; a 32-bit count then covers the run's first 2^31 - 1 samples.
__host__ __device__ inline int32_t compact_run_count(int64_t start, int64_t end) {
    const int64_t c = end - start;
    return c > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)c;
}

// ---------------------------------------------------------------- statmc_compact_offsets
constexpr int kCompactBlock = 256;                          // 4 waves
constexpr int kCompactQuad = 4;                             // consecutive pixels per lane
constexpr int kCompactChunk = kCompactBlock * kCompactQuad; // pixels per workgroup: the scan's block

inline long long compact_scan_blocks(uint16_t width, uint16_t height) {
    return ((long long)width * height + kCompactChunk - 1) / kCompactChunk;
}
// the workspace: one 64-bit word per scan block
inline size_t compact_workspace_bytes(uint16_t width, uint16_t height) { return (size_t)compact_scan_blocks(width, height) * sizeof(int64_t); }

struct CompactOffsetsArgs {
    const int32_t *counts;
    long long *offsets;          // [n_px + 1]
    int32_t *owners;             // NULL or [owners_capacity]
    long long *ws;               // [n_chunks]
    long long n_px, n_chunks, owners_capacity;
    int cap;
    int vec;                     // counts 16-byte aligned: a lane's full quad moves as one dwordx4
};

inline bool compact_misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool compact_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// In this order: the film size, NULL pointers, alignment, cap, owners_capacity and owners, the workspace size, an output over an
// input, the workspace or the other output.
inline bool check_compact_offsets_call(uint16_t width, uint16_t height, const int32_t *sample_counts, int32_t cap, const int64_t *offsets,
                                       const int32_t *owners, int64_t owners_capacity, const void *workspace, size_t workspace_bytes, Msg m) {
    if (width == 0 || height == 0) return refuse(m, "empty image: width and height must be positive");
    if (!sample_counts) return refuse(m, "null sample_counts");
    if (!offsets) return refuse(m, "null offsets");
    if (!workspace) return refuse(m, "null workspace");
    if (compact_misaligned(sample_counts, 4)) return refuse(m, "sample_counts is not 4-byte aligned");
    if (compact_misaligned(offsets, 8)) return refuse(m, "offsets is not 8-byte aligned");
    if (compact_misaligned(owners, 4)) return refuse(m, "owners is not 4-byte aligned");
    if (compact_misaligned(workspace, 8)) return refuse(m, "workspace is not 8-byte aligned");
    if (cap < 0) return refuse(m, "cap = %d: must not be negative (INT32_MAX: no cap)", (int)cap);
    if (owners_capacity < 0) return refuse(m, "owners_capacity = %lld: must not be negative", (long long)owners_capacity);
    if (owners_capacity > 0 && !owners) return refuse(m, "owners_capacity = %lld with null owners", (long long)owners_capacity);
    const size_t need = compact_workspace_bytes(width, height);
    if (workspace_bytes < need)
        return refuse(m, "workspace_bytes = %zu: statmc_compact_offsets_workspace asks for %zu", workspace_bytes, need);
    const size_t px = (size_t)width * height, counts_b = px * 4, offsets_b = (px + 1) * 8, owners_b = owners ? (size_t)owners_capacity * 4 : 0;
    if (compact_ranges_overlap(offsets, offsets_b, sample_counts, counts_b)) return refuse(m, "offsets overlaps sample_counts");
    if (compact_ranges_overlap(offsets, offsets_b, workspace, need)) return refuse(m, "offsets overlaps workspace");
    if (compact_ranges_overlap(owners, owners_b, sample_counts, counts_b)) return refuse(m, "owners overlaps sample_counts");
    if (compact_ranges_overlap(owners, owners_b, workspace, need)) return refuse(m, "owners overlaps workspace");
    if (compact_ranges_overlap(owners, owners_b, offsets, offsets_b)) return refuse(m, "owners overlaps offsets");
    return true;
}

// The kernels' argument block of a call that passed check_compact_offsets_call.
inline void fill_compact_offsets_args(CompactOffsetsArgs &a, uint16_t width, uint16_t height, const int32_t *sample_counts, int32_t cap,
                                      int64_t *offsets, int32_t *owners, int64_t owners_capacity, void *workspace) {
    a = CompactOffsetsArgs{};
    a.counts = sample_counts;
    a.offsets = reinterpret_cast<long long *>(offsets);
    a.owners = owners_capacity > 0 ? owners : nullptr;
    a.ws = static_cast<long long *>(workspace);
    a.n_px = (long long)width * height;
    a.n_chunks = compact_scan_blocks(width, height);
    a.owners_capacity = owners_capacity;
    a.cap = cap;
    a.vec = !compact_misaligned(sample_counts, 16);
}

// ---------------------------------------------------------------- statmc_compact_accumulate
// What statmc_debug_compact_path takes and statmc_debug_last_compact_path reports
enum { kCompactAuto = 0, kCompactStaged = 1, kCompactDirect = 2, kCompactSplitBit = 4 };

struct CompactArgs {
    statmc_stat_type t[kMaxStatTypes];   // samples: the type's arena [n_samples][channels]; transform as 0 or 1
    statmc_prepass_context ctx;          // the pre-pass epilogue's table and flags (types with mean_corr / discriminator)
    const long long *offsets;            // [n_px + 1]
    long long n_samples, n_px;
    int n_types;
    unsigned half_mask;                  // bit i: t[i].samples is an IEEE-half arena
    int split_above;                     // a run of more samples is folded by the 64 lanes of a wave; INT32_MAX: never
};
static_assert(sizeof(CompactArgs) <= 4096, "CompactArgs is passed by value: the kernel-argument limit");

// In the family's order: the type limit; NULL types or offsets with work to do; n_samples; the format values; a half arena at an odd
// address; fp32 arenas and offsets misaligned; split_above.  Zero types or zero samples is a valid call (a no-op).
inline bool check_compact_accumulate_call(const statmc_stat_type *types, const int32_t *sample_formats, int n_types, const int64_t *offsets,
                                          int64_t n_samples, int32_t split_above, Msg m) {
    if (!check_type_limit(n_types, nullptr, m)) return false;
    const bool work = n_types > 0 && n_samples != 0;
    if (work && !types) return refuse(m, "null types");
    if (work && !offsets) return refuse(m, "null offsets");
    if (n_samples < 0) return refuse(m, "n_samples = %lld: must not be negative", (long long)n_samples);
    if (!check_sample_formats(sample_formats, n_types, m)) return false;
    for (int i = 0; types && i < n_types; i++) {
        const uintptr_t at = reinterpret_cast<uintptr_t>(types[i].samples);
        if (is_half(sample_formats, i) && (at & 1)) return refuse(m, "types[%d]: a 16-bit sample arena at an odd address", i);
        if (!is_half(sample_formats, i) && (at & 3)) return refuse(m, "types[%d]: an fp32 sample arena that is not 4-byte aligned", i);
    }
    if (compact_misaligned(offsets, 8)) return refuse(m, "offsets is not 8-byte aligned");
    if (split_above < 1) return refuse(m, "split_above %d: at least 1 (INT32_MAX: never split)", (int)split_above);
    return true;
}

// The kernel's argument block of a call with work to do that passed check_compact_accumulate_call: every type through the family's
// validation (fill_stat_type; n_samples of a descriptor is ignored), the descriptors themselves travelling with `transform` as 0 or
// 1.  epilogue: some type has the pre-pass epilogue (the caller then fills k.ctx).
inline bool fill_compact_args(CompactArgs &k, uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                              int n_types, const int64_t *offsets, int64_t n_samples, int32_t split_above, bool &epilogue, Msg m) {
    k.n_types = n_types;
    k.offsets = reinterpret_cast<const long long *>(offsets);
    k.n_samples = n_samples;
    k.n_px = (long long)width * height;
    k.half_mask = (unsigned)half_mask_of(sample_formats, n_types);
    k.split_above = split_above;
    epilogue = false;
    for (int i = 0; i < n_types; i++) {
        AccumulateType checked;
        statmc_stat_type t = types[i];
        if (!fill_stat_type(0, 0, t, i, width, height, false, checked, m)) return false;
        t.transform = t.transform ? 1 : 0;
        k.t[i] = t;
        epilogue = epilogue || t.mean_corr != nullptr;
    }
    return true;
}

}  // namespace statmc
