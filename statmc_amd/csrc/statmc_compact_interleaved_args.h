// statmc_compact_interleaved_args.h -- what statmc_compact_accumulate_interleaved (include/statmc.h) checks and fills on the host,
// and the argument block its kernels take (statmc_compact.hip).  Pure functions of their arguments: no HIP call, no device, no global
// or thread-local state; nothing is read through a pointer but the descriptors and the layout (records and offsets are compared as
// numbers).  true: valid; false: the caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  Nothing is
// restated: the run clamp and the run count are statmc_compact_args.h's, the field rules and the type sets of the fused fold are
// statmc_records_plan.h's (check_records_interleaved, handed a pixel offset that is valid whatever the caller's layout holds there;
// plan_records_interleaved).  Also here, because the kernel and tests/cpp/test_compact_interleaved_args.cpp share it: the map from
// a position in the arena to a byte offset, 64-bit throughout.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"
#include "statmc_compact_args.h"
#include "statmc_records_plan.h"

namespace statmc {

// Where the field at `field_offset` of the record at `position` starts, in bytes from `records`.  (2^63 / stride positions: no
// arena reaches that.)
__host__ __device__ inline int64_t compact_record_byte(int64_t position, int32_t stride, int32_t field_offset) {
    return position * (int64_t)stride + (int64_t)field_offset;
}

// What statmc_debug_compact_interleaved_path takes and statmc_debug_last_compact_interleaved_path reports
enum { kCompactIlvAuto = 0, kCompactIlvFusedStaged = 1, kCompactIlvFusedDirect = 2, kCompactIlvGeneral = 3, kCompactIlvSplitBit = 4 };

// The LDS window of one wave of the staged fused fold: whole 1-KiB DMA groups, at most the 64 KiB a workgroup may ask for.
constexpr int kCompactIlvWindowMin = 1024, kCompactIlvWindowMax = 65536;
// 16 fp32 records of 48 bytes on each of a wave's 64 pixels are 48 KiB; one more KiB takes the skew.  Three such one-wave workgroups
// share a CU's 160 KiB of LDS, where the kernel's registers would allow eight waves (DESIGN.md 4.1k has the A/B against 12, 24
// and 64 KiB).  tools/time_accumulate_compact_interleaved.py restates this number (DEFAULT_WINDOW): change both.
constexpr int kCompactIlvWindowDefault = 49 * 1024;
inline bool compact_interleaved_window_valid(int bytes) {
    return bytes >= kCompactIlvWindowMin && bytes <= kCompactIlvWindowMax && bytes % 1024 == 0;
}

struct CompactInterleavedArgs {
    statmc_stat_type t[kMaxStatTypes];   // samples: NULL (a type's values are its field of every record); transform as 0 or 1
    statmc_prepass_context ctx;          // the pre-pass epilogue's table and flags (types with mean_corr / discriminator)
    const long long *offsets;            // [n_px + 1]
    const char *records;                 // record i at records + i * stride
    long long n_records, n_px;
    int n_types;
    unsigned half_mask;                  // bit i: field i is IEEE half
    int split_above;                     // a run of more records is folded by the 64 lanes of a wave; INT32_MAX: never
    int stride;
    int off[kMaxStatTypes];              // field i's byte offset in a record
};
static_assert(sizeof(CompactInterleavedArgs) <= 4096, "CompactInterleavedArgs is passed by value: the kernel-argument limit");

// In the order include/statmc.h gives: the type limit; NULL types, layout, records or offsets with work to do; n_records; the
// layout's rules (stride, the records' address, every field's format, channels and offset -- check_records_interleaved's, in its
// order); offsets' alignment; split_above.  layout->pixel_offset is neither read nor checked.  Zero types or zero records is a
// valid call (a no-op); the layout of such a call is checked where it is given with all it refers to.
inline bool check_compact_interleaved_call(const statmc_stat_type *types, int n_types, const void *records, const statmc_record_layout *layout,
                                           const int64_t *offsets, int64_t n_records, int32_t split_above, Msg m) {
    if (!check_type_limit(n_types, nullptr, m)) return false;
    const bool work = n_types > 0 && n_records != 0;
    if (work && !types) return refuse(m, "null types");
    if (work && !layout) return refuse(m, "null layout");
    if (work && !records) return refuse(m, "null records");
    if (work && !offsets) return refuse(m, "null offsets");
    if (n_records < 0) return refuse(m, "n_records = %lld: must not be negative", (long long)n_records);
    if (layout && (n_types == 0 || types)) {
        statmc_record_layout fields = *layout;
        fields.pixel_offset = 0;   // valid under every stride the rules accept: a compact record has no pixel field
        const int64_t n = n_records > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : n_records;   // no 2^31 limit here
        if (!check_records_interleaved(types, n_types, records, &fields, n, m.buf, m.len)) return false;
    }
    if (compact_misaligned(offsets, 8)) return refuse(m, "offsets is not 8-byte aligned");
    if (split_above < 1) return refuse(m, "split_above %d: at least 1 (INT32_MAX: never split)", (int)split_above);
    return true;
}

// The kernel's argument block of a call with work to do that passed check_compact_interleaved_call: every type through the family's
// validation (fill_stat_type; samples and n_samples of a descriptor are ignored), the descriptors travelling with `transform` as 0
// or 1 and samples as NULL.  epilogue: some type has the pre-pass epilogue (the caller then fills k.ctx).
inline bool fill_compact_interleaved_args(CompactInterleavedArgs &k, uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                          const void *records, const statmc_record_layout &layout, const int64_t *offsets, int64_t n_records,
                                          int32_t split_above, bool &epilogue, Msg m) {
    k.n_types = n_types;
    k.offsets = reinterpret_cast<const long long *>(offsets);
    k.records = static_cast<const char *>(records);
    k.n_records = n_records;
    k.n_px = (long long)width * height;
    k.split_above = split_above;
    k.stride = layout.stride;
    k.half_mask = 0;
    epilogue = false;
    for (int i = 0; i < n_types; i++) {
        AccumulateType checked;
        statmc_stat_type t = types[i];
        t.samples = static_cast<const float *>(records);
        if (!fill_stat_type(0, 0, t, i, width, height, false, checked, m)) return false;
        t.samples = nullptr;
        t.transform = t.transform ? 1 : 0;
        k.t[i] = t;
        k.off[i] = layout.sample_offset[i];
        if (layout.sample_format[i] == STATMC_SAMPLES_F16) k.half_mask |= 1u << i;
        epilogue = epilogue || t.mean_corr != nullptr;
    }
    return true;
}

// Which fold serves the call: plan_records_interleaved's type sets (K, M, fmt, order) decide whether the fused kernel may, `force`
// (statmc_debug_compact_interleaved_path's value) and the default decide between its staged and direct variants.  *kernel: what
// is launched, kCompactIlvFusedStaged, kCompactIlvFusedDirect or kCompactIlvGeneral.  Expects a call that passed the check.
constexpr int kCompactIlvDefault = kCompactIlvFusedDirect;   // the A/B this rests on
inline RecordsInterleavedPlan plan_compact_interleaved(const statmc_stat_type *types, int n_types, const statmc_record_layout &layout, int force,
                                                       int *kernel) {
    const RecordsInterleavedPlan p = plan_records_interleaved(types, n_types, layout, force == kCompactIlvGeneral ? 1 : 0);
    if (p.path != kRecIlvFused) *kernel = kCompactIlvGeneral;
    else *kernel = force == kCompactIlvFusedStaged || force == kCompactIlvFusedDirect ? force : kCompactIlvDefault;
    return p;
}

}  // namespace statmc
