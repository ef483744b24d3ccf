// statmc_state_records_args.h -- what statmc_state_dwords, statmc_gather_states and statmc_combine_records (include/statmc.h) check
// and fill on the host, each rule stated once, and the argument block their kernels take (statmc_state_records.hip).  Pure
// functions of their arguments: no HIP call, no device, no global or thread-local state; nothing is read through a pointer but the
// descriptors and the host array `states` (the device pointers in both are compared as numbers).  true: valid; false: the caller's
// buffer names the argument (the code is STATMC_ERR_INVALID throughout).  The rules the accumulation family already has -- the type
// limit, a type's own validation -- are statmc_accumulate_args.h's; split_above's is statmc_records_plan.h's.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"
#include "statmc_accumulate_args.h"
#include "statmc_records_plan.h"

namespace statmc {

// The dwords of one state record: the count, then per channel mean, m2 (max_moment >= 2), m3 (max_moment 3) and, for a transform
// type, film_mean and film_m2 -- statmc::device::state_dwords<C, MAXM, TRANSFORM>() for run-time values.  0: values a stat type
// cannot have.
inline size_t state_record_dwords(int channels, int max_moment, int transform) {
    if ((channels != 1 && channels != 3) || max_moment < 1 || max_moment > 3) return 0;
    return (size_t)1 + (size_t)channels * (size_t)(max_moment + (transform ? 2 : 0));
}

// What both kernels take.  t[i].samples carries type i's record array ([n_records][dwords[i]] dwords: read by the combine,
// written by the gather) in place of a sample arena; transform travels as 0 or 1.
struct StateRecordsArgs {
    statmc_stat_type t[kMaxStatTypes];
    statmc_prepass_context ctx;      // the combine's pre-pass epilogue (types with mean_corr / discriminator)
    const int32_t *pixels;           // the gather: record i's pixel
    const int32_t *order;            // the combine: record indices sorted by pixel, stable     (workspace)
    const int32_t *seg;              // ... and {start, end} of every pixel's run in order[]    (workspace)
    long long n_records, n_px;
    int n_types;
    int split_above;                 // the combine: a run of more records is folded by the 64 lanes of a wave; INT32_MAX: never
    int dwords[kMaxStatTypes];       // state_record_dwords of type i
};
static_assert(sizeof(StateRecordsArgs) <= 4096, "StateRecordsArgs is passed by value: the kernel-argument limit");

inline bool state_records_misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// What the two entries share, in this order: the type limit; n_records; (split_above: the combine's, between these and the rest);
// then, with work to do -- zero types or zero records is a valid call, a no-op, whatever the other arguments hold --: NULL types,
// pixels or states; pixels not 4-byte aligned; a NULL or misaligned states[t]; the film size.
inline bool check_state_records_limits(int n_types, int64_t n_records, Msg m) {
    if (!check_type_limit(n_types, nullptr, m)) return false;
    if (n_records < 0 || n_records > (int64_t)INT32_MAX) return refuse(m, "n_records = %lld: must be in [0, 2^31)", (long long)n_records);
    return true;
}
inline bool check_state_records_pointers(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const int32_t *pixels,
                                         int64_t n_records, const void *const *states, Msg m) {
    if (n_types == 0 || n_records == 0) return true;
    if (!types) return refuse(m, "null types");
    if (!pixels) return refuse(m, "null pixels");
    if (!states) return refuse(m, "null states");
    if (state_records_misaligned(pixels, 4)) return refuse(m, "pixels is not 4-byte aligned");
    for (int i = 0; i < n_types; i++) {
        if (!states[i]) return refuse(m, "states[%d] is null", i);
        if (state_records_misaligned(states[i], 4)) return refuse(m, "states[%d] is not 4-byte aligned", i);
    }
    if (width == 0 || height == 0) return refuse(m, "empty image: width and height must be positive");
    return true;
}
inline bool check_gather_states_call(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const int32_t *pixels,
                                     int64_t n_records, const void *const *states, Msg m) {
    return check_state_records_limits(n_types, n_records, m) && check_state_records_pointers(width, height, types, n_types, pixels, n_records, states, m);
}
inline bool check_combine_records_call(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const int32_t *pixels,
                                       int64_t n_records, const void *const *states, int32_t split_above, Msg m) {
    return check_state_records_limits(n_types, n_records, m) && check_records_split_above(split_above, m.buf, m.len) &&
           check_state_records_pointers(width, height, types, n_types, pixels, n_records, states, m);
}

// The kernels' argument block of a call with work to do that passed its check: every type through the family's validation
// (fill_stat_type).  gather: the images are only read, and mean_corr / discriminator are ignored like samples and n_samples -- they
// travel as NULL.  epilogue (the combine): some type has the pre-pass epilogue (the caller then fills k.ctx).
inline bool fill_state_records_args(StateRecordsArgs &k, uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                    const int32_t *pixels, int64_t n_records, const void *const *states, int32_t split_above, bool gather,
                                    bool &epilogue, Msg m) {
    k.n_types = n_types;
    k.pixels = pixels;
    k.n_records = n_records;
    k.n_px = (long long)width * height;
    k.split_above = split_above;
    epilogue = false;
    for (int i = 0; i < n_types; i++) {
        AccumulateType checked;
        statmc_stat_type t = types[i];
        t.samples = static_cast<const float *>(states[i]);
        t.n_samples = 0;
        if (gather) t.mean_corr = t.discriminator = nullptr;
        if (!fill_stat_type(0, 0, t, i, width, height, false, checked, m)) return false;
        t.transform = t.transform ? 1 : 0;
        k.t[i] = t;
        k.dwords[i] = (int)state_record_dwords(t.channels, t.max_moment, t.transform);
        epilogue = epilogue || t.mean_corr != nullptr;
    }
    return true;
}

}  // namespace statmc
