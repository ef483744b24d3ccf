// statmc_accumulate_args.h -- what the accumulation entries of include/statmc.h check and fill on the host, each rule
// stated once.  Pure functions of their arguments: no HIP call, no device, no global or thread-local state; nothing is read through
// a pointer but the descriptors, the formats and the ranges.  true: valid; false: the caller's buffer names the argument (the code
// is STATMC_ERR_INVALID throughout).  tests/cpp/test_accumulate_args.cpp compiles this header alone, with and without sanitizers.
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "statmc_device.h"

namespace statmc {

struct Msg { char *buf; size_t len; };   // the caller's buffer
__attribute__((format(printf, 2, 3))) inline bool refuse(Msg m, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m.buf, m.len, fmt, ap);
    va_end(ap);
    return false;
}

// One call, as its entry describes it to the family's body (statmc_abi.hip).  What the dense families share ...
struct ArenaCall {
    uint16_t width, height;
    const statmc_stat_type *types;
    int n_types;
    const int32_t *formats;   // optional (the _formats entries): NULL = every arena fp32
    const int32_t *counts;    // optional (the _counted entries): the film's per-pixel sample counts
    void *stream;
};
struct FilmCall : ArenaCall {   // ... film-major: every type's `samples` is [n_samples][height][width][channels]
    const int32_t *ranges;
    int n_ranges;
    bool whole_film_default;    // the entries with formats or counts: NULL or 0 ranges mean the whole film (default_row_ranges)
};
struct TilesCall : ArenaCall {   // ... tile-fed: every type's `samples` is an arena of tile blocks (AccumulateTilesArgs)
    const int32_t *tile_bounds;
    const int64_t *tile_offsets;
    const int32_t *tile_samples;
    int n_tiles;
};
struct RecordsCall {   // unordered (pixel, sample) records
    uint16_t width, height;
    const statmc_stat_type *types;
    int n_types;
    const int32_t *pixels;                // the record-major entries: every type's `samples` is [n_records][channels]
    const void *records;                  // the interleaved entries: records and layout instead
    const statmc_record_layout *layout;
    bool interleaved;
    int64_t n_records;
    const int32_t *split_above;           // optional (the _split entries)
    void *stream;
};
// The type-count limit.  n_ranges: the film-major entries' range count, whose launch has one entry per (row range, type); NULL for
// the tile and records entries.
inline bool check_type_limit(int n_types, const int *n_ranges, Msg m) {
    if (!n_ranges) return (n_types >= 0 && n_types <= kMaxStatTypes) || refuse(m, "n_types must be in [0,%d]", kMaxStatTypes);
    return (n_types >= 0 && *n_ranges >= 0 && (long long)n_types * *n_ranges <= kMaxStatTypes) ||
           refuse(m, "n_types x n_ranges must be in [0,%d]", kMaxStatTypes);
}
inline bool check_n_tiles(int n_tiles, Msg m) { return n_tiles >= 0 || refuse(m, "n_tiles = %d: negative tile count", n_tiles); }
inline bool default_row_ranges(FilmCall &c, int32_t *whole, Msg m) {
    if (c.ranges && c.n_ranges != 0) return true;
    if (c.n_ranges != 0) return refuse(m, "n_ranges = %d without ranges", c.n_ranges);
    whole[0] = 0, whole[1] = c.height;
    c.ranges = whole, c.n_ranges = 1;
    return true;
}
// Sample formats: the values ...
inline bool is_half(const int32_t *formats, int i) { return formats && formats[i] == STATMC_SAMPLES_F16; }
inline int half_mask_of(const int32_t *formats, int n_types) {
    int mask = 0;
    for (int i = 0; i < n_types; i++) mask |= (is_half(formats, i) ? 1 : 0) << i;
    return mask;
}
inline bool check_sample_formats(const int32_t *formats, int n_types, Msg m) {
    for (int i = 0; formats && i < n_types; i++)
        if (formats[i] != STATMC_SAMPLES_F32 && formats[i] != STATMC_SAMPLES_F16)
            return refuse(m, "sample_formats[%d] = %d: STATMC_SAMPLES_F32 (0) or STATMC_SAMPLES_F16 (1)", i, (int)formats[i]);
    return true;
}
// ... and what the arenas must be, in the order the counted entries report it: sample_counts 4-byte aligned, the format values,
// types given, no 16-bit arena at an odd address (types[i].samples is read as a number, not through)
inline bool check_sample_arenas(const ArenaCall &c, Msg m) {
    if (reinterpret_cast<uintptr_t>(c.counts) & 3) return refuse(m, "sample_counts is not 4-byte aligned");
    if (!check_sample_formats(c.formats, c.n_types, m)) return false;
    if (c.n_types > 0 && !c.types) return refuse(m, "null types");
    for (int i = 0; i < c.n_types; i++)
        if (is_half(c.formats, i) && (reinterpret_cast<uintptr_t>(c.types[i].samples) & 1))
            return refuse(m, "types[%d]: a 16-bit sample arena at an odd address", i);
    return true;
}
// What an entry has always refused before it looked at the device: nothing without formats and counts; else the limit (n_ranges:
// film-major) and, with counts, n_tiles (tile-fed); then the format values or, with counts or a half arena, check_sample_arenas.
inline bool check_ahead_of_device(const ArenaCall &c, const int *n_ranges, const int *n_tiles, Msg m) {
    if (!c.formats && !c.counts) return true;
    if (!check_type_limit(c.n_types, n_ranges, m) || (c.counts && n_tiles && !check_n_tiles(*n_tiles, m))) return false;
    return (c.counts || half_mask_of(c.formats, c.n_types)) ? check_sample_arenas(c, m) : check_sample_formats(c.formats, c.n_types, m);
}

// Validates one statmc_stat_type and translates it for the kernels.  batch: the film-major entries, whose n_samples counts (0: no
// samples needed); the tile and records entries ignore it.  pre_table / pre_flags: the device's pre-pass table and flags, handed to
// a type with the optional epilogue (mean_corr and discriminator: the pre-pass of the updated moments).
inline bool fill_stat_type(int pre_table, int pre_flags, const statmc_stat_type &t, int i, uint16_t width, uint16_t height, bool batch,
                           AccumulateType &d, Msg m) {
    if (t.channels != 1 && t.channels != 3) return refuse(m, "types[%d]: channels must be 1 or 3", i);
    if (t.max_moment < 1 || t.max_moment > 3) return refuse(m, "types[%d]: max_moment must be 1..3", i);
    if (batch && t.n_samples < 0) return refuse(m, "types[%d]: negative n_samples", i);
    if (!t.n || !t.mean || ((!batch || t.n_samples) && !t.samples)) return refuse(m, "types[%d]: null pointer", i);
    if (t.max_moment >= 2 && !t.m2) return refuse(m, "types[%d]: null m2", i);
    if (t.max_moment >= 3 && !t.m3) return refuse(m, "types[%d]: null m3", i);
    if (t.transform && (!t.film_mean || !t.film_m2)) return refuse(m, "types[%d]: transform types need film_mean and film_m2", i);
    const bool epilogue = t.mean_corr || t.discriminator;
    if (epilogue && (!t.mean_corr || !t.discriminator)) return refuse(m, "types[%d]: mean_corr and discriminator come together", i);
    if (epilogue && t.max_moment < 3) return refuse(m, "types[%d]: the pre-pass epilogue needs max_moment 3 (it reads m2 and m3)", i);
    const long long n_elems = (long long)width * height * t.channels;   // (also the stride: the whole film's plane)
    d = AccumulateType{t.samples, t.n, t.mean, t.m2, t.m3, t.film_mean, t.film_m2, n_elems, /* stride */ n_elems, t.channels, t.n_samples,
                       t.transform ? 1 : 0, t.max_moment, t.mean_corr, t.discriminator, epilogue ? pre_table : 0, epilogue ? pre_flags : 0};
    return true;
}

// The entries of a film-major launch (k: AccumulateArgs or AccumulateCountedArgs): one per (non-empty row range, stat type), every
// pointer advanced to the range's first row; bit e of half_mask: entry e reads a half arena.  Every range lies inside the film, is
// not reversed and overlaps none before it.  counts_out (the counted block's, else NULL): the film's count image, advanced
// likewise; there a valid entry with n_samples == 0 folds nothing and is left out of the launch.  k.t holds kMaxStatTypes
// entries: the call passed check_type_limit.
template <class Args>
inline bool fill_row_range_entries(Args &k, int pre_table, int pre_flags, const FilmCall &c, const int32_t **counts_out, Msg m) {
    k.n_types = k.half_mask = 0;
    for (int r = 0; r < c.n_ranges; r++) {
        const int y0 = c.ranges[2 * r], y1 = c.ranges[2 * r + 1];
        if (y0 < 0 || y1 > c.height || y0 > y1) return refuse(m, "rows [%d,%d) outside the %d-row image", y0, y1, (int)c.height);
        for (int q = 0; q < r; q++)
            if (y0 < c.ranges[2 * q + 1] && c.ranges[2 * q] < y1) return refuse(m, "row ranges %d and %d overlap", q, r);
        for (int i = 0; i < c.n_types && y0 < y1; i++) {
            AccumulateType &d = k.t[k.n_types];
            if (!fill_stat_type(pre_table, pre_flags, c.types[i], i, c.width, c.height, true, d, m)) return false;
            if (counts_out && d.n_samples == 0) continue;
            const long long px0 = (long long)y0 * c.width, e0 = px0 * d.channels;
            const bool half = is_half(c.formats, i);
            if (d.samples) d.samples = half ? reinterpret_cast<const float *>(reinterpret_cast<const uint16_t *>(d.samples) + e0) : d.samples + e0;
            if (half) k.half_mask |= 1 << k.n_types;
            d.n += px0;
            for (float **plane : {&d.mean, &d.m2, &d.m3, &d.film_mean, &d.film_m2, &d.mean_corr, &d.disc})
                if (*plane) *plane += e0;
            d.n_elems = (long long)(y1 - y0) * c.width * d.channels;   // d.stride stays the whole film's plane
            if (counts_out) counts_out[k.n_types] = c.counts + px0;
            k.n_types++;
        }
    }
    return true;
}

// What AccumulateTilesArgs and AccumulateTilesCountedArgs share: the types, the half mask and the tile descriptors.
template <class Args>
inline bool fill_tiles_args(Args &k, int pre_table, int pre_flags, const TilesCall &c, Msg m) {
    k.n_types = c.n_types;
    for (int i = 0; i < c.n_types; i++)
        if (!fill_stat_type(pre_table, pre_flags, c.types[i], i, c.width, c.height, false, k.t[i], m)) return false;
    k.half_mask = half_mask_of(c.formats, c.n_types);
    k.tile_bounds = c.tile_bounds;
    k.tile_offsets = reinterpret_cast<const long long *>(c.tile_offsets);
    k.tile_samples = c.tile_samples;
    k.n_tiles = c.n_tiles;
    k.width = c.width, k.height = c.height;
    return true;
}

// What RecordsArgs and RecordsInterleavedArgs share.  The types: every accumulate entry's validation (n_samples is ignored), the
// descriptors themselves travelling to the kernel with `transform` as 0 or 1; an interleaved call's samples are its records'
// fields, so types[i].samples is not looked at and travels as NULL.  epilogue: some type has the pre-pass epilogue.
template <class Args>
inline bool fill_records_args(Args &k, const RecordsCall &c, bool &epilogue, Msg m) {
    k.n_types = c.n_types;
    k.n_records = c.n_records;
    k.n_px = (long long)c.width * c.height;
    epilogue = false;
    for (int i = 0; i < c.n_types; i++) {
        AccumulateType checked;
        statmc_stat_type t = c.types[i];
        if (c.interleaved) t.samples = static_cast<const float *>(c.records);
        if (!fill_stat_type(0, 0, t, i, c.width, c.height, false, checked, m)) return false;
        if (c.interleaved) t.samples = nullptr;
        t.transform = t.transform ? 1 : 0;
        k.t[i] = t;
        epilogue = epilogue || t.mean_corr != nullptr;
    }
    return true;
}

}  // namespace statmc
