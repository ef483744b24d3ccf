// statmc_pool_args.h -- what statmc_pool_statistics (include/statmc.h) checks and fills on the host, each rule stated once, and
// the argument block its kernel takes (statmc_pool.hip).  Pure functions of their arguments: no HIP call, no device, no global or
// thread-local state; nothing is read through a pointer but the entries (the image pointers are compared as numbers).  true: valid;
// false: the caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  Host-only and on its own:
// tests/cpp/test_pool_args.cpp compiles this header with nothing but include/statmc.h, with and without sanitizers.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"

namespace statmc {

constexpr int kMaxPoolEntries = 16;
enum { kPoolMean = 0, kPoolM2, kPoolM3, kPoolFilmMean, kPoolFilmM2, kPoolFields };

// One entry as the kernel walks it.  cnt_src: the fine counts every merge of the entry is weighed with -- the entry's own src.n, or
// those of the entry it borrows them from (read only, so the entry order of a launch does not matter).  cnt_dst: NULL unless the
// entry owns its counts.
struct PoolEntry {
    const int32_t *cnt_src;
    int32_t *cnt_dst;
    const float *s[kPoolFields];     // fine planes (NULL: not pooled)
    float *d[kPoolFields];           // the matching coarse planes
    float *mean_corr, *disc;         // optional pre-pass epilogue (own counts, max_moment 3)
    int channels, moments, film, reserved;   // film: 0, 1 (film_mean) or 2 (film_mean and film_m2) planes of their own
};
struct PoolArgs {
    PoolEntry e[kMaxPoolEntries];
    statmc_prepass_context ctx;      // the epilogue's table and flags (entries with mean_corr / disc)
    int n_entries, k;
    int width, height, wc, hc;       // the fine film and the coarse one: wc = ceil(width / k), hc = ceil(height / k)
    int vec, reserved;               // vec: every plane 8-byte aligned and width even -- a lane's pixel pair moves as one dwordx2
};
static_assert(sizeof(PoolArgs) <= 4096, "PoolArgs is passed by value: the kernel-argument limit");

struct PoolMsg { char *buf; size_t len; };   // the caller's buffer
__attribute__((format(printf, 2, 3))) inline bool pool_refuse(PoolMsg m, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m.buf, m.len, fmt, ap);
    va_end(ap);
    return false;
}

inline int pool_coarse(int fine, int k) { return (fine + k - 1) / k; }

// the planes of one side an entry moves, NULL where it moves none: mean .. film_m2, n, mean_corr, discriminator
enum { kPoolPlaneN = kPoolFields, kPoolPlaneMeanCorr, kPoolPlaneDisc, kPoolPlanes };
struct PoolPlanes {
    const void *p[kPoolPlanes];
    size_t bytes[kPoolPlanes];
};
inline bool pool_own_film_mean(const statmc_stat_type &t) { return t.film_mean && t.film_mean != t.mean; }
inline bool pool_own_film_m2(const statmc_stat_type &t) { return t.film_m2 && t.film_m2 != t.m2; }
inline PoolPlanes pool_planes(const statmc_stat_type &t, bool dst, bool own_counts, size_t n_px) {
    PoolPlanes q = {};
    const size_t img = n_px * (size_t)t.channels * sizeof(float);
    q.p[kPoolMean] = t.mean;
    q.p[kPoolM2] = t.max_moment >= 2 ? t.m2 : nullptr;
    q.p[kPoolM3] = t.max_moment >= 3 ? t.m3 : nullptr;
    q.p[kPoolFilmMean] = pool_own_film_mean(t) ? t.film_mean : nullptr;
    q.p[kPoolFilmM2] = pool_own_film_m2(t) ? t.film_m2 : nullptr;
    q.p[kPoolPlaneN] = own_counts ? t.n : nullptr;
    q.p[kPoolPlaneMeanCorr] = dst ? t.mean_corr : nullptr;
    q.p[kPoolPlaneDisc] = dst ? t.discriminator : nullptr;
    for (int f = 0; f < kPoolPlanes; f++) q.bytes[f] = f == kPoolPlaneN ? n_px * sizeof(int32_t) : img;
    return q;
}
inline bool pool_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

// What a call is refused for before anything looks at the device, in this order: k, the film size, n_entries, NULL entries; then
// entry by entry the fields of statmc_pool_entry; then the rules between entries (two writers of one image, a dst image over a src
// image).  n_entries == 0 passes with entries == NULL.
inline bool check_pool_call(uint16_t width, uint16_t height, int k, const statmc_pool_entry *entries, int n_entries, PoolMsg m) {
    if (k != 2 && k != 4 && k != 8) return pool_refuse(m, "k = %d: must be 2, 4 or 8", k);
    if (width == 0 || height == 0) return pool_refuse(m, "empty image: width and height must be positive");
    if (n_entries < 0 || n_entries > kMaxPoolEntries) return pool_refuse(m, "n_entries must be in [0,%d]", kMaxPoolEntries);
    if (n_entries == 0) return true;
    if (!entries) return pool_refuse(m, "null entries");
    static const char *names[kPoolFields] = {"mean", "m2", "m3", "film_mean", "film_m2"};
    for (int i = 0; i < n_entries; i++) {
        const statmc_pool_entry &e = entries[i];
        const statmc_stat_type &d = e.dst, &s = e.src;
        if (d.channels != 1 && d.channels != 3) return pool_refuse(m, "entries[%d]: channels must be 1 or 3", i);
        if (d.max_moment < 1 || d.max_moment > 3) return pool_refuse(m, "entries[%d]: max_moment must be 1..3", i);
        if (s.channels != d.channels || s.max_moment != d.max_moment)
            return pool_refuse(m, "entries[%d]: dst and src disagree on channels or max_moment", i);
        if (e.count_of == -1) {
            if (!d.n || !s.n) return pool_refuse(m, "entries[%d]: null n (count_of = -1: the entry's own counts)", i);
        } else if (e.count_of < 0 || e.count_of >= n_entries || e.count_of == i || entries[e.count_of].count_of != -1) {
            return pool_refuse(m, "entries[%d]: bad count_of %d (-1, or an entry with counts of its own)", i, (int)e.count_of);
        } else if (d.n || s.n) {
            return pool_refuse(m, "entries[%d]: borrows entry %d's counts, dst.n and src.n must be NULL", i, (int)e.count_of);
        }
        // the raw-sample chain: film images of their own only (aliased ones are the moments, pooled once)
        if ((pool_own_film_m2(d) && !pool_own_film_mean(d)) || (pool_own_film_m2(s) && !pool_own_film_mean(s)))
            return pool_refuse(m, "entries[%d]: film_m2 without a film_mean of its own", i);
        if (pool_own_film_mean(d) != pool_own_film_mean(s) || pool_own_film_m2(d) != pool_own_film_m2(s))
            return pool_refuse(m, "entries[%d]: dst and src disagree on their film planes", i);
        const PoolPlanes dp = pool_planes(d, true, false, 0), sp = pool_planes(s, false, false, 0);
        for (int f = 0; f < kPoolM3 + 1; f++)
            if (f < d.max_moment && (!dp.p[f] || !sp.p[f])) return pool_refuse(m, "entries[%d]: null %s", i, names[f]);
        if (d.mean_corr || d.discriminator) {
            if (!d.mean_corr || !d.discriminator) return pool_refuse(m, "entries[%d]: mean_corr and discriminator come together", i);
            if (d.max_moment < 3) return pool_refuse(m, "entries[%d]: the pre-pass epilogue needs max_moment 3", i);
            if (e.count_of != -1) return pool_refuse(m, "entries[%d]: the pre-pass epilogue needs counts of the entry's own", i);
        }
    }
    const size_t fine = (size_t)width * height, coarse = (size_t)pool_coarse(width, k) * pool_coarse(height, k);
    for (int i = 0; i < n_entries; i++) {
        const PoolPlanes di = pool_planes(entries[i].dst, true, entries[i].count_of == -1, coarse);
        for (int j = 0; j < n_entries; j++) {
            const PoolPlanes dj = pool_planes(entries[j].dst, true, entries[j].count_of == -1, coarse);
            const PoolPlanes sj = pool_planes(entries[j].src, false, entries[j].count_of == -1, fine);
            for (int f = 0; f < kPoolPlanes; f++)
                for (int g = 0; g < kPoolPlanes; g++) {
                    if (!di.p[f]) continue;
                    if (j < i && di.p[f] == dj.p[g]) {
                        if (f == kPoolPlaneN && g == kPoolPlaneN) return pool_refuse(m, "entries[%d] and [%d] own the same count image", j, i);
                        return pool_refuse(m, "entries[%d] and [%d] write the same dst image", j, i);
                    }
                    if (j == i && f < g && di.p[f] == dj.p[g]) return pool_refuse(m, "entries[%d]: two of its dst images are the same", i);
                    if (pool_ranges_overlap(di.p[f], di.bytes[f], sj.p[g], sj.bytes[g]))
                        return pool_refuse(m, "entries[%d]: a dst image overlaps a src image of entries[%d]", i, j);
                }
        }
    }
    return true;
}

// The kernel's argument block of a call that passed check_pool_call (ctx is the caller's to fill).
inline void fill_pool_args(PoolArgs &a, uint16_t width, uint16_t height, int k, const statmc_pool_entry *entries, int n_entries) {
    a = PoolArgs{};
    a.n_entries = n_entries;
    a.k = k;
    a.width = width, a.height = height;
    a.wc = pool_coarse(width, k), a.hc = pool_coarse(height, k);
    a.vec = width % 2 == 0;
    const auto aligned8 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    for (int i = 0; i < n_entries; i++) {
        const statmc_pool_entry &e = entries[i];
        const bool own = e.count_of == -1;
        PoolEntry &q = a.e[i];
        const PoolPlanes dp = pool_planes(e.dst, true, own, 0), sp = pool_planes(e.src, false, own, 0);
        for (int f = 0; f < kPoolFields; f++) {
            q.d[f] = static_cast<float *>(const_cast<void *>(dp.p[f]));
            q.s[f] = static_cast<const float *>(sp.p[f]);
            a.vec &= aligned8(sp.p[f]);   // (the coarse planes are written pixel by pixel)
        }
        q.cnt_src = own ? e.src.n : entries[e.count_of].src.n;
        q.cnt_dst = own ? e.dst.n : nullptr;
        a.vec &= aligned8(q.cnt_src);
        q.mean_corr = e.dst.mean_corr;
        q.disc = e.dst.discriminator;
        q.channels = e.dst.channels;
        q.moments = e.dst.max_moment;
        q.film = dp.p[kPoolFilmM2] ? 2 : dp.p[kPoolFilmMean] ? 1 : 0;
    }
}

}  // namespace statmc
