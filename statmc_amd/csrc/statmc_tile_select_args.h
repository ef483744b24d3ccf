// statmc_tile_select_args.h -- what statmc_score_tile_select and statmc_gate_tiles (include/statmc.h) check and fill on the host, each
// rule stated once, the nearest-rank rule of a tile, the argument blocks their kernels take (statmc_tile_select.hip) and a plain host
// evaluation of both over a whole film.  Pure functions of their arguments: no HIP call, no device, no global or thread-local state;
// nothing is read through a device pointer (the planes and images are compared as numbers; `out`, `q_num`, `src` and `dst` are host
// memory and are read).  The key is statmc_select_args.h's, the tile grid statmc_score_tiles_args.h's.
// tests/cpp/test_tile_select_args.cpp compiles this header with nothing but include/statmc.h, with and without sanitizers.
#pragma once

#include "statmc_score_tiles_args.h"

namespace statmc {

constexpr int kTileSelectPlanes = 3 * STATMC_TILE_SELECT_MAX_RANKS;
constexpr int kTileSelectMaxDen = 65536;
static_assert(STATMC_TILE_SELECT_MAX_RANKS == 4, "the kernel packs four 16-bit counts into two 32-bit words");
static_assert((long long)kTileMaxPixels * kTileSelectMaxDen == 1ll << 28, "n * q_num fits 32 bits");

// The nearest-rank rule: the 0-based rank of quantile q_num / q_den among n >= 1 sorted keys, max(0, ceil(n q_num / q_den) - 1).
STATMC_SUM_HD inline uint32_t tile_select_rank(uint32_t n, uint32_t q_num, uint32_t q_den) {
    const uint32_t up = (n * q_num + q_den - 1u) / q_den;   // below 2^28 + 2^16
    return up ? up - 1u : 0u;
}

struct TileSelectArgs {
    const float *score;
    statmc_tile_quantiles out;   // device pointers, NULL: not formed
    long long n_px, n_tiles;
    int width, height;
    int tile, tiles_x, tiles_y;
    uint32_t q_num[STATMC_TILE_SELECT_MAX_RANKS], q_den;   // slots n_ranks .. 3: q_num 0
    int n_ranks;
    int vec;   // score 16-byte aligned: a full aligned quad moves as dwordx4
};

struct GateArgs {
    const float *tile_value;
    int32_t *closed, *open;
    statmc_gate_result *result;   // NULL: not formed
    const uint32_t *src[STATMC_GATE_MAX_IMAGES];
    uint32_t *dst[STATMC_GATE_MAX_IMAGES];
    long long n_px, n_tiles;
    int width, height;
    int tile, tile_shift, tiles_x, tiles_y;
    uint32_t threshold_key;
    int n_images;
    int vec;   // every image 16-byte aligned: a full aligned quad moves as dwordx4
};

// the planes in the struct's order: name, slot, address
struct TileSelectPlane { const char *name; int slot; const void *at; };
inline void tile_select_planes(const statmc_tile_quantiles &o, TileSelectPlane (&p)[kTileSelectPlanes]) {
    for (int i = 0; i < STATMC_TILE_SELECT_MAX_RANKS; i++) {
        p[i] = TileSelectPlane{"value", i, o.value[i]};
        p[STATMC_TILE_SELECT_MAX_RANKS + i] = TileSelectPlane{"n_below", i, o.n_below[i]};
        p[2 * STATMC_TILE_SELECT_MAX_RANKS + i] = TileSelectPlane{"n_equal", i, o.n_equal[i]};
    }
}

inline bool tile_size_valid(int tile) { return tile == 8 || tile == 16 || tile == 32 || tile == 64; }

// statmc_score_tile_select, in this order: the film size, NULL score, q_num or out, every plane NULL or a plane in a slot >= n_ranks
// (for n_ranks in 1 .. 4: an n_ranks out of range is named further down), score's alignment, the planes' alignment, tile, n_ranks,
// q_den, q_num, a plane over the score image or over another plane.
inline bool check_tile_select_call(uint16_t width, uint16_t height, const float *score, int tile, const int32_t *q_num, int32_t q_den,
                                   int n_ranks, const statmc_tile_quantiles *out, SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!q_num) return select_refuse(m, "null q_num");
    if (!out) return select_refuse(m, "null out");
    TileSelectPlane p[kTileSelectPlanes];
    tile_select_planes(*out, p);
    bool any = false;
    for (int i = 0; i < kTileSelectPlanes; i++) any |= p[i].at != nullptr;
    if (!any) return select_refuse(m, "every plane of out is null");
    if (n_ranks >= 1 && n_ranks <= STATMC_TILE_SELECT_MAX_RANKS)
        for (int i = 0; i < kTileSelectPlanes; i++)
            if (p[i].at && p[i].slot >= n_ranks)
                return select_refuse(m, "out->%s[%d] is given: slots %d .. %d must be null", p[i].name, p[i].slot, n_ranks,
                                     STATMC_TILE_SELECT_MAX_RANKS - 1);
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    for (int i = 0; i < kTileSelectPlanes; i++)
        if (select_misaligned(p[i].at, 4)) return select_refuse(m, "out->%s[%d] is not 4-byte aligned", p[i].name, p[i].slot);
    if (!tile_size_valid(tile)) return select_refuse(m, "tile = %d: one of 8, 16, 32, 64", tile);
    if (n_ranks < 1 || n_ranks > STATMC_TILE_SELECT_MAX_RANKS) return select_refuse(m, "n_ranks = %d: 1 to %d", n_ranks, STATMC_TILE_SELECT_MAX_RANKS);
    if (q_den < 1 || q_den > kTileSelectMaxDen) return select_refuse(m, "q_den = %d: 1 to %d", (int)q_den, kTileSelectMaxDen);
    for (int i = 0; i < n_ranks; i++)
        if (q_num[i] < 0 || q_num[i] > q_den) return select_refuse(m, "q_num[%d] = %d: 0 to %d", i, (int)q_num[i], (int)q_den);
    const size_t px = (size_t)width * height * 4;
    const size_t plane = (size_t)tiles_across(width, tile) * (size_t)tiles_across(height, tile) * 4;
    for (int i = 0; i < kTileSelectPlanes; i++) {
        if (select_ranges_overlap(p[i].at, plane, score, px)) return select_refuse(m, "out->%s[%d] overlaps score", p[i].name, p[i].slot);
        for (int j = 0; j < i; j++)
            if (select_ranges_overlap(p[i].at, plane, p[j].at, plane))
                return select_refuse(m, "out->%s[%d] overlaps out->%s[%d]", p[i].name, p[i].slot, p[j].name, p[j].slot);
    }
    return true;
}

// The kernel's argument block of a call that passed check_tile_select_call.
inline void fill_tile_select_args(TileSelectArgs &a, uint16_t width, uint16_t height, const float *score, int tile, const int32_t *q_num,
                                  int32_t q_den, int n_ranks, const statmc_tile_quantiles *out) {
    a = TileSelectArgs{};
    a.score = score, a.out = *out;
    a.width = width, a.height = height;
    a.n_px = (long long)width * height;
    a.tile = tile;
    a.tiles_x = tiles_across(width, tile), a.tiles_y = tiles_across(height, tile);
    a.n_tiles = (long long)a.tiles_x * a.tiles_y;
    for (int i = 0; i < n_ranks; i++) a.q_num[i] = (uint32_t)q_num[i];
    a.q_den = (uint32_t)q_den;
    a.n_ranks = n_ranks;
    a.vec = !select_misaligned(score, 16);
}

// statmc_gate_tiles, in this order: the film size, NULL tile_value or open, n_images, NULL src or dst, a NULL image, alignment (the
// planes, the images, result), tile, a NaN threshold, the overlaps: among tile_value, closed, open and result; src[i] with dst[i]
// unless equal; an image with one of the four; dst[i] with another image.
inline bool check_gate_call(uint16_t width, uint16_t height, int tile, const float *tile_value, float threshold, const int32_t *closed,
                            const int32_t *open, const void *const *src, void *const *dst, int n_images, const statmc_gate_result *result,
                            SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!tile_value) return select_refuse(m, "null tile_value");
    if (!open) return select_refuse(m, "null open");
    if (n_images < 0 || n_images > STATMC_GATE_MAX_IMAGES) return select_refuse(m, "n_images = %d: 0 to %d", n_images, STATMC_GATE_MAX_IMAGES);
    if (n_images > 0 && !src) return select_refuse(m, "null src");
    if (n_images > 0 && !dst) return select_refuse(m, "null dst");
    for (int i = 0; i < n_images; i++) {
        if (!src[i]) return select_refuse(m, "null src[%d]", i);
        if (!dst[i]) return select_refuse(m, "null dst[%d]", i);
    }
    if (select_misaligned(tile_value, 4)) return select_refuse(m, "tile_value is not 4-byte aligned");
    if (select_misaligned(closed, 4)) return select_refuse(m, "closed is not 4-byte aligned");
    if (select_misaligned(open, 4)) return select_refuse(m, "open is not 4-byte aligned");
    for (int i = 0; i < n_images; i++) {
        if (select_misaligned(src[i], 4)) return select_refuse(m, "src[%d] is not 4-byte aligned", i);
        if (select_misaligned(dst[i], 4)) return select_refuse(m, "dst[%d] is not 4-byte aligned", i);
    }
    if (select_misaligned(result, 8)) return select_refuse(m, "result is not 8-byte aligned");
    if (!tile_size_valid(tile)) return select_refuse(m, "tile = %d: one of 8, 16, 32, 64", tile);
    if ((select_float_bits(threshold) & 0x7FFFFFFFu) > 0x7F800000u) return select_refuse(m, "threshold is NaN");
    const size_t px = (size_t)width * height * 4;
    const size_t plane = (size_t)tiles_across(width, tile) * (size_t)tiles_across(height, tile) * 4;
    struct { const char *name; const void *at; size_t bytes; } small[4] = {
        {"tile_value", tile_value, plane}, {"closed", closed, plane}, {"open", open, plane}, {"result", result, sizeof(statmc_gate_result)}};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < i; j++)
            if (select_ranges_overlap(small[i].at, small[i].bytes, small[j].at, small[j].bytes))
                return select_refuse(m, "%s overlaps %s", small[i].name, small[j].name);
    for (int i = 0; i < n_images; i++) {
        if (src[i] != dst[i] && select_ranges_overlap(src[i], px, dst[i], px))
            return select_refuse(m, "dst[%d] overlaps src[%d] without being equal to it", i, i);
        for (int j = 0; j < 4; j++) {
            if (select_ranges_overlap(src[i], px, small[j].at, small[j].bytes)) return select_refuse(m, "src[%d] overlaps %s", i, small[j].name);
            if (select_ranges_overlap(dst[i], px, small[j].at, small[j].bytes)) return select_refuse(m, "dst[%d] overlaps %s", i, small[j].name);
        }
        for (int j = 0; j < n_images; j++) {
            if (j == i) continue;
            if (select_ranges_overlap(dst[i], px, src[j], px)) return select_refuse(m, "dst[%d] overlaps src[%d]", i, j);
            if (j < i && select_ranges_overlap(dst[i], px, dst[j], px)) return select_refuse(m, "dst[%d] overlaps dst[%d]", i, j);
        }
    }
    return true;
}

// The kernels' argument block of a call that passed check_gate_call.
inline void fill_gate_args(GateArgs &a, uint16_t width, uint16_t height, int tile, const float *tile_value, float threshold, int32_t *closed,
                           int32_t *open, const void *const *src, void *const *dst, int n_images, statmc_gate_result *result) {
    a = GateArgs{};
    a.tile_value = tile_value, a.closed = closed, a.open = open, a.result = result;
    a.width = width, a.height = height;
    a.n_px = (long long)width * height;
    a.tile = tile;
    a.tile_shift = tile == 8 ? 3 : tile == 16 ? 4 : tile == 32 ? 5 : 6;
    a.tiles_x = tiles_across(width, tile), a.tiles_y = tiles_across(height, tile);
    a.n_tiles = (long long)a.tiles_x * a.tiles_y;
    a.threshold_key = select_key(select_float_bits(threshold));
    a.n_images = n_images;
    a.vec = 1;
    for (int i = 0; i < n_images; i++) {
        a.src[i] = static_cast<const uint32_t *>(src[i]), a.dst[i] = static_cast<uint32_t *>(dst[i]);
        if (select_misaligned(src[i], 16) || select_misaligned(dst[i], 16)) a.vec = 0;
    }
}

// The pixels of tile (tx, ty) of the grid.
inline uint32_t tile_pixels(int width, int height, int tile, int tx, int ty) {
    const int w = (tx + 1) * tile < width ? tile : width - tx * tile, h = (ty + 1) * tile < height ? tile : height - ty * tile;
    return (uint32_t)(w * h);
}

// ---------------------------------------------------------------- the whole computation on the host, the plain way
// The rank-th smallest of keys[0 .. n) by the kernel's rule: a descent over the 31 key bits, one count per bit.  *below: the number of
// keys under the result, *equal: the number equal to it.
inline uint32_t tile_select_descend(const uint32_t *keys, uint32_t n, uint32_t rank, uint32_t *below, uint32_t *equal) {
    uint32_t prefix = 0, under = 0;
    for (int bit = 30; bit >= 0; bit--) {
        const uint32_t cand = prefix | (1u << bit);
        uint32_t c = 0;
        for (uint32_t i = 0; i < n; i++) c += keys[i] < cand;
        if (c <= rank) prefix = cand, under = c;
    }
    uint32_t same = 0;
    for (uint32_t i = 0; i < n; i++) same += keys[i] == prefix;
    *below = under, *equal = same;
    return prefix;
}

// statmc_score_tile_select over the film bits[height][width] (float bit patterns, host memory): the planes of `out` are HOST memory
// here, NULL ones skipped.  scratch: kTileMaxPixels words.
inline void tile_select_host(const TileSelectArgs &a, const uint32_t *bits, const statmc_tile_quantiles &out, uint32_t *scratch) {
    for (int ty = 0; ty < a.tiles_y; ty++)
        for (int tx = 0; tx < a.tiles_x; tx++) {
            uint32_t n = 0;
            for (int y = ty * a.tile; y < (ty + 1) * a.tile && y < a.height; y++)
                for (int x = tx * a.tile; x < (tx + 1) * a.tile && x < a.width; x++) scratch[n++] = select_key(bits[(size_t)y * (size_t)a.width + (size_t)x]);
            const size_t t = (size_t)ty * (size_t)a.tiles_x + (size_t)tx;
            for (int i = 0; i < a.n_ranks; i++) {
                uint32_t below, equal;
                const uint32_t v = tile_select_descend(scratch, n, tile_select_rank(n, a.q_num[i], a.q_den), &below, &equal);
                if (out.value[i]) memcpy(out.value[i] + t, &v, 4);
                if (out.n_below[i]) out.n_below[i][t] = (int32_t)below;
                if (out.n_equal[i]) out.n_equal[i][t] = (int32_t)equal;
            }
        }
}

// statmc_gate_tiles' tile pass on HOST planes; the images are the caller's (dst_i[p] = open[tile of p] ? src_i[p] : 0).
inline void gate_tiles_host(const GateArgs &a, const uint32_t *tile_value_bits, int32_t *closed, int32_t *open, statmc_gate_result *result) {
    statmc_gate_result r = {a.n_tiles, 0, 0, 0};
    for (int ty = 0; ty < a.tiles_y; ty++)
        for (int tx = 0; tx < a.tiles_x; tx++) {
            const size_t t = (size_t)ty * (size_t)a.tiles_x + (size_t)tx;
            const bool was_closed = closed && closed[t] != 0;
            const bool above = select_key(tile_value_bits[t]) > a.threshold_key;
            open[t] = !was_closed && above ? 1 : 0;
            if (closed && !was_closed) closed[t] = above ? 0 : 1;
            r.n_open += open[t];
            r.n_closed_now += !was_closed && !above;
            if (open[t]) r.n_px_open += tile_pixels(a.width, a.height, a.tile, tx, ty);
        }
    if (result) *result = r;
}

}  // namespace statmc
