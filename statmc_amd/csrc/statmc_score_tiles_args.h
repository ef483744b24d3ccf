// statmc_score_tiles_args.h -- what statmc_score_tiles (include/statmc.h) checks and fills on the host, each rule stated once, the
// argument block its kernel takes (statmc_score_tiles.hip) and the finalisation of a tile: the capped totals as limbs, and their
// quotient by the tile's pixel count to the nearest float, in integers alone.  Pure functions of their arguments: no HIP call, no
// device, no global or thread-local state; nothing is read through a device pointer (the planes of `out` are compared as numbers;
// `out` itself is a host struct and is read).  The key, the limbs, the carries and the rounding to a double are
// statmc_score_sum_args.h's.  The finalisation is written once for host and device: tests/cpp/test_score_tiles_args.cpp compiles this
// header with nothing but include/statmc.h, with and without sanitizers, and holds it to a long division of its own.
#pragma once

#include "statmc_score_sum_args.h"

namespace statmc {

constexpr int kTilePlanes = 8;
constexpr int kTileMaxPixels = STATMC_SCORE_TILES_MAX_TILE * STATMC_SCORE_TILES_MAX_TILE;   // the largest divisor of a mean
constexpr int kTileAccWords = kSumLimbs + kSumSqLimbs;   // a tile's table, in 64-bit words: the sum's accumulators, then the squares'
constexpr int kTileLimbs = kSumSqLimbs + 2;              // a carried integer, in 32-bit limbs: the squares' is the longest
static_assert(kTileMaxPixels == 4096, "tile_mean_bits divides 28-bit numbers by it in 32 bits");

struct TilesArgs {
    const float *score;
    statmc_tile_scores out;   // device pointers, NULL: not formed
    long long n_px, n_tiles;
    int width, height;
    int tile, tiles_x, tiles_y;
    uint32_t cap_key;
    int vec;   // score 16-byte aligned: a full aligned quad moves as dwordx4
};

inline int tiles_across(int extent, int tile) { return (extent + tile - 1) / tile; }

// the planes in the struct's order: name, address, bytes per entry
struct TilePlane { const char *name; const void *at; size_t entry; };
inline void tile_planes(const statmc_tile_scores &o, TilePlane (&p)[kTilePlanes]) {
    p[0] = TilePlane{"sum", o.sum, 8}, p[1] = TilePlane{"sum_sq", o.sum_sq, 8};
    p[2] = TilePlane{"mean", o.mean, 4}, p[3] = TilePlane{"max", o.max, 4};
    p[4] = TilePlane{"n_px", o.n_px, 4}, p[5] = TilePlane{"n_zero", o.n_zero, 4};
    p[6] = TilePlane{"n_infinite", o.n_infinite, 4}, p[7] = TilePlane{"n_clipped", o.n_clipped, 4};
}

// statmc_score_tiles, in this order: the film size, NULL score or out, every plane NULL, score's alignment, the planes' alignment,
// tile, a NaN cap, a plane over the score image or over another plane.
inline bool check_score_tiles_call(uint16_t width, uint16_t height, const float *score, int tile, float cap, const statmc_tile_scores *out,
                                   SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!out) return select_refuse(m, "null out");
    TilePlane p[kTilePlanes];
    tile_planes(*out, p);
    bool any = false;
    for (int i = 0; i < kTilePlanes; i++) any |= p[i].at != nullptr;
    if (!any) return select_refuse(m, "every plane of out is null");
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    for (int i = 0; i < kTilePlanes; i++)
        if (p[i].at && select_misaligned(p[i].at, p[i].entry)) return select_refuse(m, "out->%s is not %zu-byte aligned", p[i].name, p[i].entry);
    if (tile != 8 && tile != 16 && tile != 32 && tile != 64) return select_refuse(m, "tile = %d: one of 8, 16, 32, 64", tile);
    if ((select_float_bits(cap) & 0x7FFFFFFFu) > 0x7F800000u) return select_refuse(m, "cap is NaN");
    const size_t px = (size_t)width * height * 4;
    const size_t n_tiles = (size_t)tiles_across(width, tile) * (size_t)tiles_across(height, tile);
    for (int i = 0; i < kTilePlanes; i++) {
        if (select_ranges_overlap(p[i].at, n_tiles * p[i].entry, score, px)) return select_refuse(m, "out->%s overlaps score", p[i].name);
        for (int j = 0; j < i; j++)
            if (select_ranges_overlap(p[i].at, n_tiles * p[i].entry, p[j].at, n_tiles * p[j].entry))
                return select_refuse(m, "out->%s overlaps out->%s", p[i].name, p[j].name);
    }
    return true;
}

// The kernel's argument block of a call that passed check_score_tiles_call.
inline void fill_score_tiles_args(TilesArgs &a, uint16_t width, uint16_t height, const float *score, int tile, float cap,
                                  const statmc_tile_scores *out) {
    a = TilesArgs{};
    a.score = score, a.out = *out;
    a.width = width, a.height = height;
    a.n_px = (long long)width * height;
    a.tile = tile;
    a.tiles_x = tiles_across(width, tile), a.tiles_y = tiles_across(height, tile);
    a.n_tiles = (long long)a.tiles_x * a.tiles_y;
    a.cap_key = select_key(select_float_bits(cap));
    a.vec = !select_misaligned(score, 16);
}

// ---------------------------------------------------------------- the finalisation: integers only
// A tile's capped total as limbs.  acc[0 .. n): the accumulators of the pixels with 0 < key <= ck, key < 0x7F800000 -- the sum's
// (n = kSumLimbs) or, with `squares`, the squares' (n = kSumSqLimbs) --; the `clipped` pixels above ck count at val(ck), or at its
// square.  limb[0 .. n + 2): the total, every limb below 2^32.  One body for both, so that lanes of a wave that form a sum, a sum of
// squares and a mean side by side run the same instructions.
STATMC_SUM_HD inline void tile_capped_limbs(const uint64_t *acc, int n, bool squares, uint32_t ck, uint32_t clipped, uint32_t *limb) {
    sum_carry(acc, n, limb);
    const bool at_cap = ck > 0 && ck < kSumInfinite;
    const uint64_t M = sum_significand(ck);
    const int s = sum_shift(ck);
    const uint64_t q = squares ? M * M : M;           // below 2^48
    const int sh = squares ? 2 * s : s;
    const uint64_t upper = q >> (32 - (sh & 31));     // a shift of 1 .. 32
    const uint32_t v32[3] = {(uint32_t)(q << (sh & 31)), (uint32_t)upper, (uint32_t)(upper >> 32)};
    sum_add_product(limb, n + 2, sh >> 5, v32, 3, at_cap ? clipped : 0u);
}

// The bits of the float nearest, ties to even, to N * 2^-149 / count, N the integer of limb[0 .. n), 0 < count <= 4096; the quotient
// must not exceed the largest finite float (a mean of finite floats does not).  A long division from the top limb down, 16 bits of
// the dividend at a time so that every step is a 32-bit division of a number below 2^28; the quotient's leading digits are kept in
// a 64-bit window, the rest of them and the remainder only as "something non-zero lies below".  Below 2^24 units every integer is a
// float, subnormal or of exponent 1: the rounding there looks at twice the remainder against count alone.
STATMC_SUM_HD inline uint32_t tile_mean_bits(const uint32_t *limb, int n, uint32_t count) {
    uint64_t window = 0;     // the quotient's digits so far, while they fit
    int below = 0;           // the number of quotient bits under the window
    bool sticky = false;     // one of those bits is set
    uint32_t rem = 0;        // below count
    for (int i = n - 1; i >= 0; i--)
        for (int half = 1; half >= 0; half--) {
            const uint32_t cur = (rem << 16) | ((limb[i] >> (16 * half)) & 0xFFFFu);   // below 2^12 * 2^16
            const uint32_t digit = cur / count;   // below 2^16
            rem = cur % count;
            if (window >> 32) below += 16, sticky |= digit != 0;
            else window = (window << 16) | digit;
        }
    if (!(window >> 24)) {   // below is 0: the quotient is the window
        const uint32_t twice = 2 * rem;
        return (uint32_t)window + (twice > count || (twice == count && (window & 1u)) ? 1u : 0u);
    }
    int hb = 63;
    while (!((window >> hb) & 1u)) hb--;   // 24 .. 47
    const int drop = hb - 23;              // 1 .. 24
    uint32_t mant = (uint32_t)(window >> drop);   // 24 bits, the leading one set
    const bool half = (window >> (drop - 1)) & 1u;
    sticky |= (window & ((1ull << (drop - 1)) - 1u)) != 0 || rem != 0;
    if (half && (sticky || (mant & 1u))) mant++;   // 2^24: the carry goes into the exponent below
    const uint32_t e = (uint32_t)(drop + below) + 1u;   // the float of M * 2^(s - 149), s = drop + below, has exponent field s + 1
    return (e << 23) + (mant - 0x800000u);
}

}  // namespace statmc
