// statmc_score_window_args.h -- what statmc_score_window (include/statmc.h) checks and fills on the host, each rule stated once, the
// tile geometry and the argument block its kernel takes (statmc_score_window.hip).  Pure functions of their arguments: no HIP call,
// no device, no global or thread-local state; nothing is read through a pointer (the image pointers are compared as numbers).
// true: valid; false: the caller's buffer names the argument (the code is STATMC_ERR_INVALID throughout).  The key, the message
// buffer and the pointer helpers are statmc_select_args.h's.  Host-only: tests/cpp/test_score_window_args.cpp compiles this header
// with nothing but include/statmc.h behind it, with and without sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/statmc.h"
#include "statmc_select_args.h"

namespace statmc {

// ---- the tile.  A workgroup owns kWindowTile x kWindowTile outputs and stages them with a halo of `radius` keys
// to every side: side = kWindowTile + 2 radius rows of `side` keys (array A, pitch `side`: lanes run along x).  The row pass
// leaves its result transposed in array B, kWindowTile rows (one per output column) of `side` keys at an odd pitch: 32 lanes that
// step by it land on 32 banks.  Both arrays are dynamic LDS, sized by the radius of the call.
constexpr int kWindowTile = 32;
constexpr int kWindowBlock = 256;                // 4 waves; a wave owns whole rows of A, then whole rows of B
constexpr int kWindowQuad = 4;                   // consecutive pixels of one dwordx4
constexpr int window_side(int radius) { return kWindowTile + 2 * radius; }
constexpr int window_pitch_b(int radius) { return window_side(radius) | 1; }
constexpr size_t window_lds_bytes(int radius) {
    return (size_t)(window_side(radius) * window_side(radius) + kWindowTile * window_pitch_b(radius)) * sizeof(uint32_t);
}
static_assert(window_lds_bytes(STATMC_SCORE_WINDOW_MAX_RADIUS) == 49280, "96 x 96 keys and 32 x 97 row results: 48.1 KiB at radius 32");
static_assert(window_lds_bytes(STATMC_SCORE_WINDOW_MAX_RADIUS) <= 64 * 1024, "the largest radius fits the LDS a workgroup may have");
static_assert(window_side(STATMC_SCORE_WINDOW_MAX_RADIUS) <= 2 * 64, "a wave holds a row of either array in two registers per lane");
constexpr uint32_t window_identity(int op) { return op == STATMC_SCORE_WINDOW_MIN ? 0xFFFFFFFFu : 0u; }   // of a tap outside the film

struct ScoreWindowArgs {
    const float *score;
    float *out;
    int width, height;
    int op, radius;
    int vec_in, vec_out;         // score / out 16-byte aligned: quads of the film's linear index move as dwordx4
    unsigned tiles_x, tiles_y;
    unsigned lds_bytes;
};

// statmc_score_window, in this order: the film size, NULL pointers, alignment, op, radius, out over score.
inline bool check_score_window_call(uint16_t width, uint16_t height, const float *score, int op, int radius, const float *out, SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!out) return select_refuse(m, "null out");
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    if (select_misaligned(out, 4)) return select_refuse(m, "out is not 4-byte aligned");
    if (op != STATMC_SCORE_WINDOW_MAX && op != STATMC_SCORE_WINDOW_MIN)
        return select_refuse(m, "op = %d: STATMC_SCORE_WINDOW_MAX (%d) or STATMC_SCORE_WINDOW_MIN (%d)", op, STATMC_SCORE_WINDOW_MAX, STATMC_SCORE_WINDOW_MIN);
    if (radius < 0 || radius > STATMC_SCORE_WINDOW_MAX_RADIUS) return select_refuse(m, "radius = %d: 0 to %d", radius, STATMC_SCORE_WINDOW_MAX_RADIUS);
    const size_t px = (size_t)width * height * 4;
    if (select_ranges_overlap(out, px, score, px)) return select_refuse(m, "out overlaps score: there is no in-place mode");
    return true;
}

// The kernel's argument block of a call that passed check_score_window_call.
inline void fill_score_window_args(ScoreWindowArgs &a, uint16_t width, uint16_t height, const float *score, int op, int radius, float *out) {
    a = ScoreWindowArgs{};
    a.score = score, a.out = out;
    a.width = width, a.height = height;
    a.op = op, a.radius = radius;
    a.vec_in = !select_misaligned(score, 16);
    a.vec_out = !select_misaligned(out, 16);
    a.tiles_x = (unsigned)((width + kWindowTile - 1) / kWindowTile);
    a.tiles_y = (unsigned)((height + kWindowTile - 1) / kWindowTile);
    a.lds_bytes = (unsigned)window_lds_bytes(radius);
}

}  // namespace statmc
