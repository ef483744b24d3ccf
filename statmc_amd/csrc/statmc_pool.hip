// statmc_pool.hip -- statmc_pool_statistics: the statistics of k x k blocks of fine pixels put together into one coarse pixel
// (include/statmc.h: the balanced tree of two-part combines over the block's k * k slots in Morton order).
//
// The arithmetic is include/statmc_device_api.hpp's: PixelStats::merge inside a lane, merge_lanes<G> across lanes -- there is no
// second copy of the formulas here.  The lane mapping:
//   - a lane owns a 2 x 2 sub-block of fine pixels -- slots 4 j .. 4 j + 3 of its block, j the sub-block's Morton index inside the
//     block -- loads the two pixel pairs (one dwordx2 per plane, row and channel pair where the planes allow it) and runs the
//     tree's first two levels on its own: s0.merge(s1), s2.merge(s3), s0.merge(s2);
//   - the G = k * k / 4 lanes of a block are consecutive lanes in Morton order of their sub-blocks, so merge_lanes<G> is the rest of
//     the tree (nothing for k = 2) and lane 0 of the group stores the coarse pixel;
//   - a wave holds 64 / G blocks that follow each other in x: 128, 64 or 32 fine pixels of 2, 4 or 8 rows.
// That is 3 / 4 + (log2 G) / 4 merges per fine pixel (0.75, 1.25, 1.75) where one lane per fine pixel would run 2, 4, 6.
// Every lane of a wave reaches merge_lanes: a lane whose sub-block or block lies past the film carries cleared states and skips
// only its loads and its store.  The entries of a call are walked one after the other, so a lane holds four states of ONE entry at
// a time (at most 4 x 16 dwords).
#include "statmc_device.h"
#include "statmc_pool_args.h"
#include "../../include/statmc_device_api.hpp"

namespace statmc {

namespace {

constexpr int kPoolBlock = 256;   // 4 waves; each wave works on a tile of its own

// One plane's values of two horizontally adjacent fine pixels, the first at pixel index px: t[0 .. C) and t[C .. 2 C).  A pixel
// that is not live (outside the film) reads nothing and gives zeros -- the cleared state.  vec: both are live and the pair moves as
// dwordx2 (the planes are 8-byte aligned and the film's width is even, so px * C is even).
template <int C>
__device__ __forceinline__ void pool_load2(const float *plane, long long px, bool live_a, bool live_b, bool vec, float (&t)[2 * C]) {
    const float *p = plane + px * C;
    if (vec) {
#pragma unroll
        for (int q = 0; q < C; q++) {
            const float2 x = reinterpret_cast<const float2 *>(p)[q];
            t[2 * q] = x.x;
            t[2 * q + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2 * C; j++) t[j] = (j < C ? live_a : live_b) ? p[j] : 0.f;
    }
}
// Fine pixels (x0, y) and (x0 + 1, y) of entry e into a and b.
template <int C, int MAXM, bool FILM>
__device__ __forceinline__ void pool_load_pair(const PoolEntry &e, long long px, bool live_a, bool live_b, bool vec,
                                               device::PixelStats<C, MAXM, FILM> &a, device::PixelStats<C, MAXM, FILM> &b) {
    float t[2 * C];
    if (vec) {
        const int2 n = *reinterpret_cast<const int2 *>(e.cnt_src + px);
        a.n = n.x;
        b.n = n.y;
    } else {
        a.n = live_a ? e.cnt_src[px] : 0;
        b.n = live_b ? e.cnt_src[px + 1] : 0;
    }
    pool_load2<C>(e.s[kPoolMean], px, live_a, live_b, vec, t);
#pragma unroll
    for (int c = 0; c < C; c++) a.st[c].mean = t[c], b.st[c].mean = t[C + c];
    if (MAXM >= 2) {
        pool_load2<C>(e.s[kPoolM2], px, live_a, live_b, vec, t);
#pragma unroll
        for (int c = 0; c < C; c++) a.st[c].m2 = t[c], b.st[c].m2 = t[C + c];
    }
    if (MAXM >= 3) {
        pool_load2<C>(e.s[kPoolM3], px, live_a, live_b, vec, t);
#pragma unroll
        for (int c = 0; c < C; c++) a.st[c].m3 = t[c], b.st[c].m3 = t[C + c];
    }
    if (FILM) {
        pool_load2<C>(e.s[kPoolFilmMean], px, live_a, live_b, vec, t);
#pragma unroll
        for (int c = 0; c < C; c++) a.st[c].fmean = t[c], b.st[c].fmean = t[C + c];
        if (e.s[kPoolFilmM2]) {
            pool_load2<C>(e.s[kPoolFilmM2], px, live_a, live_b, vec, t);
#pragma unroll
            for (int c = 0; c < C; c++) a.st[c].fm2 = t[c], b.st[c].fm2 = t[C + c];
        }
    }
}

// One entry, one lane.  (x0, y0): the lane's 2 x 2 sub-block; out: the coarse pixel, or -1 where the lane stores nothing.
template <int K, int C, int MAXM, bool FILM>
__device__ __forceinline__ void pool_entry(const PoolEntry &e, const PoolArgs &a, int x0, int y0, bool in_block, long long out) {
#pragma clang fp contract(off)
    using State = device::PixelStats<C, MAXM, FILM>;
    State s0, s1, s2, s3;
    s0.clear();
    s1.clear();
    s2.clear();
    s3.clear();
    const bool col0 = in_block && x0 < a.width, col1 = in_block && x0 + 1 < a.width;
    const bool row0 = y0 < a.height, row1 = y0 + 1 < a.height;
    const long long px = (long long)y0 * a.width + x0;
    if (col0 && row0) pool_load_pair<C, MAXM, FILM>(e, px, true, col1, a.vec != 0, s0, s1);
    if (col0 && row1) pool_load_pair<C, MAXM, FILM>(e, px + a.width, true, col1, a.vec != 0, s2, s3);
    // the tree's levels 1 and 2 (slots 4 j .. 4 j + 3), then the levels across the block's lanes
    s0.merge(s1);
    s2.merge(s3);
    s0.merge(s2);
    if constexpr (K > 2) device::merge_lanes<K * K / 4>(s0);
    if (out < 0) return;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const long long o = out * C + c;
        e.d[kPoolMean][o] = s0.st[c].mean;
        if (MAXM >= 2) e.d[kPoolM2][o] = s0.st[c].m2;
        if (MAXM >= 3) e.d[kPoolM3][o] = s0.st[c].m3;
        if (FILM) {
            e.d[kPoolFilmMean][o] = s0.st[c].fmean;
            if (e.d[kPoolFilmM2]) e.d[kPoolFilmM2][o] = s0.st[c].fm2;
        }
    }
    if (e.cnt_dst) e.cnt_dst[out] = s0.n;
    if constexpr (MAXM >= 3) {
        if (e.mean_corr) {   // the pre-pass of the pooled moments: PixelStats::store(t, pixel, ctx)'s lines, the bits of statmc_prepass
            const float tq = (a.ctx.flags & 1) ? 1.f : device::t_quantile(a.ctx, s0.n - 1);
#pragma unroll
            for (int c = 0; c < C; c++) {
                float mc, dc;
                device::prepass_elem(s0.n, tq, s0.st[c].mean, s0.st[c].m2, s0.st[c].m3, mc, dc, (a.ctx.flags & 2) != 0);
                e.mean_corr[out * C + c] = mc;
                e.disc[out * C + c] = dc;
            }
        }
    }
}

template <int K, int C, bool FILM>
__device__ __forceinline__ void pool_entry_moments(const PoolEntry &e, const PoolArgs &a, int x0, int y0, bool in_block, long long out) {
    if (e.moments == 3) pool_entry<K, C, 3, FILM>(e, a, x0, y0, in_block, out);
    else if (e.moments == 2) pool_entry<K, C, 2, FILM>(e, a, x0, y0, in_block, out);
    else pool_entry<K, C, 1, FILM>(e, a, x0, y0, in_block, out);
}

}  // namespace

// The (channels, max_moment, film planes) of an entry pick its instantiation; every choice is uniform over the launch.  An entry
// with a film_mean of its own and no film_m2 runs the two-plane chain with a zero film_m2 that is never stored: the mean line
// does not read it.
template <int K>
__global__ __launch_bounds__(kPoolBlock) void pool_stats_kernel(PoolArgs a) {
    constexpr int G = K * K / 4;      // lanes per block
    constexpr int BPW = 64 / G;       // blocks per wave, consecutive in x
    constexpr int H = K / 2;          // sub-blocks per block side
    const int lane = (int)(threadIdx.x & 63);
    const int tiles_x = (a.wc + BPW - 1) / BPW;
    const long long tile = (long long)blockIdx.x * (kPoolBlock / 64) + (threadIdx.x >> 6);
    if (tile >= (long long)tiles_x * a.hc) return;   // the whole wave leaves
    const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long long)ty * tiles_x);
    const int X = tx * BPW + lane / G, Y = ty;
    const int j = lane % G;           // the sub-block's Morton index in its block: x bits 0 and 2, y bits 1 and 3
    const int sx = (j & 1) | ((j >> 1) & 2), sy = ((j >> 1) & 1) | ((j >> 2) & 2);
    static_assert(H <= 4, "a sub-block index has two bits per axis");
    const bool in_block = X < a.wc;
    const int x0 = K * X + 2 * sx, y0 = K * Y + 2 * sy;
    const long long out = (in_block && j == 0) ? (long long)Y * a.wc + X : -1;
    for (int i = 0; i < a.n_entries; i++) {
        const PoolEntry e = a.e[i];   // a copy, not a reference into the by-value argument
        if (e.channels == 3) {
            if (e.film) pool_entry_moments<K, 3, true>(e, a, x0, y0, in_block, out);
            else pool_entry_moments<K, 3, false>(e, a, x0, y0, in_block, out);
        } else {
            if (e.film) pool_entry_moments<K, 1, true>(e, a, x0, y0, in_block, out);
            else pool_entry_moments<K, 1, false>(e, a, x0, y0, in_block, out);
        }
    }
}

template <int K>
static hipError_t launch_pool_k(const PoolArgs &a, hipStream_t s) {
    constexpr int BPW = 64 / (K * K / 4);
    const long long tiles = (long long)((a.wc + BPW - 1) / BPW) * a.hc;
    const long long grid = (tiles + kPoolBlock / 64 - 1) / (kPoolBlock / 64);
    hipLaunchKernelGGL(pool_stats_kernel<K>, dim3((unsigned)grid), dim3(kPoolBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pool(const PoolArgs &a, hipStream_t s) {
    if (a.k == 2) return launch_pool_k<2>(a, s);
    if (a.k == 4) return launch_pool_k<4>(a, s);
    return launch_pool_k<8>(a, s);
}

}  // namespace statmc
