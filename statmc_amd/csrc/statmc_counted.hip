// statmc_counted.hip -- statmc_accumulate_counted / statmc_accumulate_tiles_counted: a dense sample arena in which every pixel has
// its own sample count (gfx950).
//
// An adaptive renderer writes the same dense [S][H][W][C] arena (or [S][th][tw][C] tile block) as a uniform one and simply stops
// early on most pixels.  The arena stays as it is; an int32 film image says how many of its S planes are live for each pixel:
// c(p) = min(max(counts[p], 0), S), clamped BEFORE anything is derived from it -- no count becomes an address or reaches n
// unclamped.  Sample s of pixel p is folded iff s < c(p), in ascending s, which leaves per pixel the bits the tile entry leaves
// for a 1 x 1 tile of c(p) samples.  No sort, no tables, no workspace.
//
//   ownership   vector path: a lane owns 4 consecutive pixels of one stat type (accumulate_lane's shape), reads its 4 counts with
//               one 16-byte load, clamps them, and leaves at once where all four are 0 -- the group keeps every bit.
//   prefix      s < min of the 4 counts: every pixel of the lane is live.  Where the wave's lanes all hold one count per group
//               (every film that was sampled uniformly so far) this is the uniform fold: one reciprocal per sample.
//   tail        [min, max): the packed fold runs on all 4 pixels and a select per pixel keeps the state of the ones that have
//               ended -- predication, no branch per element.  What a dead slot holds (NaN, inf, uninitialised bits) goes
//               through the arithmetic and is dropped by the select.
//   walk        ends at the lane's max; a wave ends at its longest lane.  Loads run U samples ahead of the fold, into registers;
//               a lane past its max issues none.  (The LDS-DMA ring is a cooperative walk whose transfers per row must not
//               depend on the lane: not used here.)
//   epilogue    one quantile per pixel; not stored for pixels with c(p) == 0.
//   element     unaligned images, ragged groups, tiles whose rows do not split into 4-pixel groups: one pixel at a time through
//   path        statmc::device::add_sample, the same bits.
//
// The arithmetic is add_sample / add_sample2 (include/statmc_device_api.hpp, statmc_accumulate_fold.h) and prepass_elem /
// t_quantile: nothing is restated.  Wasted traffic: a wave whose lanes stop at different s still pulls whole memory lines of the
// planes up to its longest lane, so the cost follows the spatial coherence of the counts, not only their sum.

#include <type_traits>

#include "statmc_device.h"

#include "../../include/statmc_device_api.hpp"
#include "statmc_accumulate_fold.h"

namespace statmc {

namespace {

using device::ElemState;
using device::add_sample;
using device::prepass_elem;
using device::refined_rcp;

constexpr int kCntBlock = 256;
constexpr int kCntWaves = 2;     // waves per SIMD the kernels are compiled for (the radiance tail holds a state, its copy and 2 U rows)
// sample rows in flight per lane (x 2: current + next group), as accumulate_lane has them
constexpr int kCntURgb = 3, kCntUF = 6;
// ... and under per-pixel counts, where an RGB lane also holds the copy of the state the select falls back to
constexpr int kCntURgbLive = 2;
constexpr int kCntPairGroup = 3;
typedef _Float16 cnt_half4 __attribute__((ext_vector_type(4)));

// THE clamp: the only way a count enters the kernels
__device__ __forceinline__ int live_count(int c, int S) { return min(max(c, 0), S); }
// the quantile the epilogue hands prepass_elem for a pixel of n samples (flags 1: Welch, t = 1)
__device__ __forceinline__ float counted_quantile(const statmc_prepass_context &ctx, int n) {
    return (ctx.flags & 1) ? 1.f : device::t_quantile(ctx, n - 1);
}

// One pixel, scalar accesses.  Sample s of channel c is at sp[s * stride + c]; cnt = the pixel's live count (clamped).
template <int C, int MAXM, bool TRANSFORM, typename ST>
__device__ __forceinline__ void counted_pixel(const AccumulateType &t, const statmc_prepass_context &ctx, long long p, int cnt, const ST *sp,
                                              long long stride) {
    if (cnt == 0) return;                          // the pixel keeps every bit of every image
    const int n0 = t.n[p];
    float *const pre_mc = MAXM >= 3 ? t.mean_corr : nullptr;
    float *const pre_dc = MAXM >= 3 ? t.disc : nullptr;
    for (int c = 0; c < C; c++) {
        const long long e = p * C + c;
        ElemState st = {t.mean[e], MAXM >= 2 ? t.m2[e] : 0.f, MAXM >= 3 ? t.m3[e] : 0.f, TRANSFORM ? t.film_mean[e] : 0.f,
                        TRANSFORM ? t.film_m2[e] : 0.f};
        for (int s = 0; s < cnt; s++) {
            const float nf = (float)(n0 + s + 1);
            add_sample<MAXM, TRANSFORM>(st, nf, refined_rcp(nf), (float)sp[(long long)s * stride + c]);
        }
        t.mean[e] = st.mean;
        if (MAXM >= 2) t.m2[e] = st.m2;
        if (MAXM >= 3) t.m3[e] = st.m3;
        if (TRANSFORM) {
            t.film_mean[e] = st.fmean;
            t.film_m2[e] = st.fm2;
        }
        if (MAXM >= 3 && pre_mc != nullptr) {
            const int ni = n0 + cnt;
            float m, d;
            prepass_elem(ni, counted_quantile(ctx, ni), st.mean, st.m2, st.m3, m, d, (ctx.flags & 2) != 0);
            pre_mc[e] = m;
            pre_dc[e] = d;
        }
    }
    t.n[p] = n0 + cnt;
}

// The lane's 4 consecutive pixels starting at film pixel p0 (16-byte aligned planes and counts): cnt4 points at their counts,
// sample s of the lane's elements is at sp + s * stride (4 C consecutive elements), S is the arena's capacity.
template <int C, int MAXM, bool TRANSFORM, typename ST>
__device__ __forceinline__ void counted_lane(const AccumulateType &t, const statmc_prepass_context &ctx, long long p0, const int32_t *cnt4,
                                             const ST *sp, long long stride, int S) {
    constexpr bool kHalf = !std::is_same<ST, float>::value;
    constexpr int NE = 4 * C;
    const int4 raw = *reinterpret_cast<const int4 *>(cnt4);
    const int c[4] = {live_count(raw.x, S), live_count(raw.y, S), live_count(raw.z, S), live_count(raw.w, S)};
    const int c_min = min(min(c[0], c[1]), min(c[2], c[3])), c_max = max(max(c[0], c[1]), max(c[2], c[3]));
    if (c_max == 0) return;                        // the group keeps every bit of every image
    const long long e0 = p0 * C;
    float *const pre_mc = MAXM >= 3 ? t.mean_corr : nullptr;      // (read before the first store, as in accumulate_lane)
    float *const pre_dc = MAXM >= 3 ? t.disc : nullptr;
    PairState st[NE / 2];   // element pairs (2 i, 2 i + 1) of the lane's 4 C consecutive elements
    const int4 n4 = *reinterpret_cast<const int4 *>(t.n + p0);
    const int n0[4] = {n4.x, n4.y, n4.z, n4.w};
    load_plane<C>(st, &PairState::mean, t.mean + e0);
    load_plane<C, MAXM >= 2>(st, &PairState::m2, t.m2 + e0);
    load_plane<C, MAXM >= 3>(st, &PairState::m3, t.m3 + e0);
    load_plane<C, TRANSFORM>(st, &PairState::fmean, t.film_mean + e0);
    load_plane<C, TRANSFORM>(st, &PairState::fm2, t.film_m2 + e0);
    constexpr int U_SAME = C == 3 ? kCntURgb : kCntUF, U_LIVE = C == 3 ? kCntURgbLive : kCntUF;
    constexpr int G = C == 3 ? kCntPairGroup : 2;
    // (C = 3: plain loads, they coalesce through the cache; C = 1 streams with non-temporal loads -- accumulate_lane's finding)
    auto load_sample = [&](vfloat4 (&dst)[C], const ST *src) {
        if constexpr (kHalf) {
            cnt_half4 h[C];
#pragma unroll
            for (int k = 0; k < C; k++)
                h[k] = C == 1 ? __builtin_nontemporal_load(reinterpret_cast<const cnt_half4 *>(src + 4 * k)) : *reinterpret_cast<const cnt_half4 *>(src + 4 * k);
#pragma unroll
            for (int k = 0; k < C; k++) dst[k] = __builtin_convertvector(h[k], vfloat4);
        } else {
#pragma unroll
            for (int k = 0; k < C; k++)
                dst[k] = C == 1 ? __builtin_nontemporal_load(reinterpret_cast<const vfloat4 *>(src + 4 * k)) : *reinterpret_cast<const vfloat4 *>(src + 4 * k);
        }
    };
    // every pixel of the lane is live and holds the same count: one count conversion and one refined reciprocal per sample
    auto fold_same = [&](const vfloat4 (&q)[C], int s) {
        const float nf0 = (float)(n0[0] + s + 1);
        const float rc0 = refined_rcp(nf0);
        v2f nf2[NE / 2], rc2[NE / 2], smp2[NE / 2];
#pragma unroll
        for (int i = 0; i < NE / 2; i++) {   // elements 2 i and 2 i + 1
            nf2[i] = v2f{nf0, nf0};
            rc2[i] = v2f{rc0, rc0};
            smp2[i] = v2f{q[i >> 1][2 * (i & 1)], q[i >> 1][2 * (i & 1) + 1]};
        }
#pragma unroll
        for (int g = 0; g < NE / 2; g += G) add_sample2<G, MAXM, TRANSFORM>(st + g, nf2 + g, rc2 + g, smp2 + g);
    };
    // per-pixel counts: the packed fold on all 4 pixels, then every field of a pixel with c <= s takes its old bits back
    auto fold_live = [&](const vfloat4 (&q)[C], int s) {
        float nf[4], rc[4];
        bool live[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            nf[p] = (float)(n0[p] + s + 1);
            rc[p] = refined_rcp(nf[p]);
            live[p] = s < c[p];
        }
#pragma unroll
        for (int g = 0; g < NE / 2; g += G) {
            PairState old[G];
            v2f nf2[G], rc2[G], smp2[G];
#pragma unroll
            for (int i = 0; i < G; i++) {
                const int ea = 2 * (g + i), eb = ea + 1;
                old[i] = st[g + i];
                nf2[i] = v2f{nf[ea / C], nf[eb / C]};
                rc2[i] = v2f{rc[ea / C], rc[eb / C]};
                smp2[i] = v2f{q[ea >> 2][ea & 3], q[eb >> 2][eb & 3]};
            }
            add_sample2<G, MAXM, TRANSFORM>(st + g, nf2, rc2, smp2);
#pragma unroll
            for (int i = 0; i < G; i++) {
                const int ea = 2 * (g + i), eb = ea + 1;
                const bool la = live[ea / C], lb = live[eb / C];
                PairState &x = st[g + i];
                x.mean = v2f{la ? x.mean.x : old[i].mean.x, lb ? x.mean.y : old[i].mean.y};
                if (MAXM >= 2) x.m2 = v2f{la ? x.m2.x : old[i].m2.x, lb ? x.m2.y : old[i].m2.y};
                if (MAXM >= 3) x.m3 = v2f{la ? x.m3.x : old[i].m3.x, lb ? x.m3.y : old[i].m3.y};
                if (TRANSFORM) {
                    x.fmean = v2f{la ? x.fmean.x : old[i].fmean.x, lb ? x.fmean.y : old[i].fmean.y};
                    x.fm2 = v2f{la ? x.fm2.x : old[i].fm2.x, lb ? x.fm2.y : old[i].fm2.y};
                }
            }
        }
    };
    // Software-pipelined walk over samples [s0, s1): the loads of the next U samples are issued before the current U are folded.
    // Nothing is loaded at or beyond s1 <= c_max <= S.
    auto walk = [&](auto depth, int s0, int s1, auto fold) {
        constexpr int U = decltype(depth)::value;
        vfloat4 cur[U][C], nxt[U][C];
        const int s_main = s1 - (s1 - s0) % U;
        if (s_main > s0) {
#pragma unroll
            for (int u = 0; u < U; u++) load_sample(cur[u], sp + (long long)(s0 + u) * stride);
        }
        for (int s = s0; s < s_main; s += U) {
            if (s + U < s_main) {
#pragma unroll
                for (int u = 0; u < U; u++) load_sample(nxt[u], sp + (long long)(s + U + u) * stride);
            }
#pragma unroll
            for (int u = 0; u < U; u++) fold(cur[u], s + u);
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < C; k++) cur[u][k] = nxt[u][k];
        }
        for (int s = s_main; s < s1; s++) {   // remainder
            vfloat4 q[C];
            load_sample(q, sp + (long long)s * stride);
            fold(q, s);
        }
    };
    // wave-uniform choice: the uniform fold for the prefix only when every lane of the wave that has work qualifies
    const bool lane_same = n0[0] == n0[1] && n0[1] == n0[2] && n0[2] == n0[3];
    if (__builtin_amdgcn_ballot_w64(!lane_same) == 0) walk(std::integral_constant<int, U_SAME>{}, 0, c_min, fold_same);
    else walk(std::integral_constant<int, U_LIVE>{}, 0, c_min, fold_live);
    walk(std::integral_constant<int, U_LIVE>{}, c_min, c_max, fold_live);
    store_plane<C>(t.mean + e0, st, &PairState::mean);
    store_plane<C, MAXM >= 2>(t.m2 + e0, st, &PairState::m2);
    store_plane<C, MAXM >= 3>(t.m3 + e0, st, &PairState::m3);
    store_plane<C, TRANSFORM>(t.film_mean + e0, st, &PairState::fmean);
    store_plane<C, TRANSFORM>(t.film_m2 + e0, st, &PairState::fm2);
    const int n_out[4] = {n0[0] + c[0], n0[1] + c[1], n0[2] + c[2], n0[3] + c[3]};
    store_counts(t.n + p0, n_out);
    if constexpr (MAXM >= 3) {
        if (pre_mc != nullptr) {
            // the pre-pass of the moments just written, one quantile per pixel (store_prepass's NC = 4 form); a pixel without a
            // live sample keeps its mean_corr / discriminator: whole 16-byte stores only where all 4 pixels are live
            float tq[4];
#pragma unroll
            for (int p = 0; p < 4; p++) tq[p] = counted_quantile(ctx, n_out[p]);
#pragma unroll
            for (int k = 0; k < C; k++) {
                vfloat4 mc, dc;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int e = 4 * k + j, px = e / C;
                    float m, d;
                    prepass_elem(n_out[px], tq[px], st[e >> 1].mean[e & 1], st[e >> 1].m2[e & 1], st[e >> 1].m3[e & 1], m, d, (ctx.flags & 2) != 0);
                    mc[j] = m;
                    dc[j] = d;
                }
                if (c_min > 0) {
                    *reinterpret_cast<vfloat4 *>(pre_mc + e0 + 4 * k) = mc;
                    *reinterpret_cast<vfloat4 *>(pre_dc + e0 + 4 * k) = dc;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (c[(4 * k + j) / C] > 0) {
                            pre_mc[e0 + 4 * k + j] = mc[j];
                            pre_dc[e0 + 4 * k + j] = dc[j];
                        }
                    }
                }
            }
        }
    }
}

// From a run-time descriptor to the compile-time shape of its walk: f(C, MAXM, TRANSFORM), each an integral constant.
template <typename F>
__device__ __forceinline__ void counted_dispatch_type(const AccumulateType &t, F f) {
    auto moments = [&](auto c) {
        if (t.transform) {
            if (t.max_moment >= 3) f(c, std::integral_constant<int, 3>{}, std::true_type{});
            else if (t.max_moment == 2) f(c, std::integral_constant<int, 2>{}, std::true_type{});
            else f(c, std::integral_constant<int, 1>{}, std::true_type{});
        } else {
            if (t.max_moment >= 3) f(c, std::integral_constant<int, 3>{}, std::false_type{});
            else if (t.max_moment == 2) f(c, std::integral_constant<int, 2>{}, std::false_type{});
            else f(c, std::integral_constant<int, 1>{}, std::false_type{});
        }
    };
    if (t.channels == 3) moments(std::integral_constant<int, 3>{});
    else moments(std::integral_constant<int, 1>{});
}

// Film-major: groups of 4 consecutive pixels of the entry, one per lane, grid-stride over the entry's workgroups.
template <int C, int MAXM, bool TRANSFORM, bool VEC, typename ST>
__device__ __forceinline__ void counted_type(const AccumulateType &t, const int32_t *counts, const statmc_prepass_context &ctx, long long blk,
                                             long long nblk) {
    const ST *const samples = reinterpret_cast<const ST *>(t.samples);   // (t.stride and t.n_elems count elements, whatever their width)
    const long long n_px = t.n_elems / C;
    const long long n_groups = (n_px + 3) >> 2;
    const long long n_full = VEC ? (n_px >> 2) : 0;          // complete 4-pixel groups: the vector path's share
    const int S = t.n_samples;
    for (long long g = blk * kCntBlock + threadIdx.x; g < n_groups; g += nblk * kCntBlock) {
        const long long p0 = g << 2;
        if (g < n_full) {
            if constexpr (VEC) counted_lane<C, MAXM, TRANSFORM, ST>(t, ctx, p0, counts + p0, samples + p0 * C, t.stride, S);
        } else {
            for (long long p = p0; p < n_px && p < p0 + 4; p++)
                counted_pixel<C, MAXM, TRANSFORM, ST>(t, ctx, p, live_count(counts[p], S), samples + p * C, t.stride);
        }
    }
}

}  // namespace

// One pass per workgroup, entries round-robin: block b serves entry b % n_types (the shape of accumulate_half_kernel).
template <bool VEC>
__global__ __launch_bounds__(kCntBlock, kCntWaves) void accumulate_counted_kernel(AccumulateCountedArgs a) {
    const int ti = blockIdx.x % a.n_types;
    const AccumulateType t = a.t[ti];                                      // (a copy, not a reference into the by-value argument)
    const int32_t *const counts = a.counts[ti];
    const statmc_prepass_context ctx = a.ctx;
    const long long blk = blockIdx.x / a.n_types, nblk = gridDim.x / a.n_types;
    if ((a.half_mask >> ti) & 1) {
        counted_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
            counted_type<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, VEC, _Float16>(t, counts, ctx, blk, nblk);
        });
    } else {
        counted_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
            counted_type<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, VEC, float>(t, counts, ctx, blk, nblk);
        });
    }
}

namespace {

// One tile of one type, one wave: the tile's block starts at element offset off * C and holds S planes of th x tw pixels; a
// pixel's count is read from the film image at its film coordinates.
template <int C, int MAXM, bool TRANSFORM, typename ST>
__device__ __forceinline__ void counted_tile(const AccumulateType &t, const AccumulateTilesCountedArgs &a, bool vec, int x0, int y0, int tw,
                                             int th, long long off, int S) {
    const int lane = threadIdx.x & 63;
    const int npx = tw * th;
    const ST *base = reinterpret_cast<const ST *>(t.samples) + off * C;
    const long long stride = (long long)npx * C;
    // rows split into 16-byte aligned 4-pixel groups: tile width, tile origin, image width and the block's offset are all
    // multiples of 4 (and the images, the arena and the counts image themselves aligned: vec)
    const bool fast = vec && ((tw | x0 | a.width) & 3) == 0 && (off & 3) == 0;
    if (fast) {
        const int n_g = npx >> 2;
        for (int g = lane; g < n_g; g += 64) {
            const int i = g << 2, row = i / tw, col = i - row * tw;
            const long long p0 = (long long)(y0 + row) * a.width + x0 + col;
            counted_lane<C, MAXM, TRANSFORM, ST>(t, a.ctx, p0, a.counts + p0, base + (long long)i * C, stride, S);
        }
    } else {
        for (int i = lane; i < npx; i += 64) {
            const int row = i / tw, col = i - row * tw;
            const long long p = (long long)(y0 + row) * a.width + x0 + col;
            counted_pixel<C, MAXM, TRANSFORM, ST>(t, a.ctx, p, live_count(a.counts[p], S), base + (long long)i * C, stride);
        }
    }
}

}  // namespace

// accumulate_tiles_kernel's item walk in its default order: one wave per (tile, type), a workgroup = four consecutive tiles of ONE
// type, workgroups round-robin over the types.
__global__ __launch_bounds__(kCntBlock, kCntWaves) void accumulate_tiles_counted_kernel(AccumulateTilesCountedArgs a) {
    const long long n_items = (((long long)a.n_tiles + 3) >> 2) * 4 * a.n_types;
    const long long n_waves = (long long)gridDim.x * (kCntBlock / 64);
    for (long long item = (long long)blockIdx.x * (kCntBlock / 64) + (threadIdx.x >> 6); item < n_items; item += n_waves) {
        const long long q = item >> 2;
        const int ti = __builtin_amdgcn_readfirstlane((int)(q % a.n_types));
        const int tile = __builtin_amdgcn_readfirstlane((int)(q / a.n_types) * 4 + (int)(item & 3));
        if (tile >= a.n_tiles) continue;
        const int x0 = a.tile_bounds[4 * tile], y0 = a.tile_bounds[4 * tile + 1];
        const int x1 = a.tile_bounds[4 * tile + 2], y1 = a.tile_bounds[4 * tile + 3];
        const int S = a.tile_samples[tile];
        if (S <= 0 || x1 <= x0 || y1 <= y0) continue;
        if (x0 < 0 || y0 < 0 || x1 > a.width || y1 > a.height) continue;     // never a count from outside the film image
        const AccumulateType &t = a.t[ti];
        const bool vec = (a.vec >> ti) & 1;
        const long long off = a.tile_offsets[tile];
        if ((a.half_mask >> ti) & 1) {
            counted_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
                counted_tile<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, _Float16>(t, a, vec, x0, y0, x1 - x0, y1 - y0, off, S);
            });
        } else {
            counted_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
                counted_tile<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, float>(t, a, vec, x0, y0, x1 - x0, y1 - y0, off, S);
            });
        }
    }
}

hipError_t launch_accumulate_counted(const AccumulateCountedArgs &a, hipStream_t s, int *path) {
    // the vector path: what the uncounted launch asks of every entry, plus a 16-byte aligned counts image
    bool vec = true;
    long long max_groups = 1;
    for (int i = 0; i < a.n_types; i++) {
        vec = vec && acc_type_vectorizable(a.t[i], (a.half_mask >> i) & 1, true) && aligned16(a.counts[i]);
        const long long groups = (a.t[i].n_elems / a.t[i].channels + 3) / 4;
        if (groups > max_groups) max_groups = groups;
    }
    const long long units = (max_groups + kCntBlock - 1) / kCntBlock;     // workgroups that cover the largest entry once
    const dim3 grid((unsigned)(units * a.n_types)), block(kCntBlock);
    if (vec) hipLaunchKernelGGL((accumulate_counted_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((accumulate_counted_kernel<false>), grid, block, 0, s, a);
    if (path) *path = vec ? 1 : 2;
    return hipGetLastError();
}

hipError_t launch_accumulate_tiles_counted(const AccumulateTilesCountedArgs &a_in, hipStream_t s, int *path) {
    AccumulateTilesCountedArgs a = a_in;
    a.vec = 0;
    for (int i = 0; i < a.n_types; i++)      // (a film whose width is no multiple of 4 has no tile with 16-byte aligned rows)
        if (acc_type_vectorizable(a.t[i], (a.half_mask >> i) & 1, false) && aligned16(a.counts) && (a.width & 3) == 0) a.vec |= 1 << i;
    // one wave per item; at most 8 workgroups per CU, walking the items with a grid stride (launch_accumulate_tiles' rule)
    const long long items = (((long long)a.n_tiles + 3) >> 2) * 4 * a.n_types;
    const bool big = a.n_tiles >= 16384;
    long long blocks = (items * 64 + kCntBlock - 1) / kCntBlock;
    const long long cap = big ? (1ll << 30) : 256 * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(accumulate_tiles_counted_kernel, dim3((unsigned)blocks), dim3(kCntBlock), 0, s, a);
    if (path) *path = a.vec == (1 << a.n_types) - 1 ? 1 : 2;
    return hipGetLastError();
}

}  // namespace statmc
