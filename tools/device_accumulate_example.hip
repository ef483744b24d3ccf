// device_accumulate_example.hip -- a renderer's kernel folding its samples into StatMC's statistics itself
// (include/statmc_device_api.hpp), built into tools/bin/libstatmc_device_example.so with hipcc's DEFAULT floating-point flags
// (-ffp-contract=fast-honor-pragmas): the header's bits must not depend on them.  The launchers, extern "C":
//
//   fold_arena  one thread per pixel folds a film-major arena ([S][H][W][C] fp32, statmc_accumulate's input) through
//               PixelStats -- the bits of statmc_accumulate on the same arena (tests/test_device_api_gpu.py)
//   fold_arena_slots  the same arena with every pixel's samples dealt to several slots: each slot folds its share, the slots
//               are merged in slot order (PixelStats::merge) and the pixel is stored once -- the bits of the slots' states
//               combined by statmc_combine_many (tests/test_combine_many_gpu.py)
//   gen_arena   a stand-in for a path tracer: one counter-based hash per (pixel, sample) gives the five G-buffer / radiance
//               values of the flagship configuration (film.STAT_TYPES: radiance, normal, albedo, depth, material id; 11
//               channels), written to one arena per type -- what feeds statmc_accumulate today
//   gen_fold    the same values, folded straight into the statistics in registers: no arena
//   fold_arena_lanes, fold_arena_waves, fold_arena_lanes_waves  fold_arena_slots with the slots of a pixel held by the lanes of
//               a wave, by the waves of a workgroup, or both: merged by the header's merge_lanes / merge_waves -- the bits of
//               the slots' states combined by two-part statmc_combine_statistics calls in the header's tree order
//               (tests/test_device_reduce_gpu.py)
//   gen_fold_lanes  gen_fold with G lanes per pixel
//   fold_arena_records  fold_arena for a kernel that does not own its pixels: one thread per pixel folds the arena's samples from
//               clear() and writes the state as a record (PixelStats::write_record) instead of storing it -- what
//               statmc_combine_records merges into a film (tests/test_state_records_gpu.py)
//
// Every launcher returns 0 or a negative STATMC_ERR_* (include/statmc.h), and only enqueues on `stream`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "statmc.h"
#include "statmc_device_api.hpp"

using statmc::device::merge_lanes;
using statmc::device::merge_waves;
using statmc::device::merge_waves_lds_bytes;
using statmc::device::PixelStats;

namespace {

constexpr int kBlock = 256;

inline int grid_for(long long n_px) { return (int)((n_px + kBlock - 1) / kBlock); }

int launched() { return hipGetLastError() == hipSuccess ? STATMC_OK : STATMC_ERR_HIP; }

// ------------------------------------------------------------------ fold_arena
template <int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(kBlock) void fold_arena_kernel(statmc_stat_type t, long long n_px, const float *arena, int n_samples,
                                                            statmc_prepass_context ctx, int with_prepass) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_px) return;
    PixelStats<C, MAXM, TRANSFORM> ps;
    ps.load(t, p);
    for (int s = 0; s < n_samples; s++) {
        const float *q = arena + ((long long)s * n_px + p) * C;
        float smp[C];
#pragma unroll
        for (int c = 0; c < C; c++) smp[c] = q[c];
        ps.add(smp);
    }
    if constexpr (MAXM >= 3) {
        if (with_prepass) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// ------------------------------------------------------------------ fold_arena_records
// The partial state of a pixel this kernel does not own: folded from clear(), never stored; record p -- state_dwords<C, MAXM,
// TRANSFORM>() dwords at records + p * D -- goes to statmc_combine_records with pixels[p] = p.
template <int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(kBlock) void fold_arena_records_kernel(long long n_px, const float *arena, int n_samples, int32_t *records) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_px) return;
    PixelStats<C, MAXM, TRANSFORM> ps;
    ps.clear();
    for (int s = 0; s < n_samples; s++) {
        const float *q = arena + ((long long)s * n_px + p) * C;
        float smp[C];
#pragma unroll
        for (int c = 0; c < C; c++) smp[c] = q[c];
        ps.add(smp);
    }
    ps.write_record(records + p * statmc::device::state_dwords<C, MAXM, TRANSFORM>());
}
template <int C>
int records_dispatch(int transform, int max_moment, long long n_px, const float *arena, int n_samples, int32_t *records, hipStream_t s) {
#define STATMC_RECORDS(m, t)                                                                                                        \
    hipLaunchKernelGGL((fold_arena_records_kernel<C, m, t>), dim3(grid_for(n_px)), dim3(kBlock), 0, s, n_px, arena, n_samples, records); \
    return launched();
    if (transform) {
        if (max_moment == 3) { STATMC_RECORDS(3, true) }
        if (max_moment == 2) { STATMC_RECORDS(2, true) }
        STATMC_RECORDS(1, true)
    }
    if (max_moment == 3) { STATMC_RECORDS(3, false) }
    if (max_moment == 2) { STATMC_RECORDS(2, false) }
    STATMC_RECORDS(1, false)
#undef STATMC_RECORDS
}

// ------------------------------------------------------------------ fold_arena_slots
// A renderer that keeps several samples of a pixel in flight: slot k of pixel p owns the samples bounds[k][p] .. bounds[k + 1][p]
// - 1 of the arena (bounds: [n_slots + 1][n_px] int32, non-decreasing per pixel; a slot may own none).  Slot 0 folds into the
// pixel's stored state, every other slot into a cleared state of its own; the slots are merged in slot order -- a left fold,
// the bits of statmc_combine_many over the slots' states -- and the pixel is stored once.
template <int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(kBlock) void fold_slots_kernel(statmc_stat_type t, long long n_px, const float *arena, const int32_t *bounds,
                                                            int n_slots, statmc_prepass_context ctx, int with_prepass) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_px) return;
    PixelStats<C, MAXM, TRANSFORM> ps;
    ps.load(t, p);
    for (int k = 0; k < n_slots; k++) {
        PixelStats<C, MAXM, TRANSFORM> slot;
        slot.clear();
        PixelStats<C, MAXM, TRANSFORM> &into = k == 0 ? ps : slot;
        const int s1 = bounds[(long long)(k + 1) * n_px + p];
        for (int s = bounds[(long long)k * n_px + p]; s < s1; s++) {
            const float *q = arena + ((long long)s * n_px + p) * C;
            float smp[C];
#pragma unroll
            for (int c = 0; c < C; c++) smp[c] = q[c];
            into.add(smp);
        }
        if (k > 0) ps.merge(slot);
    }
    if constexpr (MAXM >= 3) {
        if (with_prepass) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// bounds == NULL: fold_arena_kernel over n_samples; otherwise fold_slots_kernel over n_slots
template <int C, int MAXM, bool TRANSFORM>
int launch_fold(const statmc_stat_type &t, long long n_px, const float *arena, int n_samples, const statmc_prepass_context *ctx,
                hipStream_t s, const int32_t *bounds = nullptr, int n_slots = 0) {
    const statmc_prepass_context c = ctx ? *ctx : statmc_prepass_context{nullptr, 0, 0};
    if (bounds) {
        hipLaunchKernelGGL((fold_slots_kernel<C, MAXM, TRANSFORM>), dim3(grid_for(n_px)), dim3(kBlock), 0, s, t, n_px, arena, bounds,
                           n_slots, c, ctx ? 1 : 0);
        return launched();
    }
    hipLaunchKernelGGL((fold_arena_kernel<C, MAXM, TRANSFORM>), dim3(grid_for(n_px)), dim3(kBlock), 0, s, t, n_px, arena, n_samples, c,
                       ctx ? 1 : 0);
    return launched();
}

template <int C>
int fold_dispatch(const statmc_stat_type &t, long long n_px, const float *arena, int n_samples, const statmc_prepass_context *ctx,
                  hipStream_t s, const int32_t *bounds = nullptr, int n_slots = 0) {
    if (t.transform) {
        if (t.max_moment == 3) return launch_fold<C, 3, true>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
        if (t.max_moment == 2) return launch_fold<C, 2, true>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
        return launch_fold<C, 1, true>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
    }
    if (t.max_moment == 3) return launch_fold<C, 3, false>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
    if (t.max_moment == 2) return launch_fold<C, 2, false>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
    return launch_fold<C, 1, false>(t, n_px, arena, n_samples, ctx, s, bounds, n_slots);
}

// ------------------------------------------------------------------ fold_arena_lanes / fold_arena_waves / fold_arena_lanes_waves
// The slots of fold_slots_kernel held by different threads: slot k of pixel p still owns the samples bounds[k][p] ..
// bounds[k + 1][p] - 1, slot 0 folds into the pixel's stored state and every other slot into a cleared state of its own.  The
// slots then meet through the header's reductions -- a balanced tree, NOT fold_slots_kernel's left fold -- and slot 0 stores.
// A thread whose pixel lies past the film takes part in the reduction with a cleared state: it skips its loads and its store
// only (every lane executes merge_lanes, every wave merge_waves).
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void fold_slot(PixelStats<C, MAXM, TRANSFORM> &ps, const statmc_stat_type &t, long long n_px, long long p,
                                          int slot, const float *arena, const int32_t *bounds) {
    ps.clear();
    if (p >= n_px) return;
    if (slot == 0) ps.load(t, p);
    const int s1 = bounds[(long long)(slot + 1) * n_px + p];
    for (int s = bounds[(long long)slot * n_px + p]; s < s1; s++) {
        const float *q = arena + ((long long)s * n_px + p) * C;
        float smp[C];
#pragma unroll
        for (int c = 0; c < C; c++) smp[c] = q[c];
        ps.add(smp);
    }
}

template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void store_slot0(const PixelStats<C, MAXM, TRANSFORM> &ps, const statmc_stat_type &t, long long p,
                                            const statmc_prepass_context &ctx, int with_prepass) {
    if constexpr (MAXM >= 3) {
        if (with_prepass) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// G consecutive lanes per pixel: thread i of the grid is slot i % G of pixel i / G
template <int G, int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(kBlock) void fold_lanes_kernel(statmc_stat_type t, long long n_px, const float *arena, const int32_t *bounds,
                                                            statmc_prepass_context ctx, int with_prepass) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long p = i / G;
    const int slot = (int)(i % G);
    PixelStats<C, MAXM, TRANSFORM> ps;
    fold_slot(ps, t, n_px, p, slot, arena, bounds);
    merge_lanes<G>(ps);
    if (p < n_px && slot == 0) store_slot0(ps, t, p, ctx, with_prepass);
}

// NW waves per workgroup share 64 pixels: lane l of wave w is slot w of pixel 64 * blockIdx.x + l
template <int NW, int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(64 * NW) void fold_waves_kernel(statmc_stat_type t, long long n_px, const float *arena, const int32_t *bounds,
                                                             statmc_prepass_context ctx, int with_prepass) {
    __shared__ float scratch[merge_waves_lds_bytes<NW, C, MAXM, TRANSFORM>() / 4];
    const long long p = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    const int slot = (int)(threadIdx.x >> 6);
    PixelStats<C, MAXM, TRANSFORM> ps;
    fold_slot(ps, t, n_px, p, slot, arena, bounds);
    merge_waves<NW>(ps, scratch);
    if (p < n_px && slot == 0) store_slot0(ps, t, p, ctx, with_prepass);
}

// Both: G lanes of each of NW waves per pixel, 64 / G pixels per workgroup; lane l of wave w is slot w * G + l % G
template <int G, int NW, int C, int MAXM, bool TRANSFORM>
__global__ __launch_bounds__(64 * NW) void fold_lanes_waves_kernel(statmc_stat_type t, long long n_px, const float *arena,
                                                                   const int32_t *bounds, statmc_prepass_context ctx, int with_prepass) {
    __shared__ float scratch[merge_waves_lds_bytes<NW, C, MAXM, TRANSFORM>() / 4];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const long long p = (long long)blockIdx.x * (64 / G) + lane / G;
    const int slot = wave * G + lane % G;
    PixelStats<C, MAXM, TRANSFORM> ps;
    fold_slot(ps, t, n_px, p, slot, arena, bounds);
    merge_lanes<G>(ps);
    merge_waves<NW>(ps, scratch);
    if (p < n_px && slot == 0) store_slot0(ps, t, p, ctx, with_prepass);
}

enum class Meet { lanes, waves, lanes_waves };

template <Meet M, int C, int MAXM, bool TRANSFORM>
int launch_meet(const statmc_stat_type &t, long long n_px, const float *arena, const int32_t *bounds, int G, int NW,
                const statmc_prepass_context *ctx, hipStream_t s) {
    const statmc_prepass_context c = ctx ? *ctx : statmc_prepass_context{nullptr, 0, 0};
    const int pre = ctx ? 1 : 0;
#define STATMC_LANES(g)                                                                                                       \
    case g:                                                                                                                   \
        hipLaunchKernelGGL((fold_lanes_kernel<g, C, MAXM, TRANSFORM>), dim3(grid_for(n_px * g)), dim3(kBlock), 0, s, t, n_px, \
                           arena, bounds, c, pre);                                                                            \
        return launched();
#define STATMC_WAVES(nw)                                                                                                          \
    case nw:                                                                                                                      \
        hipLaunchKernelGGL((fold_waves_kernel<nw, C, MAXM, TRANSFORM>), dim3((unsigned)((n_px + 63) / 64)), dim3(64 * nw), 0, s, \
                           t, n_px, arena, bounds, c, pre);                                                                       \
        return launched();
    if constexpr (M == Meet::lanes) {
        switch (G) {
            STATMC_LANES(2) STATMC_LANES(4) STATMC_LANES(8) STATMC_LANES(16) STATMC_LANES(32) STATMC_LANES(64)
        }
    } else if constexpr (M == Meet::waves) {
        switch (NW) {
            STATMC_WAVES(2) STATMC_WAVES(4) STATMC_WAVES(8) STATMC_WAVES(16)
        }
    } else if (G == 4 && NW == 4) {
        hipLaunchKernelGGL((fold_lanes_waves_kernel<4, 4, C, MAXM, TRANSFORM>), dim3((unsigned)((n_px + 15) / 16)), dim3(256), 0, s, t,
                           n_px, arena, bounds, c, pre);
        return launched();
    }
#undef STATMC_LANES
#undef STATMC_WAVES
    return STATMC_ERR_INVALID;
}

template <Meet M, int C>
int meet_dispatch(const statmc_stat_type &t, long long n_px, const float *arena, const int32_t *bounds, int G, int NW,
                  const statmc_prepass_context *ctx, hipStream_t s) {
    if (t.transform) {
        if (t.max_moment == 3) return launch_meet<M, C, 3, true>(t, n_px, arena, bounds, G, NW, ctx, s);
        if (t.max_moment == 2) return launch_meet<M, C, 2, true>(t, n_px, arena, bounds, G, NW, ctx, s);
        return launch_meet<M, C, 1, true>(t, n_px, arena, bounds, G, NW, ctx, s);
    }
    if (t.max_moment == 3) return launch_meet<M, C, 3, false>(t, n_px, arena, bounds, G, NW, ctx, s);
    if (t.max_moment == 2) return launch_meet<M, C, 2, false>(t, n_px, arena, bounds, G, NW, ctx, s);
    return launch_meet<M, C, 1, false>(t, n_px, arena, bounds, G, NW, ctx, s);
}

// ------------------------------------------------------------------ the sample generator
// One 32-bit hash of (seed, pixel, sample) seeds a short PCG-style stream that yields the sample's 11 values.  Written with
// contraction off, so that gen_arena and gen_fold produce the same bits whatever the optimiser does around them.
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
struct Rng {
    uint32_t state;
    __device__ __forceinline__ float next() {   // [0, 1), 24 bits
        state = state * 747796405u + 2891336453u;
        const uint32_t w = ((state >> ((state >> 28) + 4u)) ^ state) * 277803737u;
        return (float)((w ^ (w >> 22)) >> 8) * (1.f / 16777216.f);
    }
};
struct Sample {
    float radiance[3], normal[3], albedo[3], depth, material;
};
__device__ __forceinline__ void gen_sample(uint32_t seed, long long px, int s, Sample &o) {
#pragma clang fp contract(off)
    Rng r{mix32(seed ^ mix32((uint32_t)px * 0x9e3779b9u ^ mix32((uint32_t)s + 0x632be5abu)))};
    const float scale = r.next() < 1.f / 64.f ? 64.f : 1.f;   // the odd firefly
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float u = r.next();
        o.radiance[c] = (0.01f + u * u) * scale;               // positive radiance
    }
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = 2.f * r.next() - 1.f;
    const float len2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const float inv = len2 > 1e-6f ? 1.f / __builtin_sqrtf(len2) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) o.normal[c] = len2 > 1e-6f ? v[c] * inv : (c == 2 ? 1.f : 0.f);   // unit normals
#pragma unroll
    for (int c = 0; c < 3; c++) o.albedo[c] = r.next();                                              // [0, 1)
    o.depth = 1.f + 9.f * r.next();
    o.material = __builtin_floorf(8.f * r.next());
}

__global__ __launch_bounds__(kBlock) void gen_arena_kernel(uint32_t seed, long long n_px, int sample0, int n_samples, float *rad,
                                                           float *nrm, float *alb, float *dep, float *mat) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_px) return;
    for (int s = 0; s < n_samples; s++) {
        Sample o;
        gen_sample(seed, p, sample0 + s, o);
        const long long e = (long long)s * n_px + p;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            rad[3 * e + c] = o.radiance[c];
            nrm[3 * e + c] = o.normal[c];
            alb[3 * e + c] = o.albedo[c];
        }
        dep[e] = o.depth;
        mat[e] = o.material;
    }
}

struct FiveTypes {
    statmc_stat_type t[5];
};

__global__ __launch_bounds__(kBlock) void gen_fold_kernel(uint32_t seed, long long n_px, int sample0, int n_samples, FiveTypes ft,
                                                          statmc_prepass_context ctx, int with_prepass) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_px) return;
    PixelStats<3, 3, true> rad;
    PixelStats<3, 1, false> nrm, alb;
    PixelStats<1, 1, false> dep, mat;
    rad.load(ft.t[0], p);
    nrm.load(ft.t[1], p);
    alb.load(ft.t[2], p);
    dep.load(ft.t[3], p);
    mat.load(ft.t[4], p);
    for (int s = 0; s < n_samples; s++) {
        Sample o;
        gen_sample(seed, p, sample0 + s, o);
        rad.add(o.radiance);
        nrm.add(o.normal);
        alb.add(o.albedo);
        dep.add(&o.depth);
        mat.add(&o.material);
    }
    if (with_prepass) rad.store(ft.t[0], p, ctx);
    else rad.store(ft.t[0], p);
    nrm.store(ft.t[1], p);
    alb.store(ft.t[2], p);
    dep.store(ft.t[3], p);
    mat.store(ft.t[4], p);
}

// gen_fold_kernel with G consecutive lanes per pixel: slot j folds the samples j, j + G, ... of the launch (slot 0 into the
// pixel's stored state), the five states are merged across the lanes and slot 0 stores.
template <int G>
__global__ __launch_bounds__(kBlock) void gen_fold_lanes_kernel(uint32_t seed, long long n_px, int sample0, int n_samples, FiveTypes ft,
                                                                statmc_prepass_context ctx, int with_prepass) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long p = i / G;
    const int slot = (int)(i % G);
    const bool mine = p < n_px && slot == 0;
    PixelStats<3, 3, true> rad;
    PixelStats<3, 1, false> nrm, alb;
    PixelStats<1, 1, false> dep, mat;
    rad.clear();
    nrm.clear();
    alb.clear();
    dep.clear();
    mat.clear();
    if (mine) {
        rad.load(ft.t[0], p);
        nrm.load(ft.t[1], p);
        alb.load(ft.t[2], p);
        dep.load(ft.t[3], p);
        mat.load(ft.t[4], p);
    }
    if (p < n_px) {
        for (int s = slot; s < n_samples; s += G) {
            Sample o;
            gen_sample(seed, p, sample0 + s, o);
            rad.add(o.radiance);
            nrm.add(o.normal);
            alb.add(o.albedo);
            dep.add(&o.depth);
            mat.add(&o.material);
        }
    }
    merge_lanes<G>(rad);   // every lane of the wave, pixels past the film included
    merge_lanes<G>(nrm);
    merge_lanes<G>(alb);
    merge_lanes<G>(dep);
    merge_lanes<G>(mat);
    if (!mine) return;
    if (with_prepass) rad.store(ft.t[0], p, ctx);
    else rad.store(ft.t[0], p);
    nrm.store(ft.t[1], p);
    alb.store(ft.t[2], p);
    dep.store(ft.t[3], p);
    mat.store(ft.t[4], p);
}

int launch_gen_fold_lanes(uint32_t seed, long long n_px, int sample0, int n_samples, int G, const FiveTypes &ft,
                          const statmc_prepass_context &c, int pre, hipStream_t s) {
    switch (G) {
#define STATMC_GEN_LANES(g)                                                                                                        \
    case g:                                                                                                                        \
        hipLaunchKernelGGL((gen_fold_lanes_kernel<g>), dim3(grid_for(n_px * g)), dim3(kBlock), 0, s, seed, n_px, sample0, n_samples, \
                           ft, c, pre);                                                                                            \
        return launched();
        STATMC_GEN_LANES(2) STATMC_GEN_LANES(4) STATMC_GEN_LANES(8) STATMC_GEN_LANES(16) STATMC_GEN_LANES(32) STATMC_GEN_LANES(64)
#undef STATMC_GEN_LANES
    }
    return STATMC_ERR_INVALID;
}

// gen_fold's checks of the five types (and of ctx): 0, or STATMC_ERR_INVALID
int five_types_of(const statmc_stat_type *types, const statmc_prepass_context *ctx, FiveTypes &ft) {
    static const int want[5][3] = {{3, 1, 3}, {3, 0, 1}, {3, 0, 1}, {1, 0, 1}, {1, 0, 1}};   // channels, transform, max_moment
    for (int k = 0; k < 5; k++) {
        const statmc_stat_type &t = types[k];
        if (t.channels != want[k][0] || (t.transform != 0) != (want[k][1] != 0) || t.max_moment != want[k][2] || !t.n || !t.mean)
            return STATMC_ERR_INVALID;
        if (k == 0 && (!t.m2 || !t.m3 || !t.film_mean || !t.film_m2)) return STATMC_ERR_INVALID;
        ft.t[k] = t;
    }
    if (ctx && (!types[0].mean_corr || !types[0].discriminator || !ctx->t_table)) return STATMC_ERR_INVALID;
    return STATMC_OK;
}

// fold_arena_slots' checks of one type (and of ctx)
bool fold_args_ok(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds,
                  const statmc_prepass_context *ctx) {
    if (!t || width <= 0 || height <= 0 || !arena || !bounds) return false;
    if ((t->channels != 1 && t->channels != 3) || t->max_moment < 1 || t->max_moment > 3 || !t->n || !t->mean) return false;
    if ((t->max_moment >= 2 && !t->m2) || (t->max_moment >= 3 && !t->m3) || (t->transform && (!t->film_mean || !t->film_m2))) return false;
    return !ctx || (t->max_moment >= 3 && t->mean_corr && t->discriminator && ctx->t_table);
}

template <Meet M>
int fold_meet(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds, int G, int NW,
              const statmc_prepass_context *ctx, void *stream) {
    if (!fold_args_ok(t, width, height, arena, bounds, ctx)) return STATMC_ERR_INVALID;
    const long long n_px = (long long)width * height;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return t->channels == 3 ? meet_dispatch<M, 3>(*t, n_px, arena, bounds, G, NW, ctx, s)
                            : meet_dispatch<M, 1>(*t, n_px, arena, bounds, G, NW, ctx, s);
}

}  // namespace

extern "C" {

// t: one stat type's device images (its samples / n_samples fields are not read); arena: [n_samples][height][width][channels];
// ctx != NULL: the pre-pass store (max_moment 3 and t.mean_corr / t.discriminator only).
int fold_arena(const statmc_stat_type *t, int width, int height, const float *arena, int n_samples, const statmc_prepass_context *ctx,
               void *stream) {
    if (!t || width <= 0 || height <= 0 || n_samples < 0 || (n_samples > 0 && !arena)) return STATMC_ERR_INVALID;
    if ((t->channels != 1 && t->channels != 3) || t->max_moment < 1 || t->max_moment > 3 || !t->n || !t->mean) return STATMC_ERR_INVALID;
    if ((t->max_moment >= 2 && !t->m2) || (t->max_moment >= 3 && !t->m3) || (t->transform && (!t->film_mean || !t->film_m2)))
        return STATMC_ERR_INVALID;
    if (ctx && (t->max_moment < 3 || !t->mean_corr || !t->discriminator || !ctx->t_table)) return STATMC_ERR_INVALID;
    const long long n_px = (long long)width * height;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return t->channels == 3 ? fold_dispatch<3>(*t, n_px, arena, n_samples, ctx, s) : fold_dispatch<1>(*t, n_px, arena, n_samples, ctx, s);
}

// The same with every pixel's samples dealt to n_slots slots that are merged in slot order (fold_slots_kernel): bounds is a
// device array [n_slots + 1][height][width] of sample indices into the arena, non-decreasing per pixel and within the arena
// (the caller's to guarantee: it is not read here).
int fold_arena_slots(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds, int n_slots,
                     const statmc_prepass_context *ctx, void *stream) {
    if (!fold_args_ok(t, width, height, arena, bounds, ctx) || n_slots < 1) return STATMC_ERR_INVALID;
    const long long n_px = (long long)width * height;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return t->channels == 3 ? fold_dispatch<3>(*t, n_px, arena, 0, ctx, s, bounds, n_slots)
                            : fold_dispatch<1>(*t, n_px, arena, 0, ctx, s, bounds, n_slots);
}

// arenas[5]: radiance, normal, albedo ([n_samples][height][width][3]), depth, material id ([n_samples][height][width]); samples
// sample0 .. sample0 + n_samples - 1 of every pixel.
int gen_arena(uint32_t seed, int width, int height, int sample0, int n_samples, float *const *arenas, void *stream) {
    if (!arenas || width <= 0 || height <= 0 || n_samples < 0 || sample0 < 0) return STATMC_ERR_INVALID;
    for (int k = 0; k < 5; k++)
        if (!arenas[k]) return STATMC_ERR_INVALID;
    const long long n_px = (long long)width * height;
    hipLaunchKernelGGL(gen_arena_kernel, dim3(grid_for(n_px)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), seed, n_px, sample0,
                       n_samples, arenas[0], arenas[1], arenas[2], arenas[3], arenas[4]);
    return launched();
}

// types[5] in gen_arena's order, with the configurations of film.STAT_TYPES: radiance (3 channels, transform, max_moment 3),
// normal / albedo (3, no transform, 1), depth / material id (1, no transform, 1); ctx != NULL: radiance is stored with its
// pre-pass (types[0].mean_corr / discriminator).
int gen_fold(uint32_t seed, int width, int height, int sample0, int n_samples, const statmc_stat_type *types,
             const statmc_prepass_context *ctx, void *stream) {
    if (!types || width <= 0 || height <= 0 || n_samples < 0 || sample0 < 0) return STATMC_ERR_INVALID;
    FiveTypes ft;
    if (five_types_of(types, ctx, ft) != STATMC_OK) return STATMC_ERR_INVALID;
    const statmc_prepass_context c = ctx ? *ctx : statmc_prepass_context{nullptr, 0, 0};
    const long long n_px = (long long)width * height;
    hipLaunchKernelGGL(gen_fold_kernel, dim3(grid_for(n_px)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), seed, n_px, sample0,
                       n_samples, ft, c, ctx ? 1 : 0);
    return launched();
}

// fold_arena_slots with the slots held by different threads, merged by the header's reductions: a balanced tree over the
// slots (statmc_device_api.hpp), not fold_arena_slots' left fold.  bounds: [slots + 1][height][width], as above.
// G lanes per pixel (2, 4, 8, 16, 32 or 64 slots), merge_lanes<G>:
int fold_arena_lanes(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds, int G,
                     const statmc_prepass_context *ctx, void *stream) {
    return fold_meet<Meet::lanes>(t, width, height, arena, bounds, G, 0, ctx, stream);
}

// one lane per pixel and wave, NW waves per workgroup share 64 pixels (2, 4, 8 or 16 slots), merge_waves<NW>:
int fold_arena_waves(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds, int NW,
                     const statmc_prepass_context *ctx, void *stream) {
    return fold_meet<Meet::waves>(t, width, height, arena, bounds, 0, NW, ctx, stream);
}

// both: G lanes in each of NW waves per pixel, G * NW slots with slot index w * G + j; merge_lanes<G>, then merge_waves<NW>.
// The example instantiates G = 4, NW = 4 (16 slots) only; every other pair is STATMC_ERR_INVALID.
int fold_arena_lanes_waves(const statmc_stat_type *t, int width, int height, const float *arena, const int32_t *bounds, int G, int NW,
                           const statmc_prepass_context *ctx, void *stream) {
    return fold_meet<Meet::lanes_waves>(t, width, height, arena, bounds, G, NW, ctx, stream);
}

// gen_fold with the samples of a pixel dealt to G lanes (slot j takes samples j, j + G, ... of the launch), all five types
// merged across the lanes (merge_lanes<G>): within the project's bound of gen_fold, not its bits (another merge order).
int gen_fold_lanes(uint32_t seed, int width, int height, int sample0, int n_samples, int G, const statmc_stat_type *types,
                   const statmc_prepass_context *ctx, void *stream) {
    if (!types || width <= 0 || height <= 0 || n_samples < 0 || sample0 < 0) return STATMC_ERR_INVALID;
    FiveTypes ft;
    if (five_types_of(types, ctx, ft) != STATMC_OK) return STATMC_ERR_INVALID;
    const statmc_prepass_context c = ctx ? *ctx : statmc_prepass_context{nullptr, 0, 0};
    return launch_gen_fold_lanes(seed, (long long)width * height, sample0, n_samples, G, ft, c, ctx ? 1 : 0,
                                 reinterpret_cast<hipStream_t>(stream));
}

// fold_arena without a film: every pixel's samples folded from the state of no samples and written as state record p of
// `records` (device, [width * height][statmc_state_dwords(channels, max_moment, transform)] dwords, 4-byte aligned).
int fold_arena_records(int channels, int transform, int max_moment, int width, int height, const float *arena, int n_samples, int32_t *records,
                       void *stream) {
    if (width <= 0 || height <= 0 || n_samples < 0 || (n_samples > 0 && !arena) || !records) return STATMC_ERR_INVALID;
    if ((channels != 1 && channels != 3) || max_moment < 1 || max_moment > 3) return STATMC_ERR_INVALID;
    const long long n_px = (long long)width * height;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return channels == 3 ? records_dispatch<3>(transform, max_moment, n_px, arena, n_samples, records, s)
                         : records_dispatch<1>(transform, max_moment, n_px, arena, n_samples, records, s);
}

}  // extern "C"
