// statmc_accumulate_fold.h -- what a lane of an accumulation kernel that owns 4 consecutive pixels of one stat type holds and
// does per sample: the packed twin of statmc::device::add_sample and the moves of a state plane between memory and the lane's
// element pairs.  One definition for every translation unit with such a lane (statmc_pointwise.hip: accumulate_lane and the
// type-fused walk; statmc_counted.hip: the per-pixel counts), so that their bits agree by construction.  Everything here is
// __forceinline__ device code: a kernel's code object does not depend on which file the text stands in.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/statmc_device_api.hpp"

namespace statmc {

typedef float vfloat4 __attribute__((ext_vector_type(4)));

// The same update on two elements at once (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: one issue slot for two lanes'
// worth of IEEE fp32 arithmetic, each component rounded exactly like the scalar instruction, so the bits are those of
// add_sample).  The kernel holds ~250 VGPRs, i.e. two waves per SIMD, and while one of them waits for memory the other
// issues one vector instruction per 4 cycles: the radiance type (Box-Cox + three moments + the raw-sample chain, 27
// instructions per element and sample) was bound by exactly that issue rate (5.1 TB/s on its own); paired, it is
// bound by the memory like the feature types.
typedef float v2f __attribute__((ext_vector_type(2)));
struct PairState {
    v2f mean, m2, m3, fmean, fm2;
};
__device__ __forceinline__ v2f div_by_count2(v2f d, v2f nf, v2f r) {
    const v2f q0 = d * r;
    const v2f rem = __builtin_elementwise_fma(-q0, nf, d);
    return __builtin_elementwise_fma(rem, r, q0);
}
// G pairs at a time, stage by stage: consecutive instructions belong to different pairs, so none waits for the one
// before it (a dependent packed instruction costs a wait state, and the kernel is compiled without the machine scheduler:
// the source order is the issue order).
#define STATMC_PAIRS(i) _Pragma("unroll") for (int i = 0; i < G; i++)
template <int G, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void add_sample2(PairState *st, const v2f *nf, const v2f *r, const v2f *smp) {
    v2f v[G], d[G], q0[G], dN[G];
    if (TRANSFORM) {   // estimator.h:215 -- boxCox(sample, .5f), as in add_sample
        STATMC_PAIRS(i) v[i] = v2f{__builtin_amdgcn_sqrtf(smp[i].x), __builtin_amdgcn_sqrtf(smp[i].y)};
        // (root - 1) / .5 in one instruction: fma(root, 2, -2) rounds 2 root - 2 = 2 (root - 1) once, and doubling commutes with
        // rounding (no overflow: root < 2^64; no underflow: |root - 1| is 0 or at least 2^-24) -- the bits of the two-step form
        STATMC_PAIRS(i) v[i] = __builtin_elementwise_fma(v[i], v2f{2.f, 2.f}, v2f{-2.f, -2.f});
    } else {
        STATMC_PAIRS(i) v[i] = smp[i];
    }
    STATMC_PAIRS(i) d[i] = v[i] - st[i].mean;
    STATMC_PAIRS(i) q0[i] = d[i] * r[i];                                         // div_by_count, three stages
    STATMC_PAIRS(i) dN[i] = __builtin_elementwise_fma(-q0[i], nf[i], d[i]);
    STATMC_PAIRS(i) dN[i] = __builtin_elementwise_fma(dN[i], r[i], q0[i]);
    STATMC_PAIRS(i) st[i].mean += dN[i];
    if (MAXM >= 2) {
        v2f t[G];
        STATMC_PAIRS(i) t[i] = d[i] - dN[i];
        STATMC_PAIRS(i) t[i] = d[i] * t[i];
        STATMC_PAIRS(i) st[i].m2 += t[i];
    }
    if (MAXM >= 3) {   // m3 += -3 dN m2 + d (d^2 - dN^2), with the m2 already updated (estimator.h:178-180)
        v2f a[G], b[G];
        STATMC_PAIRS(i) a[i] = -3.f * dN[i];
        STATMC_PAIRS(i) b[i] = d[i] * d[i];
        STATMC_PAIRS(i) dN[i] = dN[i] * dN[i];
        STATMC_PAIRS(i) a[i] = a[i] * st[i].m2;
        STATMC_PAIRS(i) b[i] = b[i] - dN[i];
        STATMC_PAIRS(i) b[i] = d[i] * b[i];
        STATMC_PAIRS(i) a[i] = a[i] + b[i];
        STATMC_PAIRS(i) st[i].m3 += a[i];
    }
    if (TRANSFORM) {   // the raw-sample chain (estimator.h:217-225)
        STATMC_PAIRS(i) d[i] = smp[i] - st[i].fmean;
        STATMC_PAIRS(i) q0[i] = d[i] * r[i];
        STATMC_PAIRS(i) dN[i] = __builtin_elementwise_fma(-q0[i], nf[i], d[i]);
        STATMC_PAIRS(i) dN[i] = __builtin_elementwise_fma(dN[i], r[i], q0[i]);
        STATMC_PAIRS(i) st[i].fmean += dN[i];
        STATMC_PAIRS(i) dN[i] = d[i] - dN[i];
        STATMC_PAIRS(i) dN[i] = d[i] * dN[i];
        STATMC_PAIRS(i) st[i].fm2 += dN[i];
    }
}
#undef STATMC_PAIRS

// One state plane of a lane's 4 consecutive pixels -- C float4 from p on -- into the field of the lane's element pairs (2 i, 2 i + 1)
// and back.  ON = false: a plane the stat type does not hold; it reads as zeros and is not stored.
template <int C, bool ON = true>
__device__ __forceinline__ void load_plane(PairState *st, v2f PairState::*field, const float *p) {
#pragma unroll
    for (int k = 0; k < C; k++) {
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ON) v = *reinterpret_cast<const float4 *>(p + 4 * k);
        st[2 * k].*field = v2f{v.x, v.y};
        st[2 * k + 1].*field = v2f{v.z, v.w};
    }
}
template <int C, bool ON = true>
__device__ __forceinline__ void store_plane(float *p, const PairState *st, v2f PairState::*field) {
    if constexpr (ON) {
#pragma unroll
        for (int k = 0; k < C; k++) {
            const vfloat4 v = {(st[2 * k].*field).x, (st[2 * k].*field).y, (st[2 * k + 1].*field).x, (st[2 * k + 1].*field).y};
            *reinterpret_cast<vfloat4 *>(p + 4 * k) = v;
        }
    }
}
// The counts of the lane's 4 pixels after the batch: one per pixel, or (NC = 1) the one count a group is known to hold.
// Merge*Tile casts the tile's uint64 count to int32 (estimator.cpp:347,380)
template <int NC>
__device__ __forceinline__ void store_counts(int32_t *n, const int (&n_out)[NC]) {
    typedef int vint4 __attribute__((ext_vector_type(4)));
    const vint4 v = {n_out[0], n_out[NC > 1 ? 1 : 0], n_out[NC > 1 ? 2 : 0], n_out[NC > 1 ? 3 : 0]};
    *reinterpret_cast<vint4 *>(n) = v;
}

}  // namespace statmc
