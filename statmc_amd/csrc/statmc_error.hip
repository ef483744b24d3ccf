// statmc_error.hip -- statmc_error_scores and statmc_plan_to_target (include/statmc.h): the error of the mean as a score image --
// the standard error, or the half-width of the confidence interval at one of the device's Student-t tables -- and the per-pixel
// sample counts that bring such an error to a tolerance.  DESIGN.md 4.2g.
//
// Both are one launch that streams the film once: 4 + 8 C + 4 B/px in and out for the scores (statmc_sample_scores' traffic), 8 B/px
// in and 4 B/px out for the plan.  The quantile is a gather from a 16 KiB table that neighbouring pixels mostly hit at the same
// entry; it is read through the cache -- staging it in LDS per workgroup was built and measured, and lost.
#include "statmc_device.h"
#include "statmc_error_args.h"

namespace statmc {

namespace {

// ---------------------------------------------------------------- statmc_error_scores
// Every operation rounds once (no contraction); `/` and sqrtf are the correctly rounded IEEE quotient and root.  The first three
// lines are statmc_sample_scores' v.
template <int C>
__device__ __forceinline__ float error_pixel(int n, const float (&mean)[C], const float (&m2)[C], const float *tq, int metric, float eps) {
#pragma clang fp contract(off)
    if (n < 2) return __builtin_inff();
    const float fn1 = (float)(n - 1);
    float v = m2[0] / fn1;
#pragma unroll
    for (int c = 1; c < C; c++) v = v + m2[c] / fn1;
    const float vm = v / (float)n;
    float e = sqrtf(vm);
    if (tq) e = tq[min(n - 1, kErrorDofMax) - 1] * e;   // n >= 2: the index lies in [0, 4095]
    if (metric == STATMC_SCORE_ABSOLUTE) return e;
    float m = fabsf(mean[0]);
#pragma unroll
    for (int c = 1; c < C; c++) m = m + fabsf(mean[c]);
    return e / (eps + m);
}

template <int C>
__device__ __forceinline__ void error_load_quad_plane(const float *plane, long long p0, float (&t)[4 * C]) {
#pragma unroll
    for (int i = 0; i < C; i++) {
        const float4 x = reinterpret_cast<const float4 *>(plane + p0 * C)[i];
        t[4 * i] = x.x, t[4 * i + 1] = x.y, t[4 * i + 2] = x.z, t[4 * i + 3] = x.w;
    }
}

// One lane per aligned quad of pixels: a full quad of 16-byte aligned planes moves as dwordx4 (1 + 2 C loads, one store); the
// film's last, partial quad and every quad of unaligned planes go element by element through the same error_pixel.
template <int C>
__global__ __launch_bounds__(kPlanBlock) void error_scores_kernel(ErrorArgs a) {
    const long long p0 = ((long long)blockIdx.x * kPlanBlock + threadIdx.x) * 4;
    if (p0 >= a.n_px) return;
    if (a.vec && p0 + 4 <= a.n_px) {
        const int4 n = *reinterpret_cast<const int4 *>(a.n + p0);
        float mean[4 * C], m2[4 * C];
        error_load_quad_plane<C>(a.film_mean, p0, mean);
        error_load_quad_plane<C>(a.film_m2, p0, m2);
        const int nn[4] = {n.x, n.y, n.z, n.w};
        float out[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float pm[C], p2[C];
#pragma unroll
            for (int c = 0; c < C; c++) pm[c] = mean[q * C + c], p2[c] = m2[q * C + c];
            out[q] = error_pixel<C>(nn[q], pm, p2, a.tq, a.metric, a.eps);
        }
        *reinterpret_cast<float4 *>(a.score + p0) = make_float4(out[0], out[1], out[2], out[3]);
        return;
    }
    for (long long p = p0; p < p0 + 4 && p < a.n_px; p++) {
        float pm[C], p2[C];
#pragma unroll
        for (int c = 0; c < C; c++) pm[c] = a.film_mean[p * C + c], p2[c] = a.film_m2[p * C + c];
        a.score[p] = error_pixel<C>(a.n[p], pm, p2, a.tq, a.metric, a.eps);
    }
}

// ---------------------------------------------------------------- statmc_plan_to_target
__device__ __forceinline__ long long target_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A lane's partial sums.  total and need are 64-bit: a lane of the largest film walks 2^14 pixels of up to 2^20 and 2^30 each.
struct TargetSums {
    long long total, need;
    int open, capped, unjudged, live, saturated;   // pixels: a lane has fewer than 2^31
};

// One pixel of the definition.  On an open pixel e > target, both in [2^-60, 2^60]: r >= 1, r2 and t are normal numbers or +inf
// (inf * nn with nn >= 2 is +inf), so the denormal mode reaches no bit; (int)ceilf(t) is exact below 2^30.
__device__ __forceinline__ int target_pixel(float e, int n, float target, int c_min, int c_max, TargetSums &s) {
#pragma clang fp contract(off)
    const bool live = e >= kTargetLo && e <= kTargetHi;   // NaN: neither
    const bool saturated = e > kTargetHi;
    const int nn = min(max(n, 0), kPlanMaxTarget);
    const bool unjudged = saturated || (live && nn < 2);
    const bool open = live && nn >= 2 && e > target;
    s.live += live, s.saturated += saturated, s.unjudged += unjudged, s.open += open;
    int c = unjudged ? c_max : c_min;
    if (open) {
        const float r = e / target;
        const float r2 = r * r;
        const float t = r2 * (float)nn;
        const int big_n = t >= (float)kPlanMaxTarget ? kPlanMaxTarget : (int)ceilf(t);
        const int d = max(big_n - nn, 0);
        s.need += d;
        s.capped += d > c_max;
        c = min(max(d, c_min), c_max);
    }
    s.total += c;
    return c;
}

// One pass: a lane walks its quads (dwordx4 where error, n and counts are 16-byte aligned), keeps its sums in registers, a wave adds
// its lanes through cross-lane shuffles, the workgroup's waves meet in LDS, and one 64-bit atomicAdd per word of the result and
// workgroup lands there (n_live and n_saturated share the last word: neither sum reaches 2^32, so no carry crosses).  Integer sums:
// the order of the atomics reaches no bit.
constexpr int kTargetWords = 6;
static_assert(sizeof(statmc_target_result) == kTargetWords * sizeof(long long), "one atomic per 64-bit word of the result");

__global__ __launch_bounds__(kPlanBlock) void plan_to_target_kernel(TargetArgs a) {
    __shared__ long long part[kPlanBlock / 64][kTargetWords];
    TargetSums s{0, 0, 0, 0, 0, 0, 0};
    for (long long chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const long long p0 = chunk * kPlanChunk + (long long)threadIdx.x * kPlanQuad;
        if (p0 >= a.n_px) continue;
        if (a.vec && p0 + kPlanQuad <= a.n_px) {
            const float4 ev = *reinterpret_cast<const float4 *>(a.error + p0);
            const int4 nv = *reinterpret_cast<const int4 *>(a.n + p0);
            int4 c;
            c.x = target_pixel(ev.x, nv.x, a.target, a.c_min, a.c_max, s);
            c.y = target_pixel(ev.y, nv.y, a.target, a.c_min, a.c_max, s);
            c.z = target_pixel(ev.z, nv.z, a.target, a.c_min, a.c_max, s);
            c.w = target_pixel(ev.w, nv.w, a.target, a.c_min, a.c_max, s);
            *reinterpret_cast<int4 *>(a.counts + p0) = c;
        } else {
            for (long long p = p0; p < p0 + kPlanQuad && p < a.n_px; p++)
                a.counts[p] = target_pixel(a.error[p], a.n[p], a.target, a.c_min, a.c_max, s);
        }
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const long long w[kTargetWords] = {target_wave_sum(s.total),
                                       target_wave_sum(s.need),
                                       target_wave_sum((long long)s.open),
                                       target_wave_sum((long long)s.capped),
                                       target_wave_sum((long long)s.unjudged),
                                       target_wave_sum((long long)s.live | ((long long)s.saturated << 32))};
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kTargetWords; j++) part[wave][j] = w[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < kTargetWords) {
        long long v = 0;
#pragma unroll
        for (int k = 0; k < kPlanBlock / 64; k++) v += part[k][threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(a.result) + threadIdx.x, (unsigned long long)v);
    }
}

}  // namespace

hipError_t launch_error_scores(const ErrorArgs &a, hipStream_t s) {
    const long long quads = (a.n_px + 3) / 4;
    const unsigned grid = (unsigned)((quads + kPlanBlock - 1) / kPlanBlock);
    if (a.channels == 3) hipLaunchKernelGGL(error_scores_kernel<3>, dim3(grid), dim3(kPlanBlock), 0, s, a);
    else hipLaunchKernelGGL(error_scores_kernel<1>, dim3(grid), dim3(kPlanBlock), 0, s, a);
    return hipGetLastError();
}

// The result is zeroed on the stream, then the one launch adds into it.
hipError_t launch_plan_to_target(const TargetArgs &a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.result, 0, sizeof(statmc_target_result), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(plan_to_target_kernel, dim3((unsigned)a.grid), dim3(kPlanBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc
