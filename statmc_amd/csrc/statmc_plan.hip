// statmc_plan.hip -- statmc_sample_scores and statmc_plan_samples (include/statmc.h): a per-pixel noise score from the running
// statistics, and the per-pixel sample counts that spend a budget by it -- n_p + c_p proportional to the score, clamped per pixel,
// the one level found by water-filling on the device.  DESIGN.md 4.2c.
//
// The plan is eight launches on one stream, none of which waits for another workgroup:
//   - kPlanPasses = 5 search passes (plan_pass_kernel).  A pass evaluates T(u) = sum_p c_p(u) at 64 candidate levels at once: a lane
//     keeps 64 partial sums in registers over its pixels, a wave adds them through cross-lane shuffles (a reduce-scatter: 63
//     exchanges for all 64 sums), the workgroup's four waves through LDS, and one 64-bit vector atomicAdd per candidate and
//     workgroup lands in the workspace.  Every workgroup of the NEXT pass reads those 64 totals and derives its own candidates
//     from them (plan_search): the search never leaves the device.
//     The sums are integers, so the order of the atomics reaches no bit.
//   - the raster-order trim of the last float step, an exclusive prefix sum of d_p = c_p(u*) - c_p(u* - 1) in three ordinary
//     launches: per-block sums (plan_block_sums_kernel), one workgroup over the block sums which also writes the result
//     (plan_scan_blocks_kernel), and the apply that writes sample_counts (plan_apply_kernel).
// score and n are 8 B/px and are read once per launch: 16.6 MB at 1080p, resident in the last-level cache between them.
#include "statmc_device.h"
#include "statmc_plan_args.h"
#include "statmc_scan.h"

namespace statmc {

namespace {

// ---------------------------------------------------------------- the definition's per-pixel pieces
constexpr float kPlanLiveLo = 0x1p-60f, kPlanLiveHi = 0x1p60f;

// c_p(u) of a live pixel: t = fl32(level * s), N = min(ceil(t), 2^30), clamp(N - n, c_min, c_max).  level * s is a normal number for
// every level in [2^-63, 2^63] and every live s, so the denormal mode reaches no bit; (int)ceilf(t) is exact below 2^30.
// (min(ceil(t), 2^30) is ceil(min(t, 2^30)): 2^30 is an integer.)  Seven VALU operations: mul, min, ceil, cvt, sub, med3, and the add.
__device__ __forceinline__ int plan_count(uint32_t u, float s, int nn, int lo, int hi) {
    const float t = fminf(__uint_as_float(u) * s, (float)kPlanMaxTarget);
    return min(max((int)ceilf(t) - nn, lo), hi);
}

// One pixel as the kernels carry it.  A pixel whose count no level moves -- saturated (c_max), dead (c_min), past the film's end (0)
// -- is a live pixel of score 1 whose two bounds are that count: the candidates' loop has no class left to tell apart.
struct PlanPixel {
    float s;      // the score where live, else 1 (any level times 1 stays in plan_count's domain)
    int nn;       // clamp(n, 0, 2^30)
    int lo, hi;   // c_min, c_max where live, else the fixed count twice
    bool live, saturated;
};
__device__ __forceinline__ PlanPixel plan_pixel(float s, int n, bool inside, int c_min, int c_max) {
    PlanPixel p;
    p.live = inside && s >= kPlanLiveLo && s <= kPlanLiveHi;   // NaN: neither
    p.saturated = inside && s > kPlanLiveHi;
    const int fixed = !inside ? 0 : p.saturated ? c_max : c_min;
    p.lo = p.live ? c_min : fixed;
    p.hi = p.live ? c_max : fixed;
    p.s = p.live ? s : 1.f;
    p.nn = min(max(n, 0), kPlanMaxTarget);
    return p;
}
__device__ __forceinline__ int plan_count(const PlanPixel &p, uint32_t u) { return plan_count(u, p.s, p.nn, p.lo, p.hi); }

// The lane's quad: pixels p0 .. p0 + 3, those past the film's end counted as nothing.  p0 is a multiple of 4, so with 16-byte
// aligned images a full quad moves as one dwordx4 per image.
__device__ __forceinline__ void plan_load_quad(const PlanArgs &a, long long p0, PlanPixel (&px)[kPlanQuad]) {
    float s[kPlanQuad];
    int n[kPlanQuad] = {0, 0, 0, 0};
    const bool full = p0 + kPlanQuad <= a.n_px;
    if (a.vec && full) {
        const float4 sv = *reinterpret_cast<const float4 *>(a.score + p0);
        s[0] = sv.x, s[1] = sv.y, s[2] = sv.z, s[3] = sv.w;
        if (a.n) {
            const int4 nv = *reinterpret_cast<const int4 *>(a.n + p0);
            n[0] = nv.x, n[1] = nv.y, n[2] = nv.z, n[3] = nv.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kPlanQuad; q++) {
            const bool inside = p0 + q < a.n_px;
            s[q] = inside ? a.score[p0 + q] : 0.f;
            n[q] = inside && a.n ? a.n[p0 + q] : 0;
        }
    }
#pragma unroll
    for (int q = 0; q < kPlanQuad; q++) px[q] = plan_pixel(s[q], n[q], p0 + q < a.n_px, a.c_min, a.c_max);
}

// ---------------------------------------------------------------- the search state, from the workspace
// What the first `passes` passes' totals say.  status -1: budget lies in (T(lo), T(hi)] and t_lo = T(lo); 1 / 2: below the floor /
// above the ceiling, hi the level to plan at and t_lo its total.  Every lane of a full wave calls this (ballot); the result is
// wave-uniform.  passes = 0: the whole range, nothing read.
struct PlanSearch {
    uint32_t lo, hi;
    long long t_lo;
    int status;
};
__device__ __forceinline__ PlanSearch plan_search(const long long *ws, long long budget, int passes) {
    PlanSearch s{kPlanLevelLo, kPlanLevelHi, 0, -1};
    if (passes == 0) return s;
    const int lane = (int)(threadIdx.x & 63);
    const long long *tot = ws + kPlanWsTotals;
    unsigned long long m = __ballot(tot[lane] >= budget);
    if (m & 1ull) return PlanSearch{kPlanLevelLo, kPlanLevelLo, tot[0], 1};
    if (m == 0) return PlanSearch{kPlanLevelHi, kPlanLevelHi, tot[kPlanCandidates - 1], 2};
    int j = __ffsll((long long)m) - 1;
    s.hi = kPlanLevelLo + ((uint32_t)j << 24);
    s.lo = s.hi - (1u << 24);
    s.t_lo = tot[j - 1];
    for (int q = 1; q < passes; q++) {
        const uint32_t step = 1u << (24 - 6 * q);
        tot += kPlanCandidates;
        m = __ballot(tot[lane] >= budget);
        j = m ? __ffsll((long long)m) - 1 : kPlanCandidates - 1;   // (candidate 63 is hi, T(hi) >= budget: m is never 0)
        if (j > 0) s.t_lo = tot[j - 1];
        s.hi = s.lo + (uint32_t)(j + 1) * step;
        s.lo = s.hi - step;
    }
    return s;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// (wave_inclusive_scan and block_exclusive_scan, the trim's block step: statmc_scan.h)

// ---------------------------------------------------------------- a search pass
// The wave's sums of all 64 candidates in 63 exchanges, not 64 x 6: a reduce-scatter.  At the step of half h the lanes whose bit h
// is clear keep candidates [0, h) and hand [h, 2 h) to their partner lane ^ h, the others the other way round; after the steps
// h = 32 .. 1 lane L holds, in v[0], the wave's total of candidate L.  Static register indices throughout.
template <typename Red>
__device__ __forceinline__ Red wave_reduce_scatter(Red (&v)[kPlanCandidates]) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int h = kPlanCandidates / 2; h >= 1; h >>= 1) {
        const bool upper = (lane & h) != 0;
#pragma unroll
        for (int k = 0; k < h; k++) {
            const Red below = v[k], above = v[k + h];   // (both read first: a choice of values, never of registers)
            v[k] = (upper ? above : below) + __shfl_xor(upper ? below : above, h, 64);
        }
    }
    return v[0];
}

// Acc: a lane's partial sums, int32_t while they cannot leave 31 bits (PlanArgs::wide == 0), else int64_t.  Red: the wave's sums,
// int32_t while 64 lanes' cannot either (PlanArgs::wide_wave == 0).
template <typename Acc, typename Red>
__global__ __launch_bounds__(kPlanBlock) void plan_pass_kernel(PlanArgs a, int pass) {
    __shared__ long long part[kPlanBlock / 64][kPlanCandidates + 2];
    const PlanSearch s = plan_search(a.ws, a.budget, pass);
    if (s.status > 0) return;   // the same verdict in every workgroup: pass 0 settled it, there is nothing to search
    const uint32_t step = 1u << (24 - 6 * pass);
    const uint32_t first = pass == 0 ? kPlanLevelLo : s.lo + step;
    Acc acc[kPlanCandidates];
#pragma unroll
    for (int j = 0; j < kPlanCandidates; j++) acc[j] = 0;
    int n_live = 0, n_saturated = 0;
    for (long long chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        PlanPixel px[kPlanQuad];
        plan_load_quad(a, chunk * kPlanChunk + (long long)threadIdx.x * kPlanQuad, px);
#pragma unroll
        for (int q = 0; q < kPlanQuad; q++) {
#pragma unroll
            for (int j = 0; j < kPlanCandidates; j++) acc[j] += plan_count(px[q], first + (uint32_t)j * step);
            n_live += px[q].live;
            n_saturated += px[q].saturated;
        }
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    Red red[kPlanCandidates];
#pragma unroll
    for (int j = 0; j < kPlanCandidates; j++) red[j] = (Red)acc[j];
    part[wave][lane] = (long long)wave_reduce_scatter(red);
    if (pass == 0) {
        const long long l = wave_sum((long long)n_live), t = wave_sum((long long)n_saturated);
        if (lane == 0) part[wave][kPlanCandidates] = l, part[wave][kPlanCandidates + 1] = t;
    }
    __syncthreads();
    const int slots = pass == 0 ? kPlanCandidates + 2 : kPlanCandidates;
    if ((int)threadIdx.x < slots) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kPlanBlock / 64; w++) v += part[w][threadIdx.x];
        long long *dst = (int)threadIdx.x < kPlanCandidates ? a.ws + kPlanWsTotals + pass * kPlanCandidates + threadIdx.x
                                                            : a.ws + kPlanWsLive + (threadIdx.x - kPlanCandidates);
        atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- the trim: exclusive prefix sum of d in raster order
// d of the lane's quad and c(u* - 1); with status 1 / 2 the count at the level and d = 0.
__device__ __forceinline__ void plan_quad_steps(const PlanArgs &a, const PlanSearch &s, long long p0, int (&base)[kPlanQuad], int (&d)[kPlanQuad]) {
    PlanPixel px[kPlanQuad];
    plan_load_quad(a, p0, px);
#pragma unroll
    for (int q = 0; q < kPlanQuad; q++) {
        base[q] = plan_count(px[q], s.lo);
        d[q] = plan_count(px[q], s.hi) - base[q];
    }
}

__global__ __launch_bounds__(kPlanBlock) void plan_block_sums_kernel(PlanArgs a) {
    __shared__ int wave_tot[kPlanBlock / 64];
    const PlanSearch s = plan_search(a.ws, a.budget, kPlanPasses);
    int base[kPlanQuad], d[kPlanQuad];
    plan_quad_steps(a, s, (long long)blockIdx.x * kPlanChunk + (long long)threadIdx.x * kPlanQuad, base, d);
    int total;
    block_exclusive_scan((d[0] + d[1]) + (d[2] + d[3]), wave_tot, total);   // at most 1024 * 2^20: an int
    if (threadIdx.x == 0) a.ws[kPlanWsBlocks + blockIdx.x] = total;
}

// One workgroup: the block sums become their exclusive prefix, 256 at a step; thread 0 writes the result.
__global__ __launch_bounds__(kPlanBlock) void plan_scan_blocks_kernel(PlanArgs a) {
    __shared__ long long wave_tot[kPlanBlock / 64];
    const PlanSearch s = plan_search(a.ws, a.budget, kPlanPasses);
    long long *blk = a.ws + kPlanWsBlocks;
    long long carry = 0;
    for (long long b0 = 0; b0 < a.n_chunks; b0 += kPlanBlock) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < a.n_chunks ? blk[b] : 0;
        long long total;
        const long long before = block_exclusive_scan(v, wave_tot, total);
        if (b < a.n_chunks) blk[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        statmc_plan_result r;
        const long long rest = a.budget - s.t_lo;     // status 0: in (0, carry], carry = T(u*) - T(u* - 1)
        r.total = s.status > 0 ? s.t_lo : s.t_lo + (rest < carry ? rest : carry);
        r.budget = a.budget;
        r.level_bits = s.hi;
        r.status = s.status > 0 ? s.status : 0;
        r.n_live = (int32_t)a.ws[kPlanWsLive];
        r.n_saturated = (int32_t)a.ws[kPlanWsSaturated];
        *a.result = r;
    }
}

__global__ __launch_bounds__(kPlanBlock) void plan_apply_kernel(PlanArgs a) {
    __shared__ int wave_tot[kPlanBlock / 64];
    const PlanSearch s = plan_search(a.ws, a.budget, kPlanPasses);
    const long long p0 = (long long)blockIdx.x * kPlanChunk + (long long)threadIdx.x * kPlanQuad;
    int base[kPlanQuad], d[kPlanQuad];
    plan_quad_steps(a, s, p0, base, d);
    int total;
    const int before = block_exclusive_scan((d[0] + d[1]) + (d[2] + d[3]), wave_tot, total);
    long long left = (a.budget - s.t_lo) - (a.ws[kPlanWsBlocks + blockIdx.x] + before);   // R - E_p of the quad's first pixel
    int c[kPlanQuad];
#pragma unroll
    for (int q = 0; q < kPlanQuad; q++) {
        const long long give = left < 0 ? 0 : left < d[q] ? left : d[q];
        c[q] = base[q] + (int)give;   // (status 1 / 2: d = 0)
        left -= d[q];
    }
    if (a.vec && p0 + kPlanQuad <= a.n_px) {
        *reinterpret_cast<int4 *>(a.counts + p0) = make_int4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int q = 0; q < kPlanQuad; q++)
            if (p0 + q < a.n_px) a.counts[p0 + q] = c[q];
    }
}

// ---------------------------------------------------------------- statmc_sample_scores
// Every operation rounds once (no contraction); `/` and sqrtf are the correctly rounded IEEE quotient and root.
template <int C>
__device__ __forceinline__ float score_pixel(int n, const float (&mean)[C], const float (&m2)[C], int metric, float eps) {
#pragma clang fp contract(off)
    if (n < 2) return __builtin_inff();
    const float fn = (float)(n - 1);
    float v = m2[0] / fn;
#pragma unroll
    for (int c = 1; c < C; c++) v = v + m2[c] / fn;
    const float sd = sqrtf(v);
    if (metric == STATMC_SCORE_ABSOLUTE) return sd;
    float m = fabsf(mean[0]);
#pragma unroll
    for (int c = 1; c < C; c++) m = m + fabsf(mean[c]);
    return sd / (eps + m);
}

template <int C>
__device__ __forceinline__ void load_quad_plane(const float *plane, long long p0, float (&t)[4 * C]) {
#pragma unroll
    for (int i = 0; i < C; i++) {
        const float4 x = reinterpret_cast<const float4 *>(plane + p0 * C)[i];
        t[4 * i] = x.x, t[4 * i + 1] = x.y, t[4 * i + 2] = x.z, t[4 * i + 3] = x.w;
    }
}

// One lane per 4 pixels: a full quad of 16-byte aligned planes moves as dwordx4 (1 + 2 C loads, one store); the film's last,
// partial quad and every quad of unaligned planes go element by element through the same score_pixel.
template <int C>
__global__ __launch_bounds__(kPlanBlock) void sample_scores_kernel(ScoreArgs a) {
    const long long p0 = ((long long)blockIdx.x * kPlanBlock + threadIdx.x) * 4;
    if (p0 >= a.n_px) return;
    if (a.vec && p0 + 4 <= a.n_px) {
        const int4 n = *reinterpret_cast<const int4 *>(a.n + p0);
        float mean[4 * C], m2[4 * C];
        load_quad_plane<C>(a.film_mean, p0, mean);
        load_quad_plane<C>(a.film_m2, p0, m2);
        const int nn[4] = {n.x, n.y, n.z, n.w};
        float out[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float pm[C], p2[C];
#pragma unroll
            for (int c = 0; c < C; c++) pm[c] = mean[q * C + c], p2[c] = m2[q * C + c];
            out[q] = score_pixel<C>(nn[q], pm, p2, a.metric, a.eps);
        }
        *reinterpret_cast<float4 *>(a.score + p0) = make_float4(out[0], out[1], out[2], out[3]);
        return;
    }
    for (long long p = p0; p < p0 + 4 && p < a.n_px; p++) {
        float pm[C], p2[C];
#pragma unroll
        for (int c = 0; c < C; c++) pm[c] = a.film_mean[p * C + c], p2[c] = a.film_m2[p * C + c];
        a.score[p] = score_pixel<C>(a.n[p], pm, p2, a.metric, a.eps);
    }
}

}  // namespace

hipError_t launch_sample_scores(const ScoreArgs &a, hipStream_t s) {
    const long long quads = (a.n_px + 3) / 4;
    const unsigned grid = (unsigned)((quads + kPlanBlock - 1) / kPlanBlock);
    if (a.channels == 3) hipLaunchKernelGGL(sample_scores_kernel<3>, dim3(grid), dim3(kPlanBlock), 0, s, a);
    else hipLaunchKernelGGL(sample_scores_kernel<1>, dim3(grid), dim3(kPlanBlock), 0, s, a);
    return hipGetLastError();
}

// The workspace is zeroed on the stream, then the eight launches follow each other on it.
hipError_t launch_plan_samples(const PlanArgs &a, size_t workspace_bytes, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.ws, 0, workspace_bytes, s);
    if (e != hipSuccess) return e;
    for (int pass = 0; pass < kPlanPasses; pass++) {
        const dim3 grid((unsigned)a.grid), block(kPlanBlock);
        if (a.wide) hipLaunchKernelGGL((plan_pass_kernel<long long, long long>), grid, block, 0, s, a, pass);
        else if (a.wide_wave) hipLaunchKernelGGL((plan_pass_kernel<int32_t, long long>), grid, block, 0, s, a, pass);
        else hipLaunchKernelGGL((plan_pass_kernel<int32_t, int32_t>), grid, block, 0, s, a, pass);
    }
    hipLaunchKernelGGL(plan_block_sums_kernel, dim3((unsigned)a.n_chunks), dim3(kPlanBlock), 0, s, a);
    hipLaunchKernelGGL(plan_scan_blocks_kernel, dim3(1), dim3(kPlanBlock), 0, s, a);
    hipLaunchKernelGGL(plan_apply_kernel, dim3((unsigned)a.n_chunks), dim3(kPlanBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_plan_samples_workspace(uint16_t width, uint16_t height) { return statmc::plan_workspace_bytes(width, height); }
