// statmc_score_sum.hip -- statmc_score_sum (include/statmc.h): the exact sum and sum of squares of a score image under up to four
// caps, on the device.  DESIGN.md 4.2i.
//
// Two launches on one stream behind the zeroing of the workspace, neither of which waits for another workgroup:
//   - score_sum_pass_kernel.  A pixel's value is the integer M << s (statmc_score_sum_args.h), its square M^2 << 2 s; both are added
//     into fixed-point integers of 32-bit limbs held in 64-bit words, one set per interval between the sorted caps.  A lane sums
//     the run of its pixels that share an interval and a 16-exponent band -- the same two limbs of the sum, the same three of the
//     square -- in five 64-bit registers and hands a finished run to the workgroup's table in LDS; the table goes to the workspace
//     as one 64-bit atomicAdd per non-zero (interval, limb) and workgroup.  A converged film is one run per lane: no atomic in the
//     loop at all.
//   - score_sum_result_kernel, one lane per cap: carries, the capped totals, the rounding (sum_finalize_slot), the result.
// Everything added is an integer, so the order of the atomics reaches no bit.
#include "statmc_device.h"
#include "statmc_score_sum_args.h"

namespace statmc {

namespace {

constexpr int kSumWaves = kSelectBlock / 64;
constexpr int kSumTable = kSumIntervals * (kSumLimbs + kSumSqLimbs);   // 64-bit words of LDS: the sums' limbs, then the squares'
constexpr int kSumCounters = 2 + kSumIntervals;                        // zero, infinite, the intervals' pixels
static_assert(kSumTable <= kSelectBlock, "one thread per word when the table is flushed");
static_assert(kSumWsSq == kSumWsSum + kSumIntervals * kSumLimbs && kSumWsCount == kSumWsInfinite + 1 && kSumWsInfinite == kSumWsZero + 1,
              "the table and the counters go to the workspace in their own order");

// Pixels p0 .. p0 + 3, p0 a multiple of 4: with a 16-byte aligned image a full quad moves as one dwordx4.
__device__ __forceinline__ void sum_load_quad(const float *score, int vec, long long n_px, long long p0, uint32_t (&key)[kSelectQuad],
                                              bool (&inside)[kSelectQuad]) {
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(score);
    uint32_t b[kSelectQuad];
    if (vec && p0 + kSelectQuad <= n_px) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bits + p0);
        b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < kSelectQuad; q++) b[q] = p0 + q < n_px ? bits[p0 + q] : 0u;
    }
#pragma unroll
    for (int q = 0; q < kSelectQuad; q++) {
        inside[q] = p0 + q < n_px;
        key[q] = select_key(b[q]);
    }
}

__device__ __forceinline__ unsigned long long sum_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A lane's run: group = interval * 16 + (s >> 4), -1 none.  s >> 4 fixes the limbs: the sum's are (s >> 5), + 1; the square's
// (2 s >> 5) = (s >> 4), + 1, + 2.
struct SumRun {
    int group;
    unsigned long long lo, hi, q0, q1, q2;   // a pixel adds less than 2^32 to each, a film has fewer than 2^32 pixels
};

__device__ __forceinline__ void sum_flush(unsigned long long *table, const SumRun &r) {
    if (r.group < 0) return;
    const int t = r.group >> 4, band = r.group & 15;
    unsigned long long *sum = table + t * kSumLimbs + (band >> 1);
    unsigned long long *sq = table + kSumIntervals * kSumLimbs + t * kSumSqLimbs + band;
    if (r.lo) atomicAdd(sum, r.lo);
    if (r.hi) atomicAdd(sum + 1, r.hi);
    if (r.q0) atomicAdd(sq, r.q0);
    if (r.q1) atomicAdd(sq + 1, r.q1);
    if (r.q2) atomicAdd(sq + 2, r.q2);
}

__global__ __launch_bounds__(kSelectBlock) void score_sum_pass_kernel(SumArgs a) {
    __shared__ unsigned long long table[kSumTable];
    __shared__ unsigned long long part[kSumWaves][kSumCounters];
    if (threadIdx.x < kSumTable) table[threadIdx.x] = 0;
    __syncthreads();
    int count[kSumCounters];   // a lane has fewer than 2^31 pixels
#pragma unroll
    for (int j = 0; j < kSumCounters; j++) count[j] = 0;
    SumRun run = {-1, 0, 0, 0, 0, 0};
    for (long long chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        uint32_t key[kSelectQuad];
        bool inside[kSelectQuad];
        sum_load_quad(a.score, a.vec, a.n_px, chunk * kSelectChunk + (long long)threadIdx.x * kSelectQuad, key, inside);
#pragma unroll
        for (int q = 0; q < kSelectQuad; q++) {
            const uint32_t k = key[q];
            const bool finite = inside[q] && k != 0 && k < kSumInfinite;
            int t = 0;   // the number of caps below the key
#pragma unroll
            for (int j = 0; j < STATMC_SUM_MAX_CAPS; j++) t += k > a.sorted[j];
            count[0] += inside[q] && k == 0;
            count[1] += inside[q] && k == kSumInfinite;
#pragma unroll
            for (int j = 0; j < kSumIntervals; j++) count[2 + j] += finite && t == j;
            if (finite) {
                const uint32_t M = sum_significand(k);
                const int s = sum_shift(k);
                const int group = t * 16 + (s >> 4);
                if (group != run.group) {
                    sum_flush(table, run);
                    run = SumRun{group, 0, 0, 0, 0, 0};
                }
                const unsigned long long v = (unsigned long long)M << (s & 31);
                const unsigned long long sq = (unsigned long long)M * M;
                const int sh = (2 * s) & 31;
                const unsigned long long upper = sq >> (32 - sh);   // a shift of 1 .. 32
                run.lo += (uint32_t)v, run.hi += v >> 32;
                run.q0 += (uint32_t)(sq << sh), run.q1 += (uint32_t)upper, run.q2 += upper >> 32;
            }
        }
    }
    // the last runs: a wave whose lanes all ended in the same group (a converged film) adds them up first
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (__all(run.group == __builtin_amdgcn_readfirstlane(run.group))) {
        run.lo = sum_wave_sum(run.lo), run.hi = sum_wave_sum(run.hi);
        run.q0 = sum_wave_sum(run.q0), run.q1 = sum_wave_sum(run.q1), run.q2 = sum_wave_sum(run.q2);
        if (lane == 0) sum_flush(table, run);
    } else {
        sum_flush(table, run);
    }
#pragma unroll
    for (int j = 0; j < kSumCounters; j++) {
        const unsigned long long v = sum_wave_sum((unsigned long long)count[j]);
        if (lane == 0) part[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSumTable) {
        const unsigned long long v = table[threadIdx.x];
        if (v) atomicAdd(a.ws + kSumWsSum + threadIdx.x, v);
    }
    if (threadIdx.x < kSumCounters) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kSumWaves; w++) v += part[w][threadIdx.x];
        if (v) atomicAdd(a.ws + kSumWsZero + threadIdx.x, v);
    }
}

// One lane per slot: the totals are complete behind the pass on the stream.  Lane j forms slot j (a slot behind n_caps is written as
// 0), lane 0 the counts as well.  A slot is a chain of dependent private-memory accesses, some hundreds long; one lane doing the
// four in turn took 15 us per cap.
__global__ __launch_bounds__(64) void score_sum_result_kernel(SumArgs a) {
    const int j = (int)threadIdx.x;
    if (j >= STATMC_SUM_MAX_CAPS || blockIdx.x != 0) return;
    const uint64_t *ws = reinterpret_cast<const uint64_t *>(a.ws);
    statmc_sum_result *r = a.result;
    if (j == 0) {
        int64_t finite = 0;
        for (int t = 0; t < kSumIntervals; t++) finite += (int64_t)ws[kSumWsCount + t];
        r->n_px = a.n_px;
        r->n_zero = (int64_t)ws[kSumWsZero];
        r->n_finite = finite;
        r->n_infinite = (int64_t)ws[kSumWsInfinite];
        r->n_caps = a.n_caps;
        r->pad = 0;
    }
    uint64_t sum_bits = 0, sq_bits = 0;
    int64_t clipped = 0;
    if (j < a.n_caps) sum_finalize_slot(ws, a.cap_key[j], a.under[j], &clipped, &sum_bits, &sq_bits);
    r->cap_bits[j] = j < a.n_caps ? a.cap_key[j] : 0u;
    r->n_clipped[j] = clipped;
    r->sum[j] = __longlong_as_double((long long)sum_bits);
    r->sum_sq[j] = __longlong_as_double((long long)sq_bits);
}

}  // namespace

// The workspace is zeroed on the stream, then the two launches follow each other on it.
hipError_t launch_score_sum(const SumArgs &a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.ws, 0, sum_workspace_bytes(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_sum_pass_kernel, dim3((unsigned)a.grid), dim3(kSelectBlock), 0, s, a);
    hipLaunchKernelGGL(score_sum_result_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_score_sum_workspace(void) { return statmc::sum_workspace_bytes(); }
