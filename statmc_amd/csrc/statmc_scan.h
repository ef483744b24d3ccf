// statmc_scan.h -- the prefix sums the scan kernels share: a wave's inclusive scan through cross-lane shuffles and a workgroup's
// exclusive scan on top of it.  statmc_plan.hip's trim and statmc_compact.hip's offsets both run the same three launches over
// them: per-block sums, one workgroup over the block sums, the apply.  Device code only; no kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>

namespace statmc {

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}
// exclusive prefix of v over the workgroup's 64 * NW threads in thread order, and the workgroup's total
template <typename T, int NW>
__device__ __forceinline__ T block_exclusive_scan(T v, T (&wave_tot)[NW], T &total) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const T incl = wave_inclusive_scan(v);
    __syncthreads();   // the previous use of wave_tot is over
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        if (w < wave) before += wave_tot[w];
        total += wave_tot[w];
    }
    return before + incl - v;
}

}  // namespace statmc
