// statmc_select.hip -- statmc_score_select and statmc_score_count_above (include/statmc.h): exact order statistics and threshold
// counts of a score image, on the device.  DESIGN.md 4.2e.
//
// The select is a most-significant-digit radix select over the keys (statmc_select_args.h: select_key), four digits of 8 bits, in
// five launches on one stream behind the zeroing of the workspace, none of which waits for another workgroup:
//   - kSelectPasses = 4 passes (select_pass_kernel).  A pass histograms one digit of the keys into LDS and flushes one 64-bit
//     atomicAdd per non-empty bin and workgroup into the workspace.  Pass 0 counts every pixel in one histogram; pass q >= 1 counts
//     the pixels under the prefix (top q digits) that holds a rank, one histogram per distinct prefix.  Every workgroup derives
//     those prefixes itself from the totals of the passes before (select_derive): the search never leaves the device.
//   - select_result_kernel, one workgroup: the same derivation over all four passes, and the result.
// Counts are integers, so the order of the atomics reaches no bit.  Within a wave, lanes that hit the same bin are merged before
// the LDS atomic (wave_match): a film of one constant score costs one atomic per wave and step, not 64 on one address.
#include "statmc_device.h"
#include "statmc_scan.h"
#include "statmc_select_args.h"

namespace statmc {

namespace {

constexpr int kSelectWaves = kSelectBlock / 64;
constexpr int kSelectIndexBits = kSelectDigitBits + 3;   // slot * 256 + digit

// ---------------------------------------------------------------- the keys of a lane's quad
// Pixels p0 .. p0 + 3, p0 a multiple of 4: with a 16-byte aligned image a full quad moves as one dwordx4.  Pixels past the film's
// end are not inside.
__device__ __forceinline__ void select_load_quad(const float *score, int vec, long long n_px, long long p0, uint32_t (&key)[kSelectQuad],
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

// ---------------------------------------------------------------- the search state, from the workspace
// What the first `passes` passes' histograms say about every rank.  After q passes: prefix holds the top q digits of the rank's
// key (the rest 0), rem the rank's position among the pixels under that prefix, below the number of pixels whose key is smaller
// than every key under the prefix, equal the number of pixels under it; slot[i] is the smallest j with prefix[j] == prefix[i], the
// histogram the next pass counts rank i's pixels in.
struct SelectState {
    uint32_t prefix[STATMC_SELECT_MAX_RANKS];
    int slot[STATMC_SELECT_MAX_RANKS];
    long long rem[STATMC_SELECT_MAX_RANKS], below[STATMC_SELECT_MAX_RANKS], equal[STATMC_SELECT_MAX_RANKS];
};

// The whole workgroup calls this; st is in LDS and complete on return.  A wave takes the ranks wave, wave + 4: its lanes read four
// bins each of the rank's histogram, scan them, and the one lane whose bins hold position rem steps the state.  The histogram's
// total is the `equal` of the pass before (n_px for pass 0), which is above rem: exactly one lane steps.
__device__ __forceinline__ void select_derive(const SelectArgs &a, int passes, SelectState &st) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x < STATMC_SELECT_MAX_RANKS) {
        const int i = (int)threadIdx.x;
        st.prefix[i] = 0, st.slot[i] = 0, st.below[i] = 0;
        st.rem[i] = i < a.n_ranks ? a.rank[i] : 0;
        st.equal[i] = i < a.n_ranks ? a.n_px : 0;
    }
    __syncthreads();
    for (int q = 0; q < passes; q++) {
        for (int i = wave; i < a.n_ranks; i += kSelectWaves) {
            const long long *h = a.ws + select_hist_word(q, st.slot[i]) + 4 * lane;
            const long long c[4] = {h[0], h[1], h[2], h[3]};
            const long long mine = (c[0] + c[1]) + (c[2] + c[3]);
            const long long incl = wave_inclusive_scan(mine);
            const long long r = st.rem[i];
            long long before = incl - mine;
            if (before <= r && r < incl) {
                int d = 0;
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (d == k && r >= before + c[k]) before += c[k], d = k + 1;
                st.prefix[i] |= (uint32_t)(4 * lane + d) << (32 - kSelectDigitBits * (q + 1));
                st.rem[i] = r - before;
                st.below[i] += before;
                st.equal[i] = c[d];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < a.n_ranks) {
            const int i = (int)threadIdx.x;
            int s = i;
            for (int j = i - 1; j >= 0; j--)
                if (st.prefix[j] == st.prefix[i]) s = j;
            st.slot[i] = s;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- merging a wave's equal indices
// The lanes of the wave that are `valid` and hold the same idx (BITS bits) as this lane, by one ballot per bit: no loop whose
// length depends on the data.  Every lane of the wave calls this.
template <int BITS>
__device__ __forceinline__ unsigned long long wave_match(uint32_t idx, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const bool set = (idx >> b) & 1u;
        const unsigned long long s = __ballot(set);
        m &= set ? s : ~s;
    }
    return m;
}
// hist[idx] += the number of the wave's valid lanes with this idx, by the lowest of them
template <int BITS>
__device__ __forceinline__ void wave_hist_add(uint32_t *hist, uint32_t idx, bool valid) {
    if (__ballot(valid) == 0ull) return;   // (wave-uniform)
    const unsigned long long m = wave_match<BITS>(idx, valid);
    const int lane = (int)(threadIdx.x & 63);
    if (valid && __ffsll((long long)m) - 1 == lane) atomicAdd(&hist[idx], (uint32_t)__popcll(m));
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------- a pass
// LDS: slot s's histogram at hist[s * 256 ..]; a workgroup's counts stay below 2^32 (a film has fewer pixels).
__global__ __launch_bounds__(kSelectBlock) void select_pass_kernel(SelectArgs a, int pass) {
    __shared__ uint32_t hist[STATMC_SELECT_MAX_RANKS * kSelectBins];
    __shared__ uint32_t classes[2];
    __shared__ SelectState st;
    select_derive(a, pass, st);
    // the distinct prefixes of this pass, as (prefix, slot) pairs every lane holds; pass 0 has the one empty prefix, slot 0
    uint32_t want[STATMC_SELECT_MAX_RANKS];
    bool leads[STATMC_SELECT_MAX_RANKS];
#pragma unroll
    for (int i = 0; i < STATMC_SELECT_MAX_RANKS; i++) {
        leads[i] = pass == 0 ? i == 0 : (i < a.n_ranks && st.slot[i] == i);
        want[i] = st.prefix[i];
    }
    const int n_hist = pass == 0 ? 1 : a.n_ranks;
    // one distinct prefix (one rank, or all ranks in one run as on a constant film): the slot is the same in every counted lane and
    // the digit's 8 ballots tell them apart
    // (rank 0 always leads slot 0)
    int n_leads = 0;
#pragma unroll
    for (int i = 0; i < STATMC_SELECT_MAX_RANKS; i++) n_leads += leads[i];
    const bool one_slot = __builtin_amdgcn_readfirstlane(n_leads) == 1;   // (the same in every lane: a scalar branch)
    for (int k = (int)threadIdx.x; k < n_hist * kSelectBins; k += kSelectBlock) hist[k] = 0;
    if (threadIdx.x < 2) classes[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 32 - kSelectDigitBits * (pass + 1);           // of this pass's digit
    const uint32_t above = pass == 0 ? 0u : ~0u << (shift + kSelectDigitBits);   // the bits of the prefix
    int n_live = 0, n_saturated = 0;
    for (long long chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        uint32_t key[kSelectQuad];
        bool inside[kSelectQuad];
        select_load_quad(a.score, a.vec, a.n_px, chunk * kSelectChunk + (long long)threadIdx.x * kSelectQuad, key, inside);
#pragma unroll
        for (int q = 0; q < kSelectQuad; q++) {
            const uint32_t digit = (key[q] >> shift) & (uint32_t)(kSelectBins - 1);
            if (pass == 0) {
                wave_hist_add<kSelectDigitBits>(hist, digit, inside[q]);
                n_live += inside[q] && key[q] >= kSelectLiveLo && key[q] <= kSelectLiveHi;
                n_saturated += inside[q] && key[q] > kSelectLiveHi;
            } else {
                int slot = -1;
#pragma unroll
                for (int i = 0; i < STATMC_SELECT_MAX_RANKS; i++)
                    if (leads[i] && (key[q] & above) == want[i]) slot = i;
                const bool valid = inside[q] && slot >= 0;
                if (one_slot) wave_hist_add<kSelectDigitBits>(hist, digit, valid);
                else wave_hist_add<kSelectIndexBits>(hist, (uint32_t)(valid ? slot : 0) * kSelectBins + digit, valid);
            }
        }
    }
    if (pass == 0) {
        const long long l = wave_sum((long long)n_live), t = wave_sum((long long)n_saturated);
        if ((threadIdx.x & 63) == 0) atomicAdd(&classes[0], (uint32_t)l), atomicAdd(&classes[1], (uint32_t)t);
    }
    __syncthreads();
    for (int s = 0; s < n_hist; s++) {
        if (!leads[s]) continue;   // (the same in every lane)
        const uint32_t v = hist[s * kSelectBins + threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(a.ws + select_hist_word(pass, s) + threadIdx.x), (unsigned long long)v);
    }
    if (pass == 0 && threadIdx.x < 2 && classes[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long *>(a.ws + kSelectWsLive + threadIdx.x), (unsigned long long)classes[threadIdx.x]);
}

// One workgroup: the state after all passes is the answer.
__global__ __launch_bounds__(kSelectBlock) void select_result_kernel(SelectArgs a) {
    __shared__ SelectState st;
    select_derive(a, kSelectPasses, st);
    if (threadIdx.x == 0) {
        statmc_select_result r;
        r.n_px = a.n_px;
        r.n_live = a.ws[kSelectWsLive];
        r.n_saturated = a.ws[kSelectWsSaturated];
        r.n_ranks = a.n_ranks;
        r.pad = 0;
        for (int i = 0; i < STATMC_SELECT_MAX_RANKS; i++) {
            const bool asked = i < a.n_ranks;
            r.rank[i] = asked ? a.rank[i] : 0;
            r.value_bits[i] = asked ? st.prefix[i] : 0u;
            r.n_below[i] = asked ? st.below[i] : 0;
            r.n_equal[i] = asked ? st.equal[i] : 0;
        }
        *a.result = r;
    }
}

// ---------------------------------------------------------------- statmc_score_count_above
// One pass: a lane counts its pixels above each threshold's key in registers (a lane has fewer than 2^31 pixels), a wave adds its
// lanes, the workgroup's waves meet in LDS, and one 64-bit atomicAdd per threshold and workgroup lands in counts.
__global__ __launch_bounds__(kSelectBlock) void count_above_kernel(CountAboveArgs a) {
    __shared__ long long part[kSelectWaves][STATMC_SELECT_MAX_RANKS];
    int c[STATMC_SELECT_MAX_RANKS];
#pragma unroll
    for (int j = 0; j < STATMC_SELECT_MAX_RANKS; j++) c[j] = 0;
    for (long long chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        uint32_t key[kSelectQuad];
        bool inside[kSelectQuad];
        select_load_quad(a.score, a.vec, a.n_px, chunk * kSelectChunk + (long long)threadIdx.x * kSelectQuad, key, inside);
#pragma unroll
        for (int q = 0; q < kSelectQuad; q++)
#pragma unroll
            for (int j = 0; j < STATMC_SELECT_MAX_RANKS; j++) c[j] += inside[q] && j < a.n_thresholds && key[q] > a.key[j];
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int j = 0; j < STATMC_SELECT_MAX_RANKS; j++) {
        const long long v = wave_sum((long long)c[j]);
        if (lane == 0) part[wave][j] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.n_thresholds) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kSelectWaves; w++) v += part[w][threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + threadIdx.x), (unsigned long long)v);
    }
}

}  // namespace

// The workspace is zeroed on the stream, then the five launches follow each other on it.
hipError_t launch_score_select(const SelectArgs &a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.ws, 0, select_workspace_bytes(), s);
    if (e != hipSuccess) return e;
    for (int pass = 0; pass < kSelectPasses; pass++)
        hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)a.grid), dim3(kSelectBlock), 0, s, a, pass);
    hipLaunchKernelGGL(select_result_kernel, dim3(1), dim3(kSelectBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_score_count_above(const CountAboveArgs &a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.n_thresholds * sizeof(long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(count_above_kernel, dim3((unsigned)a.grid), dim3(kSelectBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_score_select_workspace(void) { return statmc::select_workspace_bytes(); }
