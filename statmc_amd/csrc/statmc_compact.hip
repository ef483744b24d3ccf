// statmc_compact.hip -- statmc_compact_offsets and statmc_compact_accumulate (include/statmc.h): the compact (CSR) arena of a planned
// iteration, every pixel's samples back to back and the pixels in raster order (gfx950).  DESIGN.md 4.1j.
//
//   offsets   the exclusive prefix sum of the clamped count image in three ordinary launches, the shape of statmc_plan_samples' trim
//             (statmc_scan.h): per-block sums, one workgroup over the block sums (which also writes offsets[n_px], the total), the
//             apply.  Integer sums: the same bits on every run.  owners[] is one more launch over the slots: slot i finds its pixel
//             by bisection in offsets[] (21 steps at 1080p, every probe a cached line its neighbours share), so a pixel with 2^20
//             samples costs its slots what any other pixel's cost; slots at or behind the total get -1.
//   fold      one lane per pixel and stat type: the lane reads offsets[p] and offsets[p + 1], clamps them into the arena
//             (compact_run, statmc_compact_args.h) BEFORE anything is derived from them, and folds its run in ascending position
//             with statmc::device::PixelStats (load, add, store): the bits statmc_accumulate_records leaves for the same samples.
//             A run above split_above is folded by the 64 lanes of the wave under the split entries' definition: the chunks are
//             records_split_chunk's (statmc_records_plan.h), the merge is statmc::device::merge_lanes<64>.  Positions are 64-bit:
//             the records fold's 32-bit run starts and its order[] array have no counterpart here, which is why this file has a
//             walk of its own; nothing of the arithmetic is restated.
#include "statmc_device.h"
#include "statmc_compact_args.h"
#include "statmc_scan.h"
#define STATMC_PLAN_HOST_DEVICE __host__ __device__      // records_split_chunk runs in the fold
#include "statmc_records_plan.h"

#include "../../include/statmc_device_api.hpp"

namespace statmc {

namespace {

// ---------------------------------------------------------------- offsets
// c(p) of the lane's quad: pixels p0 .. p0 + 3, those past the film's end counted as nothing.  p0 is a multiple of 4.
__device__ __forceinline__ void compact_load_quad(const CompactOffsetsArgs &a, long long p0, long long (&c)[kCompactQuad]) {
    int v[kCompactQuad] = {0, 0, 0, 0};
    if (a.vec && p0 + kCompactQuad <= a.n_px) {
        const int4 x = *reinterpret_cast<const int4 *>(a.counts + p0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
#pragma unroll
        for (int q = 0; q < kCompactQuad; q++)
            if (p0 + q < a.n_px) v[q] = a.counts[p0 + q];
    }
#pragma unroll
    for (int q = 0; q < kCompactQuad; q++) c[q] = (long long)min(max(v[q], 0), a.cap);
}

__global__ __launch_bounds__(kCompactBlock) void compact_block_sums_kernel(CompactOffsetsArgs a) {
    __shared__ long long wave_tot[kCompactBlock / 64];
    long long c[kCompactQuad];
    compact_load_quad(a, (long long)blockIdx.x * kCompactChunk + (long long)threadIdx.x * kCompactQuad, c);
    long long total;
    block_exclusive_scan((c[0] + c[1]) + (c[2] + c[3]), wave_tot, total);
    if (threadIdx.x == 0) a.ws[blockIdx.x] = total;
}

// One workgroup: the block sums become their exclusive prefix, 256 at a step; thread 0 writes the total behind the film's offsets.
__global__ __launch_bounds__(kCompactBlock) void compact_scan_blocks_kernel(CompactOffsetsArgs a) {
    __shared__ long long wave_tot[kCompactBlock / 64];
    long long carry = 0;
    for (long long b0 = 0; b0 < a.n_chunks; b0 += kCompactBlock) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < a.n_chunks ? a.ws[b] : 0;
        long long total;
        const long long before = block_exclusive_scan(v, wave_tot, total);
        if (b < a.n_chunks) a.ws[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) a.offsets[a.n_px] = carry;
}

__global__ __launch_bounds__(kCompactBlock) void compact_apply_kernel(CompactOffsetsArgs a) {
    __shared__ long long wave_tot[kCompactBlock / 64];
    const long long p0 = (long long)blockIdx.x * kCompactChunk + (long long)threadIdx.x * kCompactQuad;
    long long c[kCompactQuad];
    compact_load_quad(a, p0, c);
    long long total;
    long long at = a.ws[blockIdx.x] + block_exclusive_scan((c[0] + c[1]) + (c[2] + c[3]), wave_tot, total);
#pragma unroll
    for (int q = 0; q < kCompactQuad; q++) {
        if (p0 + q < a.n_px) a.offsets[p0 + q] = at;
        at += c[q];
    }
}

// Slot i's pixel: the p with offsets[p] <= i < offsets[p + 1].  Invariant of the bisection: offsets[lo] <= i < offsets[hi].
__global__ __launch_bounds__(kCompactBlock) void compact_owners_kernel(CompactOffsetsArgs a) {
    const long long total = a.offsets[a.n_px];
    for (long long i = (long long)blockIdx.x * kCompactBlock + threadIdx.x; i < a.owners_capacity; i += (long long)gridDim.x * kCompactBlock) {
        int32_t owner = -1;
        if (i < total) {
            long long lo = 0, hi = a.n_px;
            while (hi - lo > 1) {
                const long long mid = (lo + hi) >> 1;
                if (a.offsets[mid] <= i) lo = mid;
                else hi = mid;
            }
            owner = (int32_t)lo;
        }
        a.owners[i] = owner;
    }
}

// ---------------------------------------------------------------- a sample, and the walk over a run
typedef unsigned compact_uint3 __attribute__((ext_vector_type(3), aligned(4)));   // an RGB sample starts at any 4-byte boundary

// The loaded words of one sample between request and fold: what is in flight stays raw, a half is widened when it is folded.
template <int C>
struct CompactRaw {
    unsigned r[C];
};
template <int C, bool HALF>
__device__ __forceinline__ void compact_request(const char *__restrict__ at, CompactRaw<C> &s) {
    if constexpr (HALF) {
        const unsigned short *h = reinterpret_cast<const unsigned short *>(at);
#pragma unroll
        for (int c = 0; c < C; c++) s.r[c] = h[c];
    } else if constexpr (C == 3) {
        const compact_uint3 x = *reinterpret_cast<const compact_uint3 *>(at);   // one dwordx3
        s.r[0] = x.x, s.r[1] = x.y, s.r[2] = x.z;
    } else {
        s.r[0] = *reinterpret_cast<const unsigned *>(at);
    }
}
template <int C, bool HALF, class PS>
__device__ __forceinline__ void compact_add(PS &ps, const CompactRaw<C> &s) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        if constexpr (HALF) v[c] = (float)__builtin_bit_cast(_Float16, (unsigned short)s.r[c]);   // every half is an fp32 value
        else v[c] = __uint_as_float(s.r[c]);
    }
    ps.add(v);
}

constexpr int kCompactBatch = 4;   // samples per request group; one group is in flight behind the one being folded

// The walk over the cnt samples that start at `run`, in ascending position.  Batches of four in two register sets: past the last
// whole batch the requests repeat the run's last four samples (inside the run, never folded), so the loop has no branch between a
// request and the fold in front of it.
template <int C, bool HALF, class PS>
__device__ __forceinline__ void compact_walk(const char *__restrict__ run, int cnt, PS &ps) {
    constexpr long long kStride = C * (HALF ? 2 : 4);
    int j = 0;
    if (cnt >= kCompactBatch) {
        const int last = cnt - kCompactBatch;
        CompactRaw<C> A[kCompactBatch], B[kCompactBatch];
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++) compact_request<C, HALF>(run + u * kStride, A[u]);
        // batch 0 passes through an empty asm: loaded in front of the loop AND in it, it would become one load at the loop's head
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++)
#pragma unroll
            for (int c = 0; c < C; c++) asm("" : "+v"(A[u].r[c]));
        // invariant: A = the samples of batch j / 4 (requested)
        for (; j + 2 * kCompactBatch <= cnt; j += 2 * kCompactBatch) {
            const char *b = run + (long long)min(j + kCompactBatch, last) * kStride;
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) compact_request<C, HALF>(b + u * kStride, B[u]);
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) compact_add<C, HALF>(ps, A[u]);
            const char *a = run + (long long)min(j + 2 * kCompactBatch, last) * kStride;
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) compact_request<C, HALF>(a + u * kStride, A[u]);
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) compact_add<C, HALF>(ps, B[u]);
        }
        if (j + kCompactBatch <= cnt) {   // an odd number of whole batches: the last one is in A
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) compact_add<C, HALF>(ps, A[u]);
            j += kCompactBatch;
        }
    }
    for (; j < cnt; j++) {   // the last cnt % 4 samples, and runs shorter than a batch
        CompactRaw<C> s;
        compact_request<C, HALF>(run + (long long)j * kStride, s);
        compact_add<C, HALF>(ps, s);
    }
}

// with the pre-pass epilogue where the type asks for it (mean_corr; max_moment 3 only)
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void compact_store(const device::PixelStats<C, MAXM, TRANSFORM> &ps, const statmc_stat_type &t, long long p,
                                              const statmc_prepass_context &ctx) {
    if constexpr (MAXM >= 3) {
        if (t.mean_corr != nullptr) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// ---------------------------------------------------------------- the fold of one stat type, straight from global memory
//   phase 1   a lane with 0 < cnt <= split_above folds its own run: the sequential records entry's bits.
//   phase 2   (SPLIT) m = ballot(cnt > split_above).  For every set bit in ascending lane order -- a wave-uniform loop -- all 64
//             lanes take that lane's (start, cnt) by __shfl, walk their chunk of it (records_split_chunk; an empty chunk issues no
//             load), merge (merge_lanes<64>), and lane 0 stores: the split records entry's bits.  No lane has left the wave.
template <int C, int MAXM, bool TRANSFORM, bool HALF, bool SPLIT>
__device__ __forceinline__ void compact_fold(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, long long start, int cnt,
                                             int split_above) {
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    const char *arena = reinterpret_cast<const char *>(t.samples);
    if (cnt > 0 && (!SPLIT || cnt <= split_above)) {
        PS ps;
        ps.load(t, p);
        compact_walk<C, HALF>(arena + compact_sample_byte(start, 0, C, HALF), cnt, ps);
        compact_store(ps, t, p, ctx);
    }
    if constexpr (SPLIT) {
        static_assert(kRecSplitLanes == 64, "a split pixel's slots are the lanes of one wave");
        const int lane = (int)(threadIdx.x & 63u);
        const long long p0 = p - lane;   // the wave's first pixel
        for (unsigned long long m = __ballot(cnt > split_above); m != 0; m &= m - 1) {
            const int from = __ffsll((long long)m) - 1;
            const long long s0 = __shfl(start, from, 64);
            const int c0 = __shfl(cnt, from, 64);
            int begin, len;
            records_split_chunk(c0, lane, &begin, &len);
            PS ps;
            if (lane == 0) ps.load(t, p0 + from);
            else ps.clear();
            compact_walk<C, HALF>(arena + compact_sample_byte(s0, begin, C, HALF), len, ps);
            device::merge_lanes<kRecSplitLanes>(ps);
            if (lane == 0) compact_store(ps, t, p0 + from, ctx);
        }
    }
}

// THE type dispatch: a block-uniform stat type and its format to the compile-time C, MAXM, TRANSFORM, HALF of Fold::run
template <class Fold, int C, bool HALF, class... A>
__device__ __forceinline__ void compact_dispatch_moments(const statmc_stat_type &t, A... a) {
    if (t.transform) {
        if (t.max_moment >= 3) Fold::template run<C, 3, true, HALF>(t, a...);
        else if (t.max_moment == 2) Fold::template run<C, 2, true, HALF>(t, a...);
        else Fold::template run<C, 1, true, HALF>(t, a...);
    } else {
        if (t.max_moment >= 3) Fold::template run<C, 3, false, HALF>(t, a...);
        else if (t.max_moment == 2) Fold::template run<C, 2, false, HALF>(t, a...);
        else Fold::template run<C, 1, false, HALF>(t, a...);
    }
}
template <class Fold, class... A>
__device__ __forceinline__ void compact_dispatch_type(const statmc_stat_type &t, bool half, A... a) {
    if (t.channels == 3) {
        if (half) compact_dispatch_moments<Fold, 3, true>(t, a...);
        else compact_dispatch_moments<Fold, 3, false>(t, a...);
    } else {
        if (half) compact_dispatch_moments<Fold, 1, true>(t, a...);
        else compact_dispatch_moments<Fold, 1, false>(t, a...);
    }
}

template <bool SPLIT>
struct DirectFold {
    template <int C, int MAXM, bool TRANSFORM, bool HALF>
    static __device__ __forceinline__ void run(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, long long start, int cnt,
                                               int split_above) {
        compact_fold<C, MAXM, TRANSFORM, HALF, SPLIT>(t, ctx, p, start, cnt, split_above);
    }
};

// Workgroup b serves stat type b % n_types and pixels [256 (b / n_types), + 256): the types of one pixel block run side by side and
// share its offsets[] lines in cache.  Not SPLIT: a lane past the film or with an empty run leaves.  SPLIT: no lane returns early --
// the wave's lanes meet again in phase 2 --, such a lane carries cnt = 0 and stays.
template <bool SPLIT>
__global__ __launch_bounds__(kCompactBlock) void compact_direct_kernel(CompactArgs a) {
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kCompactBlock + threadIdx.x;
    if (!SPLIT && p >= a.n_px) return;
    int64_t start = 0, end = 0;
    if (!SPLIT || p < a.n_px) compact_run(a.offsets[p], a.offsets[p + 1], a.n_samples, &start, &end);   // the clamp, first
    const int cnt = compact_run_count(start, end);
    if (!SPLIT && cnt <= 0) return;
    // COPIED out of the by-value argument: a reference into it keeps the whole argument in scratch
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const bool half = (a.half_mask >> ti) & 1u;
    compact_dispatch_type<DirectFold<SPLIT>>(t, half, ctx, p, (long long)start, cnt, a.split_above);
}

// ---------------------------------------------------------------- the staged fold: a wave's span through LDS
// The runs of a wave's 64 consecutive pixels tile one contiguous span of the arena: [start of lane 0, end of lane 63).  Where that
// span -- with the bytes in front of it down to a 16-byte boundary, the skew -- fits the wave's kStageWaveBytes of LDS, the wave
// lands it there in whole 16-byte pieces by LDS-DMA (global_load_lds_dwordx4: 1 KiB per instruction, full memory lines, no lane
// dragging a line of its own through L1), waits once, and every lane folds its run out of LDS with all 64 lanes at work.  A span
// that does not fit is NOT walked through a ring: a window of the span holds the runs of a few pixels only, the lanes of the
// others would idle, and the fold is VALU work as much as it is memory traffic.  Such a wave, a wave with a run
// above split_above, and a wave whose clamped runs do not tile a span (wrong offsets) take compact_fold, the direct fold, in the
// same kernel: the decision is wave-uniform.
//   - Source pieces: the span's first piece is its first byte's address rounded DOWN to 16, the last piece holds its last byte.  A
//     piece shares a 16-byte line with a byte of the arena, so it is memory that exists; what a piece holds beyond the span is
//     never folded.  A DMA slot behind the last piece re-reads the last piece.
//   - LDS layout: the destination of a DMA is lane-linear, the source address is per lane, so the swizzle is on the source side:
//     LDS piece q holds span piece q ^ ((q >> 3) & 7) (an involution: bits 3 .. 5 stay).  Lanes read at a common stride of
//     c * channels * 4 bytes when the counts are uniform (16 RGB fp32 samples: 48 dwords, two banks for 32 lanes); the XOR folds
//     bits of the piece's row into its place in the row and spreads them.
// per wave; four waves: 48 KiB per workgroup, three workgroups per CU.  16 RGB fp32 samples on each of 64 pixels are exactly 12 KiB.
// (16 KiB, two workgroups per CU, measured first: level on uniform 16 samples, but 1.8 x the direct kernel where 5 % of the
// pixels hold 256 samples -- a few lanes per wave in long dependent chains want waves, not LDS.  DESIGN.md 4.1j.)
constexpr int kStageWaveBytes = 12288;
static_assert(kStageWaveBytes % 1024 == 0 && (kCompactBlock / 64) * kStageWaveBytes <= 65536, "whole 1-KiB DMA groups; 64 KiB of LDS per workgroup");

__device__ __forceinline__ int compact_swizzle_piece(int piece) { return piece ^ ((piece >> 3) & 7); }

// element e of the wave's LDS image (e counts elements from the span's first piece: dwords, or halfwords of a half arena)
template <bool HALF>
__device__ __forceinline__ unsigned compact_lds_element(const unsigned *ring, int e) {
    if constexpr (HALF) return reinterpret_cast<const unsigned short *>(ring)[(compact_swizzle_piece(e >> 3) << 3) | (e & 7)];
    else return ring[(compact_swizzle_piece(e >> 2) << 2) | (e & 3)];
}

// first: the run's first element in the wave's LDS image.  Batches of four samples are read ahead of the four folds (LDS reads do
// not depend on the fold's chain); past the run's end the reads repeat its last sample and nothing is folded.
template <int C, int MAXM, bool TRANSFORM, bool HALF>
__device__ __forceinline__ void compact_fold_staged(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, int first, int cnt,
                                                    const unsigned *ring) {
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    if (cnt <= 0) return;
    PS ps;
    ps.load(t, p);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's DMA pieces have landed (and the state)
    for (int j = 0; j < cnt; j += kCompactBatch) {
        CompactRaw<C> s[kCompactBatch];
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++) {
            const int e = first + min(j + u, cnt - 1) * C;
#pragma unroll
            for (int c = 0; c < C; c++) s[u].r[c] = compact_lds_element<HALF>(ring, e + c);
        }
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++)
            if (j + u < cnt) compact_add<C, HALF>(ps, s[u]);
    }
    compact_store(ps, t, p, ctx);
}

struct StagedFold {
    template <int C, int MAXM, bool TRANSFORM, bool HALF>
    static __device__ __forceinline__ void run(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, long long start, int cnt,
                                               int split_above, bool staged, int first, const unsigned *ring) {
        if (staged) compact_fold_staged<C, MAXM, TRANSFORM, HALF>(t, ctx, p, first, cnt, ring);
        else compact_fold<C, MAXM, TRANSFORM, HALF, true>(t, ctx, p, start, cnt, split_above);
    }
};

// Workgroups and types as compact_direct_kernel has them; no lane leaves before its wave has decided.
__global__ __launch_bounds__(kCompactBlock) void compact_staged_kernel(CompactArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned ring_all[kCompactBlock / 64][kStageWaveBytes / 4];
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kCompactBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    unsigned *ring = ring_all[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
    // a lane past the film carries the empty run at the film's end: it breaks no tiling
    const long long pc = p < a.n_px ? p : a.n_px, pc1 = p + 1 < a.n_px ? p + 1 : a.n_px;
    int64_t start, end;
    compact_run(a.offsets[pc], a.offsets[pc1], a.n_samples, &start, &end);   // the clamp, first
    const int cnt = p < a.n_px ? compact_run_count(start, end) : 0;
    if (!__any(cnt > 0)) return;
    // COPIED out of the by-value argument: a reference into it keeps the whole argument in scratch
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const bool half = (a.half_mask >> ti) & 1u;
    const int elem = half ? 2 : 4;
    const long long E = (long long)t.channels * elem;      // bytes per sample
    const long long span0 = __shfl((long long)start, 0, 64), span1 = __shfl((long long)end, 63, 64);
    const long long before = __shfl_up((long long)end, 1, 64);
    const bool tiles = __all(lane == 0 || (long long)start == before);
    const uintptr_t at = reinterpret_cast<uintptr_t>(t.samples) + (uintptr_t)(span0 * E);
    const long long skew = (long long)(at & 15), bytes = skew + (span1 - span0) * E;
    const bool staged = tiles && span1 >= span0 && bytes <= kStageWaveBytes && !__any(cnt > a.split_above);
    int first = 0;
    if (staged) {
        const char *piece0 = reinterpret_cast<const char *>(at - (uintptr_t)skew);
        const int n_pieces = (int)((bytes + 15) >> 4);      // 1 .. kStageWavePieces: bytes > 0, some lane has samples
        const int n_dma = __builtin_amdgcn_readfirstlane((n_pieces + 63) >> 6);
#pragma unroll 1
        for (int k = 0; k < n_dma; k++) {
            const int src = compact_swizzle_piece(64 * k + lane);   // LDS piece 64 k + lane holds span piece src
            const char *from = piece0 + 16ll * (src < n_pieces ? src : n_pieces - 1);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(from), (__attribute__((address_space(3))) void *)(ring + 256 * k), 16, 0, 2);
        }
        first = (int)((skew + ((long long)start - span0) * E) / elem);
    }
    compact_dispatch_type<StagedFold>(t, half, ctx, p, (long long)start, cnt, a.split_above, staged, first, static_cast<const unsigned *>(ring));
}

}  // namespace

// ---------------------------------------------------------------- the host side
hipError_t launch_compact_offsets(const CompactOffsetsArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.n_chunks), block(kCompactBlock);
    hipLaunchKernelGGL(compact_block_sums_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(compact_scan_blocks_kernel, dim3(1), block, 0, s, a);
    hipLaunchKernelGGL(compact_apply_kernel, grid, block, 0, s, a);
    if (a.owners) {
        const long long blocks = (a.owners_capacity + kCompactBlock - 1) / kCompactBlock;
        hipLaunchKernelGGL(compact_owners_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), block, 0, s, a);
    }
    return hipGetLastError();
}

// force: kCompactAuto, kCompactStaged or kCompactDirect (statmc_debug_compact_path).  path (out): the kernel that ran, with
// kCompactSplitBit where the call asked for runs above split_above to be split.
constexpr int kCompactDefault = kCompactStaged;   // the A/B this rests on
hipError_t launch_compact_accumulate(const CompactArgs &a, int force, hipStream_t s, int *path) {
    const dim3 grid((unsigned)((a.n_px + kCompactBlock - 1) / kCompactBlock * a.n_types)), block(kCompactBlock);
    const bool split = a.split_above != INT32_MAX;
    const int kernel = force == kCompactAuto ? kCompactDefault : force;
    if (kernel == kCompactStaged) hipLaunchKernelGGL(compact_staged_kernel, grid, block, 0, s, a);
    else if (split) hipLaunchKernelGGL(compact_direct_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(compact_direct_kernel<false>, grid, block, 0, s, a);
    *path = kernel | (split ? kCompactSplitBit : 0);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_compact_offsets_workspace(uint16_t width, uint16_t height) { return statmc::compact_workspace_bytes(width, height); }
