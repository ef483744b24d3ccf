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
//   records   statmc_compact_accumulate_interleaved: the same arena as ONE array of interleaved records (statmc_record_layout), folded
//             in place by a general kernel (one lane per pixel and stat type) or a fused one (one lane per pixel holds every type and
//             reads each record once; direct, or with a wave's span of records staged through LDS).  Its own section below; the host
//             checks and the plan are statmc_compact_interleaved_args.h's.  DESIGN.md 4.1k.
#include "statmc_device.h"
#include "statmc_compact_args.h"
#include "statmc_scan.h"
#define STATMC_PLAN_HOST_DEVICE __host__ __device__      // records_split_chunk runs in the fold
#include "statmc_records_plan.h"
#include "statmc_compact_interleaved_args.h"
#include "statmc_record_field.h"

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

// ---------------------------------------------------------------- interleaved records: statmc_compact_accumulate_interleaved
// The arena is ONE array of records, `stride` bytes each, record i holding every type's field (statmc_record_layout; a record's
// field as it is requested and decoded: statmc_record_field.h).  Pixel p owns records [offsets[p], offsets[p + 1]), clamped by
// compact_run before anything is derived from them.  DESIGN.md 4.1k.
//
// The walk over the cnt records that start at `run`, `stride` bytes apart, in ascending position: compact_walk's batches -- four
// records in two register sets, past the last whole batch the requests repeat the run's last four records (inside the run, never
// folded) -- with the request and the fold handed in: gather(record, s) loads only, fold(s) folds.
template <class S, class G, class F>
__device__ __forceinline__ void compact_walk_records(const char *__restrict__ run, long long stride, int cnt, G gather, F fold) {
    int j = 0;
    if (cnt >= kCompactBatch) {
        const int last = cnt - kCompactBatch;
        S A[kCompactBatch], B[kCompactBatch];
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++) gather(run + u * stride, A[u]);
        // batch 0 passes through an empty asm: loaded in front of the loop AND in it, it would become one load at the loop's head
#pragma unroll
        for (int u = 0; u < kCompactBatch; u++) A[u].pin();
        // invariant: A = the records of batch j / 4 (requested)
        for (; j + 2 * kCompactBatch <= cnt; j += 2 * kCompactBatch) {
            const char *b = run + (long long)min(j + kCompactBatch, last) * stride;
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) gather(b + u * stride, B[u]);
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) fold(A[u]);
            const char *a = run + (long long)min(j + 2 * kCompactBatch, last) * stride;
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) gather(a + u * stride, A[u]);
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) fold(B[u]);
        }
        if (j + kCompactBatch <= cnt) {   // an odd number of whole batches: the last one is in A
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) fold(A[u]);
            j += kCompactBatch;
        }
    }
    for (; j < cnt; j++) {   // the last cnt % 4 records, and runs shorter than a batch
        S s;
        gather(run + (long long)j * stride, s);
        fold(s);
    }
}

// The general fold: one lane per pixel and stat type, each reading its own field through the stride.  compact_fold's two phases
// (field0 = records + the type's field offset); short_too == 0 skips phase 1: the fused kernel has served those runs.
template <int C, int MAXM, bool TRANSFORM, bool HALF, bool SPLIT>
__device__ __forceinline__ void compact_fold_records(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, const char *field0,
                                                     int stride_in, long long start, int cnt, int split_above, int short_too) {
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    using Field = RecField<C, HALF ? kFieldHalfElems : kFieldF32>;
    using S = RecRaw<Field::kRegs>;
    const long long stride = stride_in;
    auto gather = [](const char *at, S &s) __attribute__((always_inline)) { Field::load(at, s.r); };
    if (short_too && cnt > 0 && (!SPLIT || cnt <= split_above)) {
        PS ps;
        ps.load(t, p);
        compact_walk_records<S>(field0 + compact_record_byte(start, stride_in, 0), stride, cnt, gather, [&](const S &s) __attribute__((always_inline)) {
            float v[C];
            Field::decode(s.r, 0, v);
            ps.add(v);
        });
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
            compact_walk_records<S>(field0 + compact_record_byte(s0 + begin, stride_in, 0), stride, len, gather, [&](const S &s) __attribute__((always_inline)) {
                float v[C];
                Field::decode(s.r, 0, v);
                ps.add(v);
            });
            device::merge_lanes<kRecSplitLanes>(ps);
            if (lane == 0) compact_store(ps, t, p0 + from, ctx);
        }
    }
}

template <bool SPLIT>
struct RecordsFold {
    template <int C, int MAXM, bool TRANSFORM, bool HALF>
    static __device__ __forceinline__ void run(const statmc_stat_type &t, const statmc_prepass_context &ctx, long long p, const char *field0, int stride,
                                               long long start, int cnt, int split_above, int short_too) {
        compact_fold_records<C, MAXM, TRANSFORM, HALF, SPLIT>(t, ctx, p, field0, stride, start, cnt, split_above, short_too);
    }
};

// Workgroups, types and early exits as compact_direct_kernel has them.
template <bool SPLIT>
__global__ __launch_bounds__(kCompactBlock) void compact_interleaved_general_kernel(CompactInterleavedArgs a, int short_too) {
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kCompactBlock + threadIdx.x;
    if (!SPLIT && p >= a.n_px) return;
    int64_t start = 0, end = 0;
    if (!SPLIT || p < a.n_px) compact_run(a.offsets[p], a.offsets[p + 1], a.n_records, &start, &end);   // the clamp, first
    const int cnt = compact_run_count(start, end);
    if (!SPLIT && cnt <= 0) return;
    // COPIED out of the by-value argument: a reference into it keeps the whole argument in scratch
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const bool half = (a.half_mask >> ti) & 1u;
    const char *field0 = a.records + a.off[ti];
    compact_dispatch_type<RecordsFold<SPLIT>>(t, half, ctx, p, field0, a.stride, (long long)start, cnt, a.split_above, short_too);
}

// The fused fold: one lane per pixel holds the state of every type of the set (plan_records_interleaved's: the radiance type,
// K <= 2 mean-only RGB types, M <= 2 mean-only 1-channel types) and reads every field of a record once, as dwords at 4-byte
// alignment -- records_interleaved_fused_kernel's fold on a run that needs no order[].  offsets[] is read once per pixel, not once
// per pixel and type.  A run above skip_above is left alone: the general split kernel follows and serves those runs alone
// (short_too == 0), as the records entries have it -- the shipped five-type fp32 set already needs 188 VGPRs, two waves per SIMD
// (features half 171, all half 164: DESIGN.md 4.1k lists the code objects), and 64 lanes' worth of merge state on top of
// 16 + 4 K + 2 M state registers and two batches in flight would be paid by every short run.
//   not STAGED   256 lanes per workgroup, no LDS; a lane walks its run straight from global memory (compact_walk_records).
//   STAGED       one wave per workgroup with `window` bytes of LDS.  The clamped runs of the wave's 64 pixels tile ONE span of
//                records that holds every type: where they do, the span plus its skew fits the window and no run is above
//                skip_above, the wave lands the span by LDS-DMA in whole 16-byte pieces exactly as compact_staged_kernel does
//                (pieces, clamp of the last piece and source-side swizzle are its), waits once, and every lane folds its records
//                out of LDS: one staging area for all types.  Every other wave folds directly; the decision is wave-uniform.
//                A record starts at any 4-byte boundary of the image (the stride is a multiple of 4, not of 16; the skew is one
//                too), so a field is read dword by dword through the swizzle.
struct CompactFusedArgs {
    statmc_stat_type t[kRecFusedTypes];   // slot 0 the radiance type, then the K mean-only RGB types, then the M 1-channel types
    statmc_prepass_context ctx;
    const long long *offsets;
    const char *records;
    long long n_records, n_px;
    int stride;
    int off[kRecFusedTypes];
    int skip_above;       // a run of more records is left alone; INT32_MAX: never
    int window;           // STAGED: bytes of LDS, a multiple of 1024
};

template <int K, int M, int FMT, bool STAGED>
__global__ __launch_bounds__(STAGED ? 64 : kCompactBlock) void compact_interleaved_fused_kernel(CompactFusedArgs a) {
    using FRad = RecField<3, FMT == 2 ? kFieldHalfDwords : kFieldF32>;
    using FRgb = RecField<3, FMT >= 1 ? kFieldHalfDwords : kFieldF32>;
    using FOne = RecField<1, FMT >= 1 ? kFieldHalfDwords : kFieldF32>;
    constexpr int kRgb0 = FRad::kRegs, kOne0 = kRgb0 + K * FRgb::kRegs;
    using S = RecRaw<kOne0 + M * FOne::kRegs>;
    constexpr int kAlign = FMT >= 1 ? ~3 : ~0;      // where a field's load starts: half fields at the dword that holds their first element
    constexpr int kBlock = STAGED ? 64 : kCompactBlock;
    extern __shared__ __attribute__((aligned(16))) unsigned ring[];   // STAGED: the wave's window

    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    // a lane past the film carries the empty run at the film's end: it breaks no tiling
    const long long pc = p < a.n_px ? p : a.n_px, pc1 = p + 1 < a.n_px ? p + 1 : a.n_px;
    int64_t start, end;
    compact_run(a.offsets[pc], a.offsets[pc1], a.n_records, &start, &end);   // the clamp, first
    const int cnt = p < a.n_px ? compact_run_count(start, end) : 0;
    const bool mine = cnt > 0 && cnt <= a.skip_above;
    bool staged = false;
    int first = 0;                                  // STAGED: the run's first dword in the wave's LDS image
    if constexpr (STAGED) {
        if (!__any(mine)) return;
        const int lane = (int)(threadIdx.x & 63u);
        const long long stride = a.stride;
        const long long span0 = __shfl((long long)start, 0, 64), span1 = __shfl((long long)end, 63, 64);
        const long long before = __shfl_up((long long)end, 1, 64);
        const bool tiles = __all(lane == 0 || (long long)start == before);
        const uintptr_t at = reinterpret_cast<uintptr_t>(a.records) + (uintptr_t)compact_record_byte(span0, a.stride, 0);
        const long long skew = (long long)(at & 15);
        // (span1 - span0 <= window / 4 is tested first: the product below then stays far inside 64 bits)
        const bool fits = span1 >= span0 && span1 - span0 <= (long long)(a.window >> 2) && skew + (span1 - span0) * stride <= (long long)a.window;
        staged = tiles && fits && !__any(cnt > a.skip_above);
        if (staged) {
            const long long bytes = skew + (span1 - span0) * stride;
            const char *piece0 = reinterpret_cast<const char *>(at - (uintptr_t)skew);
            const int n_pieces = (int)((bytes + 15) >> 4);      // >= 1: bytes > 0, some lane has records
            const int n_dma = __builtin_amdgcn_readfirstlane((n_pieces + 63) >> 6);
#pragma unroll 1
            for (int k = 0; k < n_dma; k++) {
                const int src = compact_swizzle_piece(64 * k + lane);   // LDS piece 64 k + lane holds span piece src
                const char *from = piece0 + 16ll * (src < n_pieces ? src : n_pieces - 1);
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(from), (__attribute__((address_space(3))) void *)(ring + 256 * k), 16, 0, 2);
            }
            first = (int)((skew + ((long long)start - span0) * stride) >> 2);
        }
    }
    if (!mine) return;
    // COPIED out of the by-value argument; every index below is a constant after unrolling
    const statmc_stat_type t_rad = a.t[0];
    statmc_stat_type t_rgb[K > 0 ? K : 1], t_one[M > 0 ? M : 1];
    int rgb_off[K > 0 ? K : 1], one_off[M > 0 ? M : 1];         // where the field's load starts in a record, bytes
    int rgb_shift[K > 0 ? K : 1], one_shift[M > 0 ? M : 1];
    const int rad_off = a.off[0] & (FMT == 2 ? ~3 : ~0);
    const int rad_shift = (a.off[0] & 2) * 8;
#pragma unroll
    for (int i = 0; i < K; i++) {
        t_rgb[i] = a.t[1 + i];
        rgb_off[i] = a.off[1 + i] & kAlign;
        rgb_shift[i] = (a.off[1 + i] & 2) * 8;
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
        t_one[i] = a.t[1 + K + i];
        one_off[i] = a.off[1 + K + i] & kAlign;
        one_shift[i] = (a.off[1 + K + i] & 2) * 8;
    }
    const statmc_prepass_context ctx = a.ctx;

    device::PixelStats<3, 3, true> rad;
    device::PixelStats<3, 1, false> rgb[K > 0 ? K : 1];
    device::PixelStats<1, 1, false> one[M > 0 ? M : 1];
    rad.load(t_rad, p);
#pragma unroll
    for (int i = 0; i < K; i++) rgb[i].load(t_rgb[i], p);
#pragma unroll
    for (int i = 0; i < M; i++) one[i].load(t_one[i], p);

    auto fold = [&](const S &s) __attribute__((always_inline)) {
        float v[3];
        FRad::decode(s.r, rad_shift, v);
        rad.add(v);
#pragma unroll
        for (int i = 0; i < K; i++) {
            FRgb::decode(s.r + kRgb0 + i * FRgb::kRegs, rgb_shift[i], v);
            rgb[i].add(v);
        }
#pragma unroll
        for (int i = 0; i < M; i++) {
            FOne::decode(s.r + kOne0 + i * FOne::kRegs, one_shift[i], v);
            one[i].add(v);
        }
    };

    if (STAGED && staged) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's DMA pieces have landed (and the state)
        const int stride_dw = a.stride >> 2;
        auto lds = [&](int e) __attribute__((always_inline)) { return ring[(compact_swizzle_piece(e >> 2) << 2) | (e & 3)]; };
        // batches of four records are read ahead of the four folds (LDS reads do not depend on the fold's chain); past the run's
        // end the reads repeat its last record and nothing is folded
        for (int j = 0; j < cnt; j += kCompactBatch) {
            S s[kCompactBatch];
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++) {
                const int e = first + min(j + u, cnt - 1) * stride_dw;
#pragma unroll
                for (int r = 0; r < FRad::kRegs; r++) s[u].r[r] = lds(e + (rad_off >> 2) + r);
#pragma unroll
                for (int i = 0; i < K; i++)
#pragma unroll
                    for (int r = 0; r < FRgb::kRegs; r++) s[u].r[kRgb0 + i * FRgb::kRegs + r] = lds(e + (rgb_off[i] >> 2) + r);
#pragma unroll
                for (int i = 0; i < M; i++) s[u].r[kOne0 + i] = lds(e + (one_off[i] >> 2));
            }
#pragma unroll
            for (int u = 0; u < kCompactBatch; u++)
                if (j + u < cnt) fold(s[u]);
        }
    } else {
        compact_walk_records<S>(
            a.records + compact_record_byte(start, a.stride, 0), (long long)a.stride, cnt,
            [&](const char *at, S &s) __attribute__((always_inline)) {
                FRad::load(at + rad_off, s.r);
#pragma unroll
                for (int i = 0; i < K; i++) FRgb::load(at + rgb_off[i], s.r + kRgb0 + i * FRgb::kRegs);
#pragma unroll
                for (int i = 0; i < M; i++) FOne::load(at + one_off[i], s.r + kOne0 + i * FOne::kRegs);
            },
            fold);
    }

    compact_store(rad, t_rad, p, ctx);
#pragma unroll
    for (int i = 0; i < K; i++) rgb[i].store(t_rgb[i], p);
#pragma unroll
    for (int i = 0; i < M; i++) one[i].store(t_one[i], p);
}

template <int FMT, bool STAGED>
hipError_t launch_compact_fused(const CompactFusedArgs &f, int K, int M, hipStream_t s) {
    constexpr int kBlock = STAGED ? 64 : kCompactBlock;
    const dim3 grid((unsigned)((f.n_px + kBlock - 1) / kBlock)), block(kBlock);
    const size_t lds = STAGED ? (size_t)f.window : 0;
    switch (3 * K + M) {
    case 1: hipLaunchKernelGGL((compact_interleaved_fused_kernel<0, 1, FMT, STAGED>), grid, block, lds, s, f); break;
    case 2: hipLaunchKernelGGL((compact_interleaved_fused_kernel<0, 2, FMT, STAGED>), grid, block, lds, s, f); break;
    case 3: hipLaunchKernelGGL((compact_interleaved_fused_kernel<1, 0, FMT, STAGED>), grid, block, lds, s, f); break;
    case 4: hipLaunchKernelGGL((compact_interleaved_fused_kernel<1, 1, FMT, STAGED>), grid, block, lds, s, f); break;
    case 5: hipLaunchKernelGGL((compact_interleaved_fused_kernel<1, 2, FMT, STAGED>), grid, block, lds, s, f); break;
    case 6: hipLaunchKernelGGL((compact_interleaved_fused_kernel<2, 0, FMT, STAGED>), grid, block, lds, s, f); break;
    case 7: hipLaunchKernelGGL((compact_interleaved_fused_kernel<2, 1, FMT, STAGED>), grid, block, lds, s, f); break;
    case 8: hipLaunchKernelGGL((compact_interleaved_fused_kernel<2, 2, FMT, STAGED>), grid, block, lds, s, f); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <bool STAGED>
hipError_t launch_compact_fused(const CompactFusedArgs &f, const RecordsInterleavedPlan &plan, hipStream_t s) {
    switch (plan.fmt) {
    case 0: return launch_compact_fused<0, STAGED>(f, plan.K, plan.M, s);
    case 1: return launch_compact_fused<1, STAGED>(f, plan.K, plan.M, s);
    case 2: return launch_compact_fused<2, STAGED>(f, plan.K, plan.M, s);
    }
    return hipErrorInvalidValue;
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

// kernel: plan_compact_interleaved's answer.  window: the staged variant's LDS bytes per wave.  path (out): the kernel that ran, with
// kCompactIlvSplitBit where the call asked for runs above split_above to be split.
hipError_t launch_compact_accumulate_interleaved(const CompactInterleavedArgs &a, const RecordsInterleavedPlan &plan, int kernel, int window,
                                                 hipStream_t s, int *path) {
    const bool split = a.split_above != INT32_MAX;
    const dim3 grid((unsigned)((a.n_px + kCompactBlock - 1) / kCompactBlock * a.n_types)), block(kCompactBlock);
    int short_too = 1;
    if (kernel != kCompactIlvGeneral) {
        CompactFusedArgs f{};
        for (int j = 0; j < 1 + plan.K + plan.M; j++) {
            f.t[j] = a.t[plan.order[j]];
            f.off[j] = a.off[plan.order[j]];
        }
        f.ctx = a.ctx;
        f.offsets = a.offsets;
        f.records = a.records;
        f.n_records = a.n_records;
        f.n_px = a.n_px;
        f.stride = a.stride;
        f.skip_above = a.split_above;
        f.window = window;
        const hipError_t e = kernel == kCompactIlvFusedStaged ? launch_compact_fused<true>(f, plan, s) : launch_compact_fused<false>(f, plan, s);
        *path = kernel | (split ? kCompactIlvSplitBit : 0);
        // the fused fold has left the runs above split_above alone: the split kernel below serves them, and them alone
        if (e != hipSuccess || !split) return e;
        short_too = 0;
    }
    if (split) hipLaunchKernelGGL(compact_interleaved_general_kernel<true>, grid, block, 0, s, a, short_too);
    else hipLaunchKernelGGL(compact_interleaved_general_kernel<false>, grid, block, 0, s, a, short_too);
    *path = kernel | (split ? kCompactIlvSplitBit : 0);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_compact_offsets_workspace(uint16_t width, uint16_t height) { return statmc::compact_workspace_bytes(width, height); }
