// statmc_records.hip -- the statmc_accumulate_records entries: samples handed in as unordered records (gfx950).
//
// A wavefront path tracer, per-pixel adaptive sampling or a sparse re-render have no film-major arena and no tile with one
// count: they have a queue of finished samples.  Record i belongs to one pixel and carries, per stat type, `channels` values.
// Per pixel its records are folded in ascending i, which leaves the bits statmc_accumulate leaves after the same samples in
// that order; nothing the hardware orders (atomic arrival, wave scheduling) reaches the fold order, so the same inputs give
// the same bits on every run.  One scheme, two SOURCES of records (include/statmc.h):
//
//   per-array     statmc_accumulate_records: record i's pixel is pixels[i], a type's values samples[i * channels], fp32.
//   interleaved   statmc_accumulate_records_interleaved: record i is `stride` bytes at records + i * stride and holds its pixel
//                 index and every type's values, fp32 or half.  Defined by the per-array entry: the bits that entry leaves for
//                 the de-interleaved arrays with half fields widened.
//
// Two steps, after the guide's "inverted index read back in a fixed order":
//
//   grouping   group_records: order[] = the record indices sorted by pixel, STABLE (ascending i survives inside a pixel):
//              rocPRIM's radix_sort_pairs over the key bits width * height needs, keys read in place through the source's key
//              iterator (a dead record -- any value outside [0, width * height) -- gets the key width * height and sorts behind
//              every pixel), values a counting iterator.  seg[p] = {start, end} of pixel p's run in order[] comes from the
//              sorted keys: the record whose left neighbour has another key writes start, the one whose right neighbour has
//              another key writes end -- plain stores, one writer per dword, no atomics, no scan.  seg[] is zeroed first: a
//              pixel without records reads {0, 0}.  Everything is linear in the records, whatever their distribution.
//   fold       records_fold_body: one lane per pixel and stat type.  A lane reads seg[p] (8 B) and leaves at once where the run
//              is empty: the pixel keeps every bit of every image.  Otherwise, through the one type dispatch, fold_one: load
//              the state (statmc::device::PixelStats::load), walk the run (walk_run), store (store_state: with the pre-pass
//              epilogue where the type asks for it).  The arithmetic is include/statmc_device_api.hpp's: nothing is restated.
//
// Two variations of the fold, each in its own section below:
//   fused      records_interleaved_fused_kernel (interleaved source, the type sets plan_records_interleaved names): one lane per
//              pixel holds the state of every type and requests every field of a record once, in the same walk_run.
//   split      statmc_accumulate_records_split / _interleaved_split (records_fold_body with SPLIT, fold_split): the fold of
//              one pixel is a sequential chain by definition, so a launch ends when its longest run ends.  Under a definition
//              of its own a run longer than split_above is cut into 64 chunks, one per lane of a wave.

#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "statmc_device.h"
#define STATMC_PLAN_HOST_DEVICE __host__ __device__      // records_split_chunk runs in records_fold_body
#include "statmc_records_plan.h"
#include "statmc_record_field.h"

#include "../../include/statmc_device_api.hpp"

namespace statmc {

namespace {

constexpr int kRecBlock = 256;
constexpr int kRecBatch = 4;   // records per index load; two batches are in flight behind the one being folded

// ------------------------------------------------------------------ grouping
// the sort key of a record: its pixel, or n_px for a dead one (sorts last, belongs to no run)
struct RecordKey {             // per-array: over pixels[]
    unsigned n_px;
    __host__ __device__ unsigned operator()(int32_t p) const { return (p >= 0 && (unsigned)p < n_px) ? (unsigned)p : n_px; }
};
using KeyIterator = rocprim::transform_iterator<const int32_t *, RecordKey, unsigned>;

struct StridedRecordKey {      // interleaved: over a counting iterator, the pixel read in place (`pixel0` = records + pixel_offset)
    const char *pixel0;
    long long stride;
    unsigned n_px;
    __host__ __device__ unsigned operator()(int32_t i) const {
        const int32_t p = *reinterpret_cast<const int32_t *>(pixel0 + (long long)i * stride);
        return (p >= 0 && (unsigned)p < n_px) ? (unsigned)p : n_px;
    }
};
using StridedKeyIterator = rocprim::transform_iterator<rocprim::counting_iterator<int32_t>, StridedRecordKey, unsigned>;

inline unsigned key_bits(unsigned n_px) {   // keys are 0 .. n_px
    unsigned b = 1;
    while (b < 32 && (n_px >> b) != 0) b++;
    return b;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// seg[k] = {start, end} for every key k < n_px that occurs in keys[0 .. n): keys is sorted, so record i starts a run iff its
// left neighbour differs and ends one iff its right neighbour does.
__global__ __launch_bounds__(kRecBlock) void records_segments_kernel(const unsigned *__restrict__ keys, long long n, unsigned n_px,
                                                                     int32_t *__restrict__ seg) {
    const long long i = (long long)blockIdx.x * kRecBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned k = keys[i];
    if (k >= n_px) return;   // dead records: the tail of the sorted array
    if (i == 0 || keys[i - 1] != k) seg[2 * (long long)k] = (int32_t)i;
    if (i + 1 == n || keys[i + 1] != k) seg[2 * (long long)k + 1] = (int32_t)(i + 1);
}

// The grouping of n records whose keys `keys_in` yields, into the workspace block ws laid out by w: seg[] zeroed, the sort,
// seg[].  ws == nullptr is the size query: temp_bytes becomes what the sort over this key iterator asks for -- no launch, nothing
// is dereferenced.
template <class Keys>
hipError_t group_records(Keys keys_in, long long n, unsigned n_px, const RecordsWorkspace &w, char *ws, size_t &temp_bytes, hipStream_t s) {
    unsigned *keys = ws ? reinterpret_cast<unsigned *>(ws + w.keys_off) : nullptr;
    int32_t *order = ws ? reinterpret_cast<int32_t *>(ws + w.order_off) : nullptr;
    int32_t *seg = ws ? reinterpret_cast<int32_t *>(ws + w.seg_off) : nullptr;
    if (ws)
        if (hipError_t e = hipMemsetAsync(seg, 0, w.seg_bytes, s); e != hipSuccess) return e;
    if (hipError_t e = rocprim::radix_sort_pairs(ws ? ws + w.temp_off : nullptr, temp_bytes, keys_in, keys, rocprim::counting_iterator<int32_t>(0), order,
                                                 (unsigned)n, 0u, key_bits(n_px), s);
        e != hipSuccess || !ws)
        return e;
    const long long blocks = (n + kRecBlock - 1) / kRecBlock;
    hipLaunchKernelGGL(records_segments_kernel, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, keys, n, n_px, seg);
    return hipGetLastError();
}

// ------------------------------------------------------------------ a record's field (statmc_record_field.h), and the walk over a run
// 4-byte aligned wide accesses: a run starts anywhere in order[]
typedef int rec_int4 __attribute__((ext_vector_type(4), aligned(4)));

// keeps the memory instructions on either side in source order (instruction selection is free to swap independent loads); no
// instruction, no wait
__device__ __forceinline__ void rec_issue_fence() { asm volatile("" ::: "memory"); }

// THE walk over run[0 .. cnt): gather(rec, s) requests record rec into s (loads only), fold(s) folds it, in ascending position.
template <class S, class G, class F>
__device__ __forceinline__ void walk_run(const int32_t *__restrict__ run, int cnt, G gather, F fold) {
    int j = 0;
    if (cnt >= kRecBatch) {
        // Batches of four, two register sets A and B.  Batch b's indices are at run[min(4 b, cnt - 4)]: past the last whole
        // batch the requests repeat the run's last four records (in bounds, never folded), so the loop body has no branch
        // between a request and the fold in front of it.  Every index load is issued BEFORE the four gathers of the batch
        // ahead of it: the wait for the indices (vmcnt counts in order) then leaves those gathers in flight.  Steady state:
        // eight gathers and an index load behind every fold.
        const int last = cnt - kRecBatch;
        rec_int4 idx_a = *reinterpret_cast<const rec_int4 *>(run);
        rec_int4 idx_b = *reinterpret_cast<const rec_int4 *>(run + min(kRecBatch, last));
        S A[kRecBatch], B[kRecBatch];
#pragma unroll
        for (int u = 0; u < kRecBatch; u++) gather(idx_a[u], A[u]);
        // Batch 0 and the second index vector pass through an empty asm: a value that is loaded in front of the loop AND in
        // it is a phi of two loads, which the optimiser turns into one load of a phi at the head of the loop -- every
        // request right in front of its own use, nothing running ahead.  The waits this costs are ones the first fold needs.
#pragma unroll
        for (int u = 0; u < kRecBatch; u++) {
            asm("" : "+v"(idx_b[u]));
            A[u].pin();
        }
        // invariant: A = the records of batch j / 4 (requested), idx_b = the indices of the batch after it
        for (; j + 2 * kRecBatch <= cnt; j += 2 * kRecBatch) {
            idx_a = *reinterpret_cast<const rec_int4 *>(run + min(j + 2 * kRecBatch, last));
            rec_issue_fence();
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) gather(idx_b[u], B[u]);
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) fold(A[u]);
            idx_b = *reinterpret_cast<const rec_int4 *>(run + min(j + 3 * kRecBatch, last));
            rec_issue_fence();
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) gather(idx_a[u], A[u]);
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) fold(B[u]);
        }
        if (j + kRecBatch <= cnt) {   // an odd number of whole batches: the last one is in A
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) fold(A[u]);
            j += kRecBatch;
        }
    }
    for (; j < cnt; j++) {   // the last cnt % 4 records, and runs shorter than a batch
        S s;
        gather(run[j], s);
        fold(s);
    }
}

// ------------------------------------------------------------------ the fold of one stat type
// A SOURCE says where stat type ti's field of record rec lies -- field0 + rec * stride --, whether it is half, and whether the
// source has halves at all (kMayBeHalf: without them no half body is instantiated).
template <class Args>
struct RecSource;
template <>
struct RecSource<RecordsArgs> {              // per-array: the type's samples, record-major [n_records][C] fp32
    static constexpr bool kMayBeHalf = false;
    static constexpr bool kArrays = true;
    static __device__ __forceinline__ const char *field0(const RecordsArgs &, const statmc_stat_type &t, int) {
        return reinterpret_cast<const char *>(t.samples);
    }
    static __device__ __forceinline__ long long stride_in(const RecordsArgs &) { return 0; }      // no run-time stride: ...
    template <int C>
    static __device__ __forceinline__ long long stride(long long) { return 4ll * C; }            // ... a constant of every body
    static __device__ __forceinline__ bool half(const RecordsArgs &, int) { return false; }
};
template <>
struct RecSource<RecordsInterleavedArgs> {   // interleaved: records + off[ti] + rec * stride, half where bit ti of half_mask is set
    static constexpr bool kMayBeHalf = true;
    static constexpr bool kArrays = false;
    static __device__ __forceinline__ const char *field0(const RecordsInterleavedArgs &a, const statmc_stat_type &, int ti) { return a.records + a.off[ti]; }
    static __device__ __forceinline__ long long stride_in(const RecordsInterleavedArgs &a) { return a.stride; }
    template <int C>
    static __device__ __forceinline__ long long stride(long long stride_in) { return stride_in; }
    static __device__ __forceinline__ bool half(const RecordsInterleavedArgs &a, int ti) { return (a.half_mask >> ti) & 1u; }
};

// walk_run's two hands for one type's field: the request of record rec, and the fold of what came into ps
template <class Field>
struct RecGather {
    const char *field0;
    long long stride;
    __device__ __forceinline__ void operator()(int rec, RecRaw<Field::kRegs> &s) const { Field::load(field0 + (long long)rec * stride, s.r); }
};
template <class Field, int C, class PS>
struct RecFold {
    PS &ps;
    __device__ __forceinline__ void operator()(const RecRaw<Field::kRegs> &s) const {
        float v[C];
        Field::decode(s.r, 0, v);
        ps.add(v);
    }
};

// THE store choice: with the pre-pass epilogue where the type asks for it (mean_corr; max_moment 3 only)
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void store_state(const device::PixelStats<C, MAXM, TRANSFORM> &ps, const statmc_stat_type &t, long long p,
                                            const statmc_prepass_context &ctx) {
    if constexpr (MAXM >= 3) {
        if (t.mean_corr != nullptr) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// THE ONE SPECIALISATION: the sequential walk of the per-array source, written out -- walk_run's loop, statement for statement,
// with the gather returning its floats by value.  walk_run over RecField<C, kFieldF32> at the constant stride compiles to
// another code object for it (records_fold_kernel 82 VGPRs and five waves per SIMD instead of 99 and four) that folds records in
// film order 1.7 % slower: 0.476 against 0.468 / 0.469 ms at 1080p, 16 records per pixel, beyond the margin of 0.003 ms (DESIGN
// 4.1c).  A change to walk_run's batching, pin, fence or clamp belongs here too.
typedef float rec_float3 __attribute__((ext_vector_type(3), aligned(4)));
template <int C>
struct RecSample {
    float v[C];
};
template <int C>
__device__ __forceinline__ RecSample<C> gather_sample(const float *__restrict__ samples, int rec) {
    RecSample<C> s;
    if constexpr (C == 3) {
        const rec_float3 x = *reinterpret_cast<const rec_float3 *>(samples + (long long)rec * 3);   // one dwordx3
        s.v[0] = x.x;
        s.v[1] = x.y;
        s.v[2] = x.z;
    } else {
        s.v[0] = samples[rec];
    }
    return s;
}
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void fold_one_arrays(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                                long long p, int start, int cnt) {
    device::PixelStats<C, MAXM, TRANSFORM> ps;
    ps.load(t, p);
    const int32_t *run = order + start;
    const float *__restrict__ samples = t.samples;
    int j = 0;
    if (cnt >= kRecBatch) {
        // Batches of four, two register sets A and B.  Batch b's indices are at run[min(4 b, cnt - 4)]: past the last whole
        // batch the requests repeat the run's last four records (in bounds, never folded), so the loop body has no branch
        // between a request and the fold in front of it.  Every index load is issued BEFORE the four gathers of the batch
        // ahead of it: the wait for the indices (vmcnt counts in order) then leaves those gathers in flight.  Steady state:
        // eight gathers and an index load behind every fold.
        const int last = cnt - kRecBatch;
        rec_int4 idx_a = *reinterpret_cast<const rec_int4 *>(run);
        rec_int4 idx_b = *reinterpret_cast<const rec_int4 *>(run + min(kRecBatch, last));
        RecSample<C> A[kRecBatch], B[kRecBatch];
#pragma unroll
        for (int u = 0; u < kRecBatch; u++) A[u] = gather_sample<C>(samples, idx_a[u]);
        // Batch 0 and the second index vector pass through an empty asm: a value that is loaded in front of the loop AND in
        // it is a phi of two loads, which the optimiser turns into one load of a phi at the head of the loop -- every
        // request right in front of its own use, nothing running ahead.  The waits this costs are ones the first fold needs.
#pragma unroll
        for (int u = 0; u < kRecBatch; u++) {
            asm("" : "+v"(idx_b[u]));
#pragma unroll
            for (int c = 0; c < C; c++) asm("" : "+v"(A[u].v[c]));
        }
        // invariant: A = the samples of batch j / 4 (requested), idx_b = the indices of the batch after it
        for (; j + 2 * kRecBatch <= cnt; j += 2 * kRecBatch) {
            idx_a = *reinterpret_cast<const rec_int4 *>(run + min(j + 2 * kRecBatch, last));
            rec_issue_fence();
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) B[u] = gather_sample<C>(samples, idx_b[u]);
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) ps.add(A[u].v);
            idx_b = *reinterpret_cast<const rec_int4 *>(run + min(j + 3 * kRecBatch, last));
            rec_issue_fence();
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) A[u] = gather_sample<C>(samples, idx_a[u]);
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) ps.add(B[u].v);
        }
        if (j + kRecBatch <= cnt) {   // an odd number of whole batches: the last one is in A
#pragma unroll
            for (int u = 0; u < kRecBatch; u++) ps.add(A[u].v);
            j += kRecBatch;
        }
    }
    for (; j < cnt; j++) {   // the last cnt % 4 records, and runs shorter than a batch
        const RecSample<C> s = gather_sample<C>(samples, run[j]);
        ps.add(s.v);
    }
    store_state(ps, t, p, ctx);
}

// THE sequential fold of one pixel: load, walk, store.  Everything arrives BY VALUE, through function arguments (no closure):
// the ranges the optimiser knows at the call (cnt > 0) reach walk_run that way.
template <class Src, int C, int MAXM, bool TRANSFORM, bool HALF>
__device__ __forceinline__ void fold_one(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                         const char *__restrict__ field0, long long stride_in, long long p, int start, int cnt) {
    if constexpr (Src::kArrays) {
        fold_one_arrays<C, MAXM, TRANSFORM>(t, ctx, order, p, start, cnt);
    } else {
        using Field = RecField<C, HALF ? kFieldHalfElems : kFieldF32>;
        using PS = device::PixelStats<C, MAXM, TRANSFORM>;
        PS ps;
        ps.load(t, p);
        walk_run<RecRaw<Field::kRegs>>(order + start, cnt, RecGather<Field>{field0, Src::template stride<C>(stride_in)}, RecFold<Field, C, PS>{ps});
        store_state(ps, t, p, ctx);
    }
}

// The split entries' fold: a pixel whose run is longer than split_above is folded by the 64 lanes of a wave, lane j over chunk j
// of the run (records_split_chunk, statmc_records_plan.h: THE chunk rule), lane 0 from the stored state and the others from
// clear(); the 64 states are put together by statmc::device::merge_lanes<64> -- a fixed tree of PixelStats::merge -- and lane 0
// stores.  Which lanes do the work decides no bit: the chunks and the tree are functions of the run's length alone.
//   phase 1   a lane with 0 < cnt <= split_above folds its own pixel with fold_one: the sequential entry's bits.
//   phase 2   m = ballot(cnt > split_above).  For every set bit in ascending lane order -- a wave-uniform loop -- all 64 lanes
//             take that lane's (start, cnt) by __shfl (its pixel is the wave's first pixel + the lane's number), walk their
//             chunk with walk_run (an empty chunk issues no load; the walk's clamped requests stay inside the chunk, hence
//             inside order[]), merge, and lane 0 stores.
// No list of long pixels, no atomics, no LDS, and one launch -- except where plan_records_interleaved sends the interleaved
// entry's short pixels to the fused kernel: that kernel then leaves the runs above split_above alone (skip_above) and this one
// follows it with short_too == 0, which skips phase 1 and serves the long pixels alone.
template <class Src, int C, int MAXM, bool TRANSFORM, bool HALF>
__device__ __forceinline__ void fold_split(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                           const char *__restrict__ field0, long long stride_in, long long p, int start, int cnt, int split_above,
                                           int short_too) {
    using Field = RecField<C, HALF ? kFieldHalfElems : kFieldF32>;
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    if (short_too && cnt > 0 && cnt <= split_above) fold_one<Src, C, MAXM, TRANSFORM, HALF>(t, ctx, order, field0, stride_in, p, start, cnt);
    const long long stride = Src::template stride<C>(stride_in);
    const int lane = (int)(threadIdx.x & 63u);
    const long long p0 = p - lane;                                     // the wave's first pixel: 256 consecutive pixels per workgroup
    for (unsigned long long m = __ballot(cnt > split_above); m != 0; m &= m - 1) {
        const int from = __ffsll((long long)m) - 1;
        const int s0 = __shfl(start, from, 64), c0 = __shfl(cnt, from, 64);
        int begin, len;
        records_split_chunk(c0, lane, &begin, &len);
        PS ps;
        if (lane == 0) ps.load(t, p0 + from);
        else ps.clear();
        walk_run<RecRaw<Field::kRegs>>(order + s0 + begin, len, RecGather<Field>{field0, stride}, RecFold<Field, C, PS>{ps});
        device::merge_lanes<kRecSplitLanes>(ps);
        if (lane == 0) store_state(ps, t, p0 + from, ctx);
    }
}

// THE type dispatch: a block-uniform stat type (and the half bit, where the source has one) to the compile-time C, MAXM,
// TRANSFORM, HALF of fold_one -- or of fold_split, where `a`, the arguments behind ctx, end in (split_above, short_too).
template <class Src, int C, int MAXM, bool TRANSFORM, bool HALF, class... A>
__device__ __forceinline__ void fold_pixel(const statmc_stat_type &t, const statmc_prepass_context &ctx, A... a) {
    if constexpr (sizeof...(A) == 6) fold_one<Src, C, MAXM, TRANSFORM, HALF>(t, ctx, a...);
    else fold_split<Src, C, MAXM, TRANSFORM, HALF>(t, ctx, a...);
}
template <class Src, int C, bool HALF, class... A>
__device__ __forceinline__ void dispatch_moments(const statmc_stat_type &t, const statmc_prepass_context &ctx, A... a) {
    if (t.transform) {
        if (t.max_moment >= 3) fold_pixel<Src, C, 3, true, HALF>(t, ctx, a...);
        else if (t.max_moment == 2) fold_pixel<Src, C, 2, true, HALF>(t, ctx, a...);
        else fold_pixel<Src, C, 1, true, HALF>(t, ctx, a...);
    } else {
        if (t.max_moment >= 3) fold_pixel<Src, C, 3, false, HALF>(t, ctx, a...);
        else if (t.max_moment == 2) fold_pixel<Src, C, 2, false, HALF>(t, ctx, a...);
        else fold_pixel<Src, C, 1, false, HALF>(t, ctx, a...);
    }
}
template <class Src, class... A>
__device__ __forceinline__ void dispatch_type(const statmc_stat_type &t, const statmc_prepass_context &ctx, bool half, A... a) {
    if (t.channels == 3) {
        if constexpr (Src::kMayBeHalf) {
            if (half) dispatch_moments<Src, 3, true>(t, ctx, a...);
            else dispatch_moments<Src, 3, false>(t, ctx, a...);
        } else {
            dispatch_moments<Src, 3, false>(t, ctx, a...);
        }
    } else {
        if constexpr (Src::kMayBeHalf) {
            if (half) dispatch_moments<Src, 1, true>(t, ctx, a...);
            else dispatch_moments<Src, 1, false>(t, ctx, a...);
        } else {
            dispatch_moments<Src, 1, false>(t, ctx, a...);
        }
    }
}

// THE kernel body, Args = RecordsArgs or RecordsInterleavedArgs.  Workgroup b serves stat type b % n_types and pixels
// [256 (b / n_types), + 256): the types of one pixel block run side by side and share its seg[] and order[] lines in cache.
// Not SPLIT: a lane past the film or with an empty run leaves.  SPLIT: no lane returns early -- the wave's lanes meet again in
// phase 2 --, such a lane carries cnt = 0 and stays.
template <bool SPLIT, class Args, class... Split>
__device__ __forceinline__ void records_fold_body(const Args &a, Split... split) {
    static_assert(kRecSplitLanes == 64, "a split pixel's slots are the lanes of one wave");
    static_assert(sizeof...(Split) == (SPLIT ? 2 : 0), "split = (split_above, short_too), for the split kernel alone");
    using Src = RecSource<Args>;
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kRecBlock + threadIdx.x;
    if (!SPLIT && p >= a.n_px) return;
    int start = 0, cnt = 0;
    if (!SPLIT || p < a.n_px) {
        start = a.seg[2 * p];
        cnt = a.seg[2 * p + 1] - start;
    }
    if (!SPLIT && cnt <= 0) return;
    // COPIED out of the by-value argument: a reference into it keeps the whole argument in scratch
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const int32_t *order = a.order;
    const char *field0 = Src::field0(a, t, ti);
    const long long stride_in = Src::stride_in(a);
    const bool half = Src::half(a, ti);
    dispatch_type<Src>(t, ctx, half, order, field0, stride_in, p, start, cnt, split...);
}

__global__ __launch_bounds__(kRecBlock) void records_fold_kernel(RecordsArgs a) { records_fold_body<false>(a); }
__global__ __launch_bounds__(kRecBlock) void records_interleaved_fold_kernel(RecordsInterleavedArgs a) { records_fold_body<false>(a); }
template <class Args>
__global__ __launch_bounds__(kRecBlock) void records_split_fold_kernel(Args a, int split_above, int short_too) {
    records_fold_body<true>(a, split_above, short_too);
}


// ------------------------------------------------------------------ the fused fold of the interleaved source
// One lane per pixel holds the state of every type of the set (the type-fused film-major walk's sets: the radiance type,
// K <= 2 mean-only RGB types, M <= 2 mean-only 1-channel types) and reads every field of the record once, as dwords at 4-byte
// alignment -- a half field as the one or two dwords that hold it, taken apart in registers: a record's memory line is requested
// by one lane instead of by one lane per type, in five workgroups.  The bits are records_interleaved_fold_kernel's.

// slot 0 the radiance type, then the K mean-only RGB types, then the M mean-only 1-channel types
struct RecordsFusedArgs {
    statmc_stat_type t[kRecFusedTypes];
    statmc_prepass_context ctx;
    const int32_t *order;
    const int32_t *seg;
    const char *records;
    long long n_px;
    int stride;
    int off[kRecFusedTypes];
    int skip_above;       // a run of more records is left alone (the split entry folds it elsewhere); INT32_MAX: never
};

// FMT as plan_records_interleaved has it: 0 every field fp32, 1 the feature fields half, 2 the radiance field too.
template <int K, int M, int FMT>
__global__ __launch_bounds__(kRecBlock) void records_interleaved_fused_kernel(RecordsFusedArgs a) {
    using FRad = RecField<3, FMT == 2 ? kFieldHalfDwords : kFieldF32>;
    using FRgb = RecField<3, FMT >= 1 ? kFieldHalfDwords : kFieldF32>;
    using FOne = RecField<1, FMT >= 1 ? kFieldHalfDwords : kFieldF32>;
    constexpr int kRgb0 = FRad::kRegs, kOne0 = kRgb0 + K * FRgb::kRegs;
    using S = RecRaw<kOne0 + M * FOne::kRegs>;
    constexpr int kAlign = FMT >= 1 ? ~3 : ~0;      // where a field's load starts: half fields at the dword that holds their first element

    const long long p = (long long)blockIdx.x * kRecBlock + threadIdx.x;
    if (p >= a.n_px) return;
    const int start = a.seg[2 * p], cnt = a.seg[2 * p + 1] - start;
    if (cnt <= 0 || cnt > a.skip_above) return;
    // COPIED out of the by-value argument; every index below is a constant after unrolling
    const statmc_stat_type t_rad = a.t[0];
    statmc_stat_type t_rgb[K > 0 ? K : 1], t_one[M > 0 ? M : 1];
    const char *rgb0[K > 0 ? K : 1], *one0[M > 0 ? M : 1];       // the field of record 0
    int rgb_shift[K > 0 ? K : 1], one_shift[M > 0 ? M : 1];
    const char *rad0 = a.records + (a.off[0] & (FMT == 2 ? ~3 : ~0));
    const int rad_shift = (a.off[0] & 2) * 8;
#pragma unroll
    for (int i = 0; i < K; i++) {
        t_rgb[i] = a.t[1 + i];
        rgb0[i] = a.records + (a.off[1 + i] & kAlign);
        rgb_shift[i] = (a.off[1 + i] & 2) * 8;
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
        t_one[i] = a.t[1 + K + i];
        one0[i] = a.records + (a.off[1 + K + i] & kAlign);
        one_shift[i] = (a.off[1 + K + i] & 2) * 8;
    }
    const statmc_prepass_context ctx = a.ctx;
    const long long stride = a.stride;

    device::PixelStats<3, 3, true> rad;
    device::PixelStats<3, 1, false> rgb[K > 0 ? K : 1];
    device::PixelStats<1, 1, false> one[M > 0 ? M : 1];
    rad.load(t_rad, p);
#pragma unroll
    for (int i = 0; i < K; i++) rgb[i].load(t_rgb[i], p);
#pragma unroll
    for (int i = 0; i < M; i++) one[i].load(t_one[i], p);

    walk_run<S>(
        a.order + start, cnt,
        [&](int rec, S &s) __attribute__((always_inline)) {
            const long long at = (long long)rec * stride;
            FRad::load(rad0 + at, s.r);
#pragma unroll
            for (int i = 0; i < K; i++) FRgb::load(rgb0[i] + at, s.r + kRgb0 + i * FRgb::kRegs);
#pragma unroll
            for (int i = 0; i < M; i++) FOne::load(one0[i] + at, s.r + kOne0 + i * FOne::kRegs);
        },
        [&](const S &s) __attribute__((always_inline)) {
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
        });

    store_state(rad, t_rad, p, ctx);
#pragma unroll
    for (int i = 0; i < K; i++) rgb[i].store(t_rgb[i], p);
#pragma unroll
    for (int i = 0; i < M; i++) one[i].store(t_one[i], p);
}

template <int FMT>
hipError_t launch_records_fused(const RecordsFusedArgs &f, int K, int M, unsigned blocks, hipStream_t s) {
    const dim3 grid(blocks), block(kRecBlock);
    switch (3 * K + M) {
    case 1: hipLaunchKernelGGL((records_interleaved_fused_kernel<0, 1, FMT>), grid, block, 0, s, f); break;
    case 2: hipLaunchKernelGGL((records_interleaved_fused_kernel<0, 2, FMT>), grid, block, 0, s, f); break;
    case 3: hipLaunchKernelGGL((records_interleaved_fused_kernel<1, 0, FMT>), grid, block, 0, s, f); break;
    case 4: hipLaunchKernelGGL((records_interleaved_fused_kernel<1, 1, FMT>), grid, block, 0, s, f); break;
    case 5: hipLaunchKernelGGL((records_interleaved_fused_kernel<1, 2, FMT>), grid, block, 0, s, f); break;
    case 6: hipLaunchKernelGGL((records_interleaved_fused_kernel<2, 0, FMT>), grid, block, 0, s, f); break;
    case 7: hipLaunchKernelGGL((records_interleaved_fused_kernel<2, 1, FMT>), grid, block, 0, s, f); break;
    case 8: hipLaunchKernelGGL((records_interleaved_fused_kernel<2, 2, FMT>), grid, block, 0, s, f); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// one lane per pixel and stat type: the split kernel where split_above >= 1, the sequential one of the source otherwise
template <class Args>
hipError_t launch_records_fold(const Args &a, int split_above, int short_too, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_px + kRecBlock - 1) / kRecBlock * a.n_types)), block(kRecBlock);
    if (split_above >= 1) hipLaunchKernelGGL(records_split_fold_kernel<Args>, grid, block, 0, s, a, split_above, short_too);
    else if constexpr (std::is_same<Args, RecordsArgs>::value) hipLaunchKernelGGL(records_fold_kernel, grid, block, 0, s, a);
    else hipLaunchKernelGGL(records_interleaved_fold_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------ the host side
hipError_t records_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w) {
    w.keys_off = 0;
    w.order_off = w.keys_off + align256((size_t)n_records * 4);
    w.seg_off = w.order_off + align256((size_t)n_records * 4);
    w.seg_bytes = (size_t)n_px * 8;
    w.temp_off = w.seg_off + align256(w.seg_bytes);
    size_t need = 0;
    if (hipError_t e = group_records(KeyIterator(nullptr, RecordKey{(unsigned)n_px}), n_records, (unsigned)n_px, w, nullptr, need, nullptr); e != hipSuccess)
        return e;
    w.temp_bytes = need;
    w.bytes = w.temp_off + align256(w.temp_bytes);
    return hipSuccess;
}

// statmc_accumulate_records' blocks at their offsets; the sort's temporary -- the last block -- is what the sort over the strided
// key iterator asks for, where that is more
hipError_t records_interleaved_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w) {
    if (hipError_t e = records_workspace_layout(n_records, n_px, w); e != hipSuccess) return e;
    size_t need = 0;
    const StridedKeyIterator keys(rocprim::counting_iterator<int32_t>(0), StridedRecordKey{nullptr, 4, (unsigned)n_px});
    if (hipError_t e = group_records(keys, n_records, (unsigned)n_px, w, nullptr, need, nullptr); e != hipSuccess) return e;
    if (need > w.temp_bytes) {
        w.temp_bytes = need;
        w.bytes = w.temp_off + align256(w.temp_bytes);
    }
    return hipSuccess;
}

// the grouping of the per-array source on its own: statmc_combine_records' records are grouped like samples (statmc_state_records.hip)
hipError_t group_records_by_pixel(const int32_t *pixels, long long n_records, long long n_px, const RecordsWorkspace &w, char *ws, hipStream_t s) {
    size_t temp_bytes = w.temp_bytes;
    return group_records(KeyIterator(pixels, RecordKey{(unsigned)n_px}), n_records, (unsigned)n_px, w, ws, temp_bytes, s);
}

hipError_t launch_accumulate_records(const RecordsArgs &a_in, const int32_t *pixels, const RecordsWorkspace &w, char *ws, int phases,
                                     int split_above, hipStream_t s) {
    RecordsArgs a = a_in;
    if (phases & 1) {
        if (hipError_t e = group_records_by_pixel(pixels, a.n_records, a.n_px, w, ws, s); e != hipSuccess) return e;
    }
    if (phases & 2) {
        a.order = reinterpret_cast<const int32_t *>(ws + w.order_off);
        a.seg = reinterpret_cast<const int32_t *>(ws + w.seg_off);
        return launch_records_fold(a, split_above, 1, s);
    }
    return hipSuccess;
}

hipError_t launch_accumulate_records_interleaved(const RecordsInterleavedArgs &a_in, const RecordsInterleavedPlan &plan, const RecordsWorkspace &w,
                                                 char *ws, int phases, int split_above, hipStream_t s) {
    RecordsInterleavedArgs a = a_in;
    if (phases & 1) {
        size_t temp_bytes = w.temp_bytes;
        const StridedKeyIterator keys(rocprim::counting_iterator<int32_t>(0), StridedRecordKey{a.records + a.pixel_off, a.stride, (unsigned)a.n_px});
        if (hipError_t e = group_records(keys, a.n_records, (unsigned)a.n_px, w, ws, temp_bytes, s); e != hipSuccess) return e;
    }
    if (phases & 2) {
        a.order = reinterpret_cast<const int32_t *>(ws + w.order_off);
        a.seg = reinterpret_cast<const int32_t *>(ws + w.seg_off);
        if (plan.path == kRecIlvFused) {
            RecordsFusedArgs f{};
            for (int j = 0; j < 1 + plan.K + plan.M; j++) {
                f.t[j] = a.t[plan.order[j]];
                f.off[j] = a.off[plan.order[j]];
            }
            f.ctx = a.ctx;
            f.order = a.order;
            f.seg = a.seg;
            f.records = a.records;
            f.n_px = a.n_px;
            f.stride = a.stride;
            f.skip_above = split_above >= 1 ? split_above : INT32_MAX;
            const unsigned px_blocks = (unsigned)((a.n_px + kRecBlock - 1) / kRecBlock);
            hipError_t e = hipErrorInvalidValue;
            switch (plan.fmt) {
            case 0: e = launch_records_fused<0>(f, plan.K, plan.M, px_blocks, s); break;
            case 1: e = launch_records_fused<1>(f, plan.K, plan.M, px_blocks, s); break;
            case 2: e = launch_records_fused<2>(f, plan.K, plan.M, px_blocks, s); break;
            }
            // the fused fold has left the runs above split_above alone: the split kernel below serves them, and them alone
            if (e != hipSuccess || split_above < 1) return e;
        }
        return launch_records_fold(a, split_above, /* short_too */ plan.path != kRecIlvFused, s);
    }
    return hipSuccess;
}

}  // namespace statmc
