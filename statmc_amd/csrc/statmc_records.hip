// statmc_records.hip -- statmc_accumulate_records: samples handed in as unordered (pixel, sample) records (gfx950).
//
// A wavefront path tracer, per-pixel adaptive sampling or a sparse re-render have no film-major arena and no tile with one
// count: they have a queue of finished samples.  Record i belongs to pixel pixels[i] and carries, per stat type, `channels`
// floats at samples[i * channels].  Per pixel its records are folded in ascending i, which leaves the bits statmc_accumulate
// leaves after the same samples in that order; nothing the hardware orders (atomic arrival, wave scheduling) reaches the
// fold order, so the same inputs give the same bits on every run.
//
// Two steps, after the guide's "inverted index read back in a fixed order":
//
//   grouping   order[] = the record indices sorted by pixel, STABLE (ascending i survives inside a pixel): rocPRIM's
//              radix_sort_pairs over the key bits width * height needs, keys read straight from pixels[] (a dead record --
//              any value outside [0, width * height) -- gets the key width * height and sorts behind every pixel), values a
//              counting iterator.  seg[p] = {start, end} of pixel p's run in order[] comes from the sorted keys: the record
//              whose left neighbour has another key writes start, the one whose right neighbour has another key writes
//              end -- plain stores, one writer per dword, no atomics, no scan.  seg[] is zeroed first: a pixel without
//              records reads {0, 0}.  Everything is linear in the records, whatever their distribution.
//   fold       one lane per pixel and stat type.  A lane reads seg[p] (8 B) and leaves at once where the run is empty: the
//              pixel keeps every bit of every image.  Otherwise it loads the state (statmc::device::PixelStats::load), walks
//              its run -- four record indices per load, the sample gathers of the next two batches requested before the
//              dependent chain of adds of this one, no branch in between -- and stores, with the pre-pass epilogue where
//              the type asks for it.  The arithmetic is include/statmc_device_api.hpp's: nothing is restated here.
//
// The fold of one pixel is a sequential chain by definition: a launch ends when its longest run ends, and a few pixels with
// tens of thousands of records end it on a few lanes.  statmc_accumulate_records_split (the end of this file) is the entry for
// such queues: another definition -- a long run is cut into 64 chunks, one per lane of a wave -- and a kernel of its own.

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "statmc_device.h"
#define STATMC_PLAN_HOST_DEVICE __host__ __device__      // records_split_chunk runs in records_split_fold_kernel
#include "statmc_records_plan.h"

#include "../../include/statmc_device_api.hpp"

namespace statmc {

namespace {

constexpr int kRecBlock = 256;
constexpr int kRecBatch = 4;   // records per index load; two batches are in flight behind the one being folded

// the sort key of a record: its pixel, or n_px for a dead one (sorts last, belongs to no run)
struct RecordKey {
    unsigned n_px;
    __host__ __device__ unsigned operator()(int32_t p) const { return (p >= 0 && (unsigned)p < n_px) ? (unsigned)p : n_px; }
};
using KeyIterator = rocprim::transform_iterator<const int32_t *, RecordKey, unsigned>;

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

// 4-byte aligned wide accesses: a run starts anywhere in order[], an RGB record is 12 B at a 12-B stride
typedef int rec_int4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float rec_float3 __attribute__((ext_vector_type(3), aligned(4)));

// keeps the memory instructions on either side in source order (instruction selection is free to swap independent loads); no
// instruction, no wait
__device__ __forceinline__ void rec_issue_fence() { asm volatile("" ::: "memory"); }

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
__device__ __forceinline__ void fold_pixel(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
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
    if constexpr (MAXM >= 3) {
        if (t.mean_corr != nullptr) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// Workgroup b serves stat type b % n_types and pixels [256 (b / n_types), + 256): the types of one pixel block run side by
// side and share its seg[] and order[] lines in cache.
__global__ __launch_bounds__(kRecBlock) void records_fold_kernel(RecordsArgs a) {
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kRecBlock + threadIdx.x;
    if (p >= a.n_px) return;
    const int start = a.seg[2 * p], cnt = a.seg[2 * p + 1] - start;
    if (cnt <= 0) return;
    // COPIED out of the by-value argument: a reference into it keeps the whole argument in scratch
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const int32_t *order = a.order;
    if (t.channels == 3) {
        if (t.transform) {
            if (t.max_moment >= 3) fold_pixel<3, 3, true>(t, ctx, order, p, start, cnt);
            else if (t.max_moment == 2) fold_pixel<3, 2, true>(t, ctx, order, p, start, cnt);
            else fold_pixel<3, 1, true>(t, ctx, order, p, start, cnt);
        } else {
            if (t.max_moment >= 3) fold_pixel<3, 3, false>(t, ctx, order, p, start, cnt);
            else if (t.max_moment == 2) fold_pixel<3, 2, false>(t, ctx, order, p, start, cnt);
            else fold_pixel<3, 1, false>(t, ctx, order, p, start, cnt);
        }
    } else {
        if (t.transform) {
            if (t.max_moment >= 3) fold_pixel<1, 3, true>(t, ctx, order, p, start, cnt);
            else if (t.max_moment == 2) fold_pixel<1, 2, true>(t, ctx, order, p, start, cnt);
            else fold_pixel<1, 1, true>(t, ctx, order, p, start, cnt);
        } else {
            if (t.max_moment >= 3) fold_pixel<1, 3, false>(t, ctx, order, p, start, cnt);
            else if (t.max_moment == 2) fold_pixel<1, 2, false>(t, ctx, order, p, start, cnt);
            else fold_pixel<1, 1, false>(t, ctx, order, p, start, cnt);
        }
    }
}

hipError_t sort_records(void *temp, size_t &temp_bytes, const int32_t *pixels, unsigned *keys, int32_t *order, long long n, unsigned n_px,
                        hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, KeyIterator(pixels, RecordKey{n_px}), keys, rocprim::counting_iterator<int32_t>(0), order,
                                     (unsigned)n, 0u, key_bits(n_px), s);
}

// ------------------------------------------------------------------ interleaved (array-of-structures) records
// statmc_accumulate_records_interleaved: record i is `stride` bytes at records + i * stride and holds its pixel index and every
// type's values (include/statmc.h).  The grouping is the one above -- the sort's key iterator reads record i's pixel through the
// stride, nothing is copied out first -- and leaves the same order[] and seg[].  Two folds (which one: plan_records_interleaved):
//
//   general   records_fold_kernel's shape: workgroup b serves stat type b % n_types and 256 pixels, one lane per pixel and type.
//             The lane reads its own field of the record at order[j]: a 4-byte aligned load of C floats, or a 2-byte aligned one of
//             C halves.  Every valid call.
//   fused     one lane per pixel holds the state of every type of the set (the type-fused film-major walk's sets: the radiance
//             type, K <= 2 mean-only RGB types, M <= 2 mean-only 1-channel types) and reads every field of the record once, as
//             dwords at 4-byte alignment -- a half field as the one or two dwords that hold it, taken apart in registers: a
//             record's memory line is requested by one lane instead of by one lane per type, in five workgroups.
//
// Both walk a run the way fold_pixel does (walk_run below is that walk with the gather and the fold handed in): four indices
// per load, the gathers of the next batches requested before this batch's dependent adds, clamped past the last whole batch.
// What is in flight stays RAW (the loaded dwords): a half is widened when its sample is folded, not when it is requested -- a
// conversion behind the load would wait for it there and nothing would run ahead.

// record i's key: its pixel, read in place (`pixel0` = records + pixel_offset), or n_px for a dead one
struct StridedRecordKey {
    const char *pixel0;
    long long stride;
    unsigned n_px;
    __host__ __device__ unsigned operator()(int32_t i) const {
        const int32_t p = *reinterpret_cast<const int32_t *>(pixel0 + (long long)i * stride);
        return (p >= 0 && (unsigned)p < n_px) ? (unsigned)p : n_px;
    }
};
using StridedKeyIterator = rocprim::transform_iterator<rocprim::counting_iterator<int32_t>, StridedRecordKey, unsigned>;

hipError_t sort_records_strided(void *temp, size_t &temp_bytes, const char *pixel0, long long stride, unsigned *keys, int32_t *order, long long n,
                                unsigned n_px, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, StridedKeyIterator(rocprim::counting_iterator<int32_t>(0), StridedRecordKey{pixel0, stride, n_px}),
                                     keys, rocprim::counting_iterator<int32_t>(0), order, (unsigned)n, 0u, key_bits(n_px), s);
}

typedef unsigned rec_uint3 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned rec_uint2 __attribute__((ext_vector_type(2), aligned(4)));

// the loaded dwords of one record: what a batch holds between request and fold
template <int N>
struct RecRaw {
    unsigned r[N];
    __device__ __forceinline__ void pin() {      // fold_pixel's empty asm (trap 1 of DESIGN 4.1c)
#pragma unroll
        for (int i = 0; i < N; i++) asm("" : "+v"(r[i]));
    }
};

// every finite half is an fp32 value, subnormals included: one v_cvt_f32_f16
__device__ __forceinline__ float rec_half_to_float(unsigned bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }

// One field of a record -- C elements -- as it is requested and as it is folded.
//   kFieldF32         C floats at a 4-byte aligned address: one dword, or one dwordx3
//   kFieldHalfElems   C halves at a 2-byte aligned address, element by element (the general fold)
//   kFieldHalfDwords  C halves as the dwords that hold them (the fused fold): load() is given the field's address rounded DOWN
//                     to 4 bytes, decode() the bit position of the first element in the first dword (0 or 16).  The record
//                     starts 4-byte aligned and the stride is a multiple of 4, so the dwords lie inside the record: three
//                     halves at offset o occupy [o, o + 6) and are read as [o & ~3, (o & ~3) + 8), one half as one dword.
enum { kFieldF32 = 0, kFieldHalfElems, kFieldHalfDwords };
template <int C, int F>
struct RecField {
    static constexpr int kRegs = F == kFieldHalfDwords ? (C == 3 ? 2 : 1) : C;
    static __device__ __forceinline__ void load(const char *__restrict__ at, unsigned *r) {
        if constexpr (F == kFieldHalfElems) {
            const unsigned short *h = reinterpret_cast<const unsigned short *>(at);
#pragma unroll
            for (int c = 0; c < C; c++) r[c] = h[c];
        } else if constexpr (kRegs == 3) {
            const rec_uint3 x = *reinterpret_cast<const rec_uint3 *>(at);
            r[0] = x.x;
            r[1] = x.y;
            r[2] = x.z;
        } else if constexpr (kRegs == 2) {
            const rec_uint2 x = *reinterpret_cast<const rec_uint2 *>(at);
            r[0] = x.x;
            r[1] = x.y;
        } else {
            r[0] = *reinterpret_cast<const unsigned *>(at);
        }
    }
    static __device__ __forceinline__ void decode(const unsigned *r, int shift, float *v) {
        if constexpr (F == kFieldF32) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = __uint_as_float(r[c]);
        } else if constexpr (F == kFieldHalfElems) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = rec_half_to_float(r[c]);
        } else if constexpr (C == 3) {
            const unsigned long long w = (((unsigned long long)r[1] << 32) | r[0]) >> shift;
            v[0] = rec_half_to_float((unsigned)w & 0xffffu);
            v[1] = rec_half_to_float((unsigned)(w >> 16) & 0xffffu);
            v[2] = rec_half_to_float((unsigned)(w >> 32) & 0xffffu);
        } else {
            v[0] = rec_half_to_float((r[0] >> shift) & 0xffffu);
        }
    }
};

// fold_pixel's walk over run[0 .. cnt) with the request and the fold handed in: gather(rec, s) requests record rec into s (loads
// only), fold(s) folds it.  The comments there apply word for word.
template <class S, class G, class F>
__device__ __forceinline__ void walk_run(const int32_t *__restrict__ run, int cnt, G gather, F fold) {
    int j = 0;
    if (cnt >= kRecBatch) {
        const int last = cnt - kRecBatch;
        rec_int4 idx_a = *reinterpret_cast<const rec_int4 *>(run);
        rec_int4 idx_b = *reinterpret_cast<const rec_int4 *>(run + min(kRecBatch, last));
        S A[kRecBatch], B[kRecBatch];
#pragma unroll
        for (int u = 0; u < kRecBatch; u++) gather(idx_a[u], A[u]);
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

template <int C, int MAXM, bool TRANSFORM, bool HALF>
__device__ __forceinline__ void fold_pixel_interleaved(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                                       const char *__restrict__ field0, long long stride, long long p, int start, int cnt) {
    using Field = RecField<C, HALF ? kFieldHalfElems : kFieldF32>;
    using S = RecRaw<Field::kRegs>;
    device::PixelStats<C, MAXM, TRANSFORM> ps;
    ps.load(t, p);
    walk_run<S>(
        order + start, cnt, [&](int rec, S &s) __attribute__((always_inline)) { Field::load(field0 + (long long)rec * stride, s.r); },
        [&](const S &s) __attribute__((always_inline)) {
            float v[C];
            Field::decode(s.r, 0, v);
            ps.add(v);
        });
    if constexpr (MAXM >= 3) {
        if (t.mean_corr != nullptr) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

template <int C, bool HALF>
__device__ __forceinline__ void fold_type_interleaved(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                                      const char *__restrict__ field0, long long stride, long long p, int start, int cnt) {
    if (t.transform) {
        if (t.max_moment >= 3) fold_pixel_interleaved<C, 3, true, HALF>(t, ctx, order, field0, stride, p, start, cnt);
        else if (t.max_moment == 2) fold_pixel_interleaved<C, 2, true, HALF>(t, ctx, order, field0, stride, p, start, cnt);
        else fold_pixel_interleaved<C, 1, true, HALF>(t, ctx, order, field0, stride, p, start, cnt);
    } else {
        if (t.max_moment >= 3) fold_pixel_interleaved<C, 3, false, HALF>(t, ctx, order, field0, stride, p, start, cnt);
        else if (t.max_moment == 2) fold_pixel_interleaved<C, 2, false, HALF>(t, ctx, order, field0, stride, p, start, cnt);
        else fold_pixel_interleaved<C, 1, false, HALF>(t, ctx, order, field0, stride, p, start, cnt);
    }
}

// The general fold.  Workgroup b serves stat type b % n_types and pixels [256 (b / n_types), + 256), as in records_fold_kernel.
__global__ __launch_bounds__(kRecBlock) void records_interleaved_fold_kernel(RecordsInterleavedArgs a) {
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kRecBlock + threadIdx.x;
    if (p >= a.n_px) return;
    const int start = a.seg[2 * p], cnt = a.seg[2 * p + 1] - start;
    if (cnt <= 0) return;
    // COPIED out of the by-value argument
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const int32_t *order = a.order;
    const char *field0 = a.records + a.off[ti];     // the type's field of record 0
    const long long stride = a.stride;
    const bool half = (a.half_mask >> ti) & 1u;
    if (t.channels == 3) {
        if (half) fold_type_interleaved<3, true>(t, ctx, order, field0, stride, p, start, cnt);
        else fold_type_interleaved<3, false>(t, ctx, order, field0, stride, p, start, cnt);
    } else {
        if (half) fold_type_interleaved<1, true>(t, ctx, order, field0, stride, p, start, cnt);
        else fold_type_interleaved<1, false>(t, ctx, order, field0, stride, p, start, cnt);
    }
}

// The fused fold's argument: slot 0 the radiance type, then the K mean-only RGB types, then the M mean-only 1-channel types.
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

    if (t_rad.mean_corr != nullptr) rad.store(t_rad, p, ctx);
    else rad.store(t_rad, p);
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

// ------------------------------------------------------------------ long runs over the lanes of a wave
// statmc_accumulate_records_split / statmc_accumulate_records_interleaved_split (include/statmc.h): a pixel whose run is longer
// than split_above is folded by the 64 lanes of a wave, lane j over chunk j of the run (records_split_chunk,
// statmc_records_plan.h: THE chunk rule), lane 0 from the stored state and the others from clear(); the 64 states are put
// together by statmc::device::merge_lanes<64> -- a fixed tree of PixelStats::merge -- and lane 0 stores.  Which lanes do the
// work decides no bit: the chunks and the tree are functions of the run's length alone.
//
// One kernel template serves both entries (RecSplitSrc below: where a type's field of record i lies; the per-array entry's phase 1
// is fold_pixel, records_fold_kernel's own body, and its stride a constant).  records_fold_kernel's grid: workgroup b
// serves stat type b % n_types and 256 consecutive pixels.  No lane returns early -- the wave's lanes meet again in phase 2:
//   phase 1   a lane with 0 < cnt <= split_above folds its own pixel with walk_run and stores: statmc_accumulate_records' bits.
//   phase 2   m = ballot(cnt > split_above).  For every set bit in ascending lane order -- a wave-uniform loop -- all 64 lanes
//             take that lane's (start, cnt) by __shfl (its pixel is the wave's first pixel + the lane's number), walk their
//             chunk with the same walk_run (an empty chunk issues no load; the walk's clamped requests stay inside the chunk,
//             hence inside order[]), merge, and lane 0 stores -- with the pre-pass epilogue where the type asks for it.
// No list of long pixels, no atomics, no LDS, and one launch -- except where plan_records_interleaved sends the interleaved
// entry's short pixels to the fused kernel: that kernel then leaves the runs above split_above alone (skip_above) and this one
// follows it with short_too == 0, which skips phase 1 and serves the long pixels alone.

// Where type ti's field of record i lies: field0 + i * stride, fp32 or half.
struct RecSplitSrc {
    const char *field0;
    long long stride;
    bool half;
};
__device__ __forceinline__ RecSplitSrc rec_split_src(const RecordsArgs &, const statmc_stat_type &t, int) {
    return {reinterpret_cast<const char *>(t.samples), 4ll * t.channels, false};      // record-major [n_records][channels] fp32
}
__device__ __forceinline__ RecSplitSrc rec_split_src(const RecordsInterleavedArgs &a, const statmc_stat_type &, int ti) {
    return {a.records + a.off[ti], (long long)a.stride, ((a.half_mask >> ti) & 1u) != 0};
}
template <class Args>
constexpr bool kRecSplitArrays = false;
template <>
constexpr bool kRecSplitArrays<RecordsArgs> = true;

// ARRAYS: the per-array entry -- record-major fp32 arrays, the stride 4 C a constant, and phase 1 is fold_pixel itself.
template <int C, int MAXM, bool TRANSFORM, bool HALF, bool ARRAYS>
__device__ __forceinline__ void fold_pixel_split(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                                 const char *__restrict__ field0, long long stride_in, long long p, int start, int cnt, int split_above,
                                                 int short_too) {
    static_assert(!(ARRAYS && HALF), "the per-array entry's samples are fp32");
    using Field = RecField<C, HALF ? kFieldHalfElems : kFieldF32>;
    using S = RecRaw<Field::kRegs>;
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    const long long stride = ARRAYS ? 4ll * C : stride_in;
    auto walk = [&](PS &ps, const int32_t *__restrict__ run, int len) __attribute__((always_inline)) {
        walk_run<S>(
            run, len, [&](int rec, S &s) __attribute__((always_inline)) { Field::load(field0 + (long long)rec * stride, s.r); },
            [&](const S &s) __attribute__((always_inline)) {
                float v[C];
                Field::decode(s.r, 0, v);
                ps.add(v);
            });
    };
    auto store = [&](const PS &ps, long long px) __attribute__((always_inline)) {
        if constexpr (MAXM >= 3) {
            if (t.mean_corr != nullptr) {
                ps.store(t, px, ctx);
                return;
            }
        }
        ps.store(t, px);
    };
    if (short_too && cnt > 0 && cnt <= split_above) {
        if constexpr (ARRAYS) {
            fold_pixel<C, MAXM, TRANSFORM>(t, ctx, order, p, start, cnt);       // records_fold_kernel's own body
        } else {
            PS ps;
            ps.load(t, p);
            walk(ps, order + start, cnt);
            store(ps, p);
        }
    }
    const int lane = (int)(threadIdx.x & 63u);
    const long long p0 = p - lane;                                     // the wave's first pixel: 256 consecutive pixels per workgroup
    for (unsigned long long m = __ballot(cnt > split_above); m != 0; m &= m - 1) {
        const int src = __ffsll((long long)m) - 1;
        const int s0 = __shfl(start, src, 64), c0 = __shfl(cnt, src, 64);
        int begin, len;
        records_split_chunk(c0, lane, &begin, &len);
        PS ps;
        if (lane == 0) ps.load(t, p0 + src);
        else ps.clear();
        walk(ps, order + s0 + begin, len);
        device::merge_lanes<kRecSplitLanes>(ps);
        if (lane == 0) store(ps, p0 + src);
    }
}

template <int C, bool HALF, bool ARRAYS>
__device__ __forceinline__ void fold_type_split(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                                const char *__restrict__ field0, long long stride, long long p, int start, int cnt, int split_above,
                                                int short_too) {
    if (t.transform) {
        if (t.max_moment >= 3) fold_pixel_split<C, 3, true, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
        else if (t.max_moment == 2) fold_pixel_split<C, 2, true, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
        else fold_pixel_split<C, 1, true, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
    } else {
        if (t.max_moment >= 3) fold_pixel_split<C, 3, false, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
        else if (t.max_moment == 2) fold_pixel_split<C, 2, false, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
        else fold_pixel_split<C, 1, false, HALF, ARRAYS>(t, ctx, order, field0, stride, p, start, cnt, split_above, short_too);
    }
}

// Args: RecordsArgs (the per-array entry) or RecordsInterleavedArgs.  The type dispatch is block-uniform.
template <class Args>
__global__ __launch_bounds__(kRecBlock) void records_split_fold_kernel(Args a, int split_above, int short_too) {
    static_assert(kRecSplitLanes == 64, "a split pixel's slots are the lanes of one wave");
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kRecBlock + threadIdx.x;
    int start = 0, cnt = 0;          // a lane past the film or with an empty run carries cnt = 0 and stays
    if (p < a.n_px) {
        start = a.seg[2 * p];
        cnt = a.seg[2 * p + 1] - start;
    }
    // COPIED out of the by-value argument
    const statmc_stat_type t = a.t[ti];
    const statmc_prepass_context ctx = a.ctx;
    const int32_t *order = a.order;
    const RecSplitSrc src = rec_split_src(a, t, ti);
    if constexpr (kRecSplitArrays<Args>) {
        if (t.channels == 3) fold_type_split<3, false, true>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
        else fold_type_split<1, false, true>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
    } else if (t.channels == 3) {
        if (src.half) fold_type_split<3, true, false>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
        else fold_type_split<3, false, false>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
    } else {
        if (src.half) fold_type_split<1, true, false>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
        else fold_type_split<1, false, false>(t, ctx, order, src.field0, src.stride, p, start, cnt, split_above, short_too);
    }
}

}  // namespace

hipError_t records_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w) {
    w.keys_off = 0;
    w.order_off = w.keys_off + align256((size_t)n_records * 4);
    w.seg_off = w.order_off + align256((size_t)n_records * 4);
    w.seg_bytes = (size_t)n_px * 8;
    w.temp_off = w.seg_off + align256(w.seg_bytes);
    w.temp_bytes = 0;
    // size query: no launch, nothing is dereferenced
    if (hipError_t e = sort_records(nullptr, w.temp_bytes, nullptr, nullptr, nullptr, n_records, (unsigned)n_px, nullptr); e != hipSuccess) return e;
    w.bytes = w.temp_off + align256(w.temp_bytes);
    return hipSuccess;
}

hipError_t launch_accumulate_records(const RecordsArgs &a_in, const int32_t *pixels, const RecordsWorkspace &w, char *ws, int phases,
                                     int split_above, hipStream_t s) {
    RecordsArgs a = a_in;
    unsigned *keys = reinterpret_cast<unsigned *>(ws + w.keys_off);
    int32_t *order = reinterpret_cast<int32_t *>(ws + w.order_off);
    int32_t *seg = reinterpret_cast<int32_t *>(ws + w.seg_off);
    if (phases & 1) {
        if (hipError_t e = hipMemsetAsync(seg, 0, w.seg_bytes, s); e != hipSuccess) return e;
        size_t temp_bytes = w.temp_bytes;
        if (hipError_t e = sort_records(ws + w.temp_off, temp_bytes, pixels, keys, order, a.n_records, (unsigned)a.n_px, s); e != hipSuccess) return e;
        const long long blocks = (a.n_records + kRecBlock - 1) / kRecBlock;
        hipLaunchKernelGGL(records_segments_kernel, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, keys, a.n_records, (unsigned)a.n_px, seg);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (phases & 2) {
        a.order = order;
        a.seg = seg;
        const long long blocks = (a.n_px + kRecBlock - 1) / kRecBlock * a.n_types;
        if (split_above >= 1) hipLaunchKernelGGL(records_split_fold_kernel<RecordsArgs>, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, a, split_above, 1);
        else hipLaunchKernelGGL(records_fold_kernel, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// statmc_accumulate_records' blocks at their offsets; the sort's temporary -- the last block -- is what the sort over the strided
// key iterator asks for, where that is more
hipError_t records_interleaved_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w) {
    if (hipError_t e = records_workspace_layout(n_records, n_px, w); e != hipSuccess) return e;
    size_t need = 0;
    if (hipError_t e = sort_records_strided(nullptr, need, nullptr, 4, nullptr, nullptr, n_records, (unsigned)n_px, nullptr); e != hipSuccess) return e;
    if (need > w.temp_bytes) {
        w.temp_bytes = need;
        w.bytes = w.temp_off + align256(w.temp_bytes);
    }
    return hipSuccess;
}

hipError_t launch_accumulate_records_interleaved(const RecordsInterleavedArgs &a_in, const RecordsInterleavedPlan &plan, const RecordsWorkspace &w,
                                                 char *ws, int phases, int split_above, hipStream_t s) {
    RecordsInterleavedArgs a = a_in;
    unsigned *keys = reinterpret_cast<unsigned *>(ws + w.keys_off);
    int32_t *order = reinterpret_cast<int32_t *>(ws + w.order_off);
    int32_t *seg = reinterpret_cast<int32_t *>(ws + w.seg_off);
    if (phases & 1) {
        if (hipError_t e = hipMemsetAsync(seg, 0, w.seg_bytes, s); e != hipSuccess) return e;
        size_t temp_bytes = w.temp_bytes;
        if (hipError_t e = sort_records_strided(ws + w.temp_off, temp_bytes, a.records + a.pixel_off, a.stride, keys, order, a.n_records, (unsigned)a.n_px, s);
            e != hipSuccess)
            return e;
        const long long blocks = (a.n_records + kRecBlock - 1) / kRecBlock;
        hipLaunchKernelGGL(records_segments_kernel, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, keys, a.n_records, (unsigned)a.n_px, seg);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (phases & 2) {
        const long long px_blocks = (a.n_px + kRecBlock - 1) / kRecBlock;
        if (plan.path == kRecIlvFused) {
            RecordsFusedArgs f{};
            for (int j = 0; j < 1 + plan.K + plan.M; j++) {
                f.t[j] = a.t[plan.order[j]];
                f.off[j] = a.off[plan.order[j]];
            }
            f.ctx = a.ctx;
            f.order = order;
            f.seg = seg;
            f.records = a.records;
            f.n_px = a.n_px;
            f.stride = a.stride;
            f.skip_above = split_above >= 1 ? split_above : INT32_MAX;
            hipError_t e = hipErrorInvalidValue;
            switch (plan.fmt) {
            case 0: e = launch_records_fused<0>(f, plan.K, plan.M, (unsigned)px_blocks, s); break;
            case 1: e = launch_records_fused<1>(f, plan.K, plan.M, (unsigned)px_blocks, s); break;
            case 2: e = launch_records_fused<2>(f, plan.K, plan.M, (unsigned)px_blocks, s); break;
            }
            if (e != hipSuccess || split_above < 1) return e;
            // the split entry: the fused fold has left the runs above split_above alone; one lane group per pixel and type folds them
            a.order = order;
            a.seg = seg;
            hipLaunchKernelGGL(records_split_fold_kernel<RecordsInterleavedArgs>, dim3((unsigned)(px_blocks * a.n_types)), dim3(kRecBlock), 0, s, a,
                               split_above, 0);
            return hipGetLastError();
        }
        a.order = order;
        a.seg = seg;
        if (split_above >= 1)
            hipLaunchKernelGGL(records_split_fold_kernel<RecordsInterleavedArgs>, dim3((unsigned)(px_blocks * a.n_types)), dim3(kRecBlock), 0, s, a,
                               split_above, 1);
        else hipLaunchKernelGGL(records_interleaved_fold_kernel, dim3((unsigned)(px_blocks * a.n_types)), dim3(kRecBlock), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace statmc
