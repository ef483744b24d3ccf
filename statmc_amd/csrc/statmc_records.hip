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
// tens of thousands of records end it on a few lanes.  The remedy is the caller's: deal such records to several states and
// put them together with statmc_combine_many (include/statmc.h says so too).

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "statmc_device.h"

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
                                     hipStream_t s) {
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
        hipLaunchKernelGGL(records_fold_kernel, dim3((unsigned)blocks), dim3(kRecBlock), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace statmc
