// statmc_state_records.hip -- statmc_gather_states and statmc_combine_records: the state of a pixel as a thing that travels (gfx950).
//
// A state record of a stat type with C channels, max_moment M and the transform flag T is D = 1 + C (M + 2 T) dwords: the int32
// count, then per channel mean, m2, m3, film_mean, film_m2 as far as the type has them -- the order of statmc::device::map_state
// (include/statmc_device_api.hpp), which PixelStats::write_record / read_record are built on.  Record i of type t lies at
// states[t] + i * D dwords and belongs to pixel pixels[i].  Two entries that are inverses (include/statmc.h):
//
//   gather    state_gather_kernel: one thread per OUTPUT dword (record = id / D, field = id % D with D a constant of the body), so a
//             wave writes 256 consecutive bytes; the reads are scattered by nature.  A pixel outside the film gives the state of no
//             samples -- every dword 0 -- and never becomes an address.
//   combine   the grouping of statmc_accumulate_records (group_records_by_pixel, statmc_records.hip: order[] = the record indices
//             sorted by pixel, stable, seg[p] = pixel p's run in it, in the records entries' per-(device, stream) workspace), then
//             state_fold_kernel: workgroup b serves stat type b % n_types and 256 consecutive pixels, one lane per pixel.  A lane
//             loads the stored state S, walks its run in ascending record index and does S.merge(R) for every record with a
//             positive count: a chain of two-part statmc_combine_statistics steps, nothing restated (PixelStats::merge is the one
//             definition).  A record's D dwords are contiguous and come in as few loads as D allows; the next record is requested
//             before the current merge.  The pixel is stored -- with the pre-pass epilogue where the type asks -- only if some
//             record had a positive count: every other pixel keeps every bit of every image.
//   split     state_split_fold_kernel: a merge is a dependent chain with two div_by_count per moment chain, so a long run on one
//             lane is bound by latency.  A run longer than split_above is cut into 64 chunks by THE chunk rule
//             (records_split_chunk), one per lane of the wave; lane 0 starts from the stored state, the others from clear(), each
//             left-folds its chunk, and merge_lanes<64> puts the 64 states together in its fixed tree -- the relation
//             statmc_accumulate_records_split has to statmc_accumulate_records.  No LDS, no atomics, no list of long pixels.
//
// Nothing the hardware orders reaches a fold order: the same inputs give the same bits on every run.

#include "statmc_device.h"
#define STATMC_PLAN_HOST_DEVICE __host__ __device__      // records_split_chunk runs in state_fold_body
#include "statmc_state_records_args.h"

#include "../../include/statmc_device_api.hpp"

namespace statmc {

namespace {

constexpr int kStateBlock = 256;

// ------------------------------------------------------------------ one record, in registers
// 4-byte aligned wide accesses: a record starts at any dword of its array
typedef int st_int2 __attribute__((ext_vector_type(2), aligned(4)));
typedef int st_int3 __attribute__((ext_vector_type(3), aligned(4)));
typedef int st_int4 __attribute__((ext_vector_type(4), aligned(4)));

template <int D>
struct StateRaw {
    int r[D];
    // D contiguous dwords as the widest loads D allows: dwordx4 pieces, then one of x3 / x2 / x1 (loads only, no wait).  Where
    // D % 4 == 0 and the array is 16-byte aligned every piece is a naturally aligned dwordx4.
    __device__ __forceinline__ void request(const int32_t *__restrict__ rec) {
#pragma unroll
        for (int i = 0; i + 4 <= D; i += 4) {
            const st_int4 v = *reinterpret_cast<const st_int4 *>(rec + i);
            r[i] = v.x, r[i + 1] = v.y, r[i + 2] = v.z, r[i + 3] = v.w;
        }
        constexpr int at = D & ~3;
        if constexpr (D % 4 == 3) {
            const st_int3 v = *reinterpret_cast<const st_int3 *>(rec + at);
            r[at] = v.x, r[at + 1] = v.y, r[at + 2] = v.z;
        } else if constexpr (D % 4 == 2) {
            const st_int2 v = *reinterpret_cast<const st_int2 *>(rec + at);
            r[at] = v.x, r[at + 1] = v.y;
        } else if constexpr (D % 4 == 1) {
            r[at] = rec[at];
        }
    }
};

// keeps the memory instructions on either side in source order; no instruction, no wait
__device__ __forceinline__ void state_issue_fence() { asm volatile("" ::: "memory"); }

// THE walk: the records run[0 .. cnt) of the type's array `recs` into ps, in ascending position; a record whose count is not
// positive is passed over (no field of it reaches a formula).  Record j + 1 and the index of record j + 2 are requested before
// record j is merged; past the run's end the requests repeat its last record (in bounds, never merged), so there is no branch
// between a request and the merge in front of it.  Returns whether some record was merged.
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ bool walk_states(device::PixelStats<C, MAXM, TRANSFORM> &ps, const int32_t *__restrict__ recs,
                                            const int32_t *__restrict__ run, int cnt) {
    constexpr int D = device::state_dwords<C, MAXM, TRANSFORM>();
    if (cnt <= 0) return false;
    bool touched = false;
    const int last = cnt - 1;
    StateRaw<D> cur;
    cur.request(recs + (long long)run[0] * D);
    int next = run[min(1, last)];
    for (int j = 0; j < cnt; j++) {
        const int after = run[min(j + 2, last)];
        state_issue_fence();
        StateRaw<D> ahead;
        ahead.request(recs + (long long)next * D);
        state_issue_fence();
        if (cur.r[0] > 0) {
            device::PixelStats<C, MAXM, TRANSFORM> rec;
            rec.read_record(cur.r);
            ps.merge(rec);
            touched = true;
        }
        cur = ahead;
        next = after;
    }
    return touched;
}

// THE store choice: with the pre-pass epilogue where the type asks for it (mean_corr; max_moment 3 only)
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void store_combined(const device::PixelStats<C, MAXM, TRANSFORM> &ps, const statmc_stat_type &t, long long p,
                                               const statmc_prepass_context &ctx) {
    if constexpr (MAXM >= 3) {
        if (t.mean_corr != nullptr) {
            ps.store(t, p, ctx);
            return;
        }
    }
    ps.store(t, p);
}

// ------------------------------------------------------------------ the fold of one stat type
// Not SPLIT: the lane's own pixel, sequentially.  SPLIT:
//   phase 1   a lane with 0 < cnt <= split_above folds its own pixel sequentially: the bits of the launch that never splits.
//   phase 2   m = ballot(cnt > split_above).  For every set bit in ascending lane order -- a wave-uniform loop -- all 64 lanes take
//             that lane's (start, cnt) by __shfl (its pixel is the wave's first pixel + the lane's number), walk their chunk (an
//             empty chunk issues no load), merge, and lane 0 stores if any lane merged a record.
template <bool SPLIT, int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void fold_states(const statmc_stat_type &t, const statmc_prepass_context &ctx, const int32_t *__restrict__ order,
                                            long long p, int start, int cnt, int split_above) {
    using PS = device::PixelStats<C, MAXM, TRANSFORM>;
    const int32_t *recs = reinterpret_cast<const int32_t *>(t.samples);
    if (cnt > 0 && (!SPLIT || cnt <= split_above)) {
        PS ps;
        ps.load(t, p);
        if (walk_states(ps, recs, order + start, cnt)) store_combined(ps, t, p, ctx);
    }
    if constexpr (SPLIT) {
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
            const bool touched = walk_states(ps, recs, order + s0 + begin, len);
            device::merge_lanes<kRecSplitLanes>(ps);
            if (__ballot(touched) != 0 && lane == 0) store_combined(ps, t, p0 + from, ctx);
        }
    }
}

// THE type dispatch: a block-uniform stat type to the compile-time C, MAXM, TRANSFORM of a body `f`, handed over as a tag
template <int C, int MAXM, bool TRANSFORM>
struct StateKind {
    static constexpr int kC = C, kM = MAXM;
    static constexpr bool kT = TRANSFORM;
};
template <class F>
__device__ __forceinline__ void dispatch_state_type(const statmc_stat_type &t, F f) {
    if (t.channels == 3) {
        if (t.transform) {
            if (t.max_moment >= 3) f(StateKind<3, 3, true>{});
            else if (t.max_moment == 2) f(StateKind<3, 2, true>{});
            else f(StateKind<3, 1, true>{});
        } else {
            if (t.max_moment >= 3) f(StateKind<3, 3, false>{});
            else if (t.max_moment == 2) f(StateKind<3, 2, false>{});
            else f(StateKind<3, 1, false>{});
        }
    } else {
        if (t.transform) {
            if (t.max_moment >= 3) f(StateKind<1, 3, true>{});
            else if (t.max_moment == 2) f(StateKind<1, 2, true>{});
            else f(StateKind<1, 1, true>{});
        } else {
            if (t.max_moment >= 3) f(StateKind<1, 3, false>{});
            else if (t.max_moment == 2) f(StateKind<1, 2, false>{});
            else f(StateKind<1, 1, false>{});
        }
    }
}
// THE kernel body.  Workgroup b serves stat type b % n_types and pixels [256 (b / n_types), + 256): the types of one pixel block
// run side by side and share its seg[] and order[] lines in cache.  Not SPLIT: a lane past the film or with an empty run leaves.
// SPLIT: no lane returns early -- the wave's lanes meet again in phase 2 --, such a lane carries cnt = 0 and stays.
template <bool SPLIT>
__device__ __forceinline__ void state_fold_body(const StateRecordsArgs &a) {
    static_assert(kRecSplitLanes == 64, "a split pixel's slots are the lanes of one wave");
    const int ti = (int)(blockIdx.x % (unsigned)a.n_types);
    const long long p = (long long)(blockIdx.x / (unsigned)a.n_types) * kStateBlock + threadIdx.x;
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
    const int split_above = a.split_above;
    dispatch_state_type(t, [&](auto kind) __attribute__((always_inline)) {
        using K = decltype(kind);
        fold_states<SPLIT, K::kC, K::kM, K::kT>(t, ctx, order, p, start, cnt, split_above);
    });
}

__global__ __launch_bounds__(kStateBlock) void state_fold_kernel(StateRecordsArgs a) { state_fold_body<false>(a); }
__global__ __launch_bounds__(kStateBlock) void state_split_fold_kernel(StateRecordsArgs a) { state_fold_body<true>(a); }

// ------------------------------------------------------------------ the gather
// Field f of a record: 0 the count; else channel (f - 1) / F and the k-th of the F = MAXM + 2 TRANSFORM planes the type has, in
// map_state's order: mean, m2, m3 as far as MAXM reaches, then film_mean, film_m2.
// The images and the record array of one type arrive as pointers of their own: the body picks a plane by a run-time field
// number, and a descriptor held as a struct goes to scratch for that.
template <int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void gather_field(const int32_t *n, const float *mean, const float *m2, const float *m3, const float *film_mean,
                                             const float *film_m2, int32_t *__restrict__ out, const int32_t *__restrict__ pixels,
                                             long long n_records, long long n_px, long long id) {
    constexpr int D = device::state_dwords<C, MAXM, TRANSFORM>(), F = MAXM + (TRANSFORM ? 2 : 0);
    if (id >= n_records * D) return;
    const long long rec = id / D;
    const int f = (int)(id - rec * D);
    const int32_t p = pixels[rec];
    int v = 0;
    if (p >= 0 && (long long)p < n_px) {       // a dead value never becomes an address
        if (f == 0) {
            v = n[p];
        } else {
            const int c = (f - 1) / F, k = (f - 1) - c * F;
            const long long e = (long long)p * C + c;
            if (k == 0) v = __float_as_int(mean[e]);
            else if (MAXM >= 2 && k == 1) v = __float_as_int(m2[e]);
            else if (MAXM >= 3 && k == 2) v = __float_as_int(m3[e]);
            else if (TRANSFORM && k == MAXM) v = __float_as_int(film_mean[e]);
            else if (TRANSFORM) v = __float_as_int(film_m2[e]);
        }
    }
    out[id] = v;
}

// grid: (blocks over the longest type's dwords, n_types)
__global__ __launch_bounds__(kStateBlock) void state_gather_kernel(StateRecordsArgs a) {
    const int ti = (int)blockIdx.y;
    const long long id = (long long)blockIdx.x * kStateBlock + threadIdx.x;
    if (id >= a.n_records * a.dwords[ti]) return;      // block-uniform for the blocks behind a short type's end
    // every member COPIED out of the by-value argument on its own
    const int channels = a.t[ti].channels, transform = a.t[ti].transform, max_moment = a.t[ti].max_moment;
    const int32_t *n = a.t[ti].n;
    const float *mean = a.t[ti].mean, *m2 = a.t[ti].m2, *m3 = a.t[ti].m3, *film_mean = a.t[ti].film_mean, *film_m2 = a.t[ti].film_m2;
    int32_t *out = reinterpret_cast<int32_t *>(const_cast<float *>(a.t[ti].samples));
    const int32_t *pixels = a.pixels;
    const long long n_records = a.n_records, n_px = a.n_px;
#define STATMC_GATHER(c, m, t) gather_field<c, m, t>(n, mean, m2, m3, film_mean, film_m2, out, pixels, n_records, n_px, id)
    if (channels == 3) {
        if (transform) {
            if (max_moment >= 3) STATMC_GATHER(3, 3, true);
            else if (max_moment == 2) STATMC_GATHER(3, 2, true);
            else STATMC_GATHER(3, 1, true);
        } else {
            if (max_moment >= 3) STATMC_GATHER(3, 3, false);
            else if (max_moment == 2) STATMC_GATHER(3, 2, false);
            else STATMC_GATHER(3, 1, false);
        }
    } else {
        if (transform) {
            if (max_moment >= 3) STATMC_GATHER(1, 3, true);
            else if (max_moment == 2) STATMC_GATHER(1, 2, true);
            else STATMC_GATHER(1, 1, true);
        } else {
            if (max_moment >= 3) STATMC_GATHER(1, 3, false);
            else if (max_moment == 2) STATMC_GATHER(1, 2, false);
            else STATMC_GATHER(1, 1, false);
        }
    }
#undef STATMC_GATHER
}

}  // namespace

// ------------------------------------------------------------------ the host side
hipError_t launch_gather_states(const StateRecordsArgs &a, hipStream_t s) {
    int widest = 0;
    for (int i = 0; i < a.n_types; i++) widest = a.dwords[i] > widest ? a.dwords[i] : widest;
    const long long blocks = (a.n_records * widest + kStateBlock - 1) / kStateBlock;      // < 2^31 * 16 / 256 = 2^27
    if (blocks == 0 || a.n_types == 0) return hipSuccess;
    hipLaunchKernelGGL(state_gather_kernel, dim3((unsigned)blocks, (unsigned)a.n_types), dim3(kStateBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_combine_records(const StateRecordsArgs &a_in, const RecordsWorkspace &w, char *ws, hipStream_t s) {
    StateRecordsArgs a = a_in;
    if (hipError_t e = group_records_by_pixel(a.pixels, a.n_records, a.n_px, w, ws, s); e != hipSuccess) return e;
    a.order = reinterpret_cast<const int32_t *>(ws + w.order_off);
    a.seg = reinterpret_cast<const int32_t *>(ws + w.seg_off);
    const dim3 grid((unsigned)((a.n_px + kStateBlock - 1) / kStateBlock * a.n_types)), block(kStateBlock);
    if (a.split_above == INT32_MAX) hipLaunchKernelGGL(state_fold_kernel, grid, block, 0, s, a);      // no run is longer: nothing to split
    else hipLaunchKernelGGL(state_split_fold_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc

extern "C" size_t statmc_state_dwords(int channels, int max_moment, int transform) {
    return statmc::state_record_dwords(channels, max_moment, transform);
}
