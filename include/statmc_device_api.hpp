// statmc_device_api.hpp -- StatMC's per-sample update as device code a renderer can call inside its own kernel (HIP, gfx950).
//
// statmc_accumulate reads every sample back from a film-major arena ([S][H][W][C] fp32) that the renderer wrote.  A renderer
// that holds a sample in registers right after it traced the path can instead fold it into the statistics on the spot:
//
//   statmc::device::PixelStats<C, MAXM, TRANSFORM> ps;
//   ps.load(t, pixel);                 // t: the (type, bounce)'s statmc_stat_type (samples / n_samples are ignored)
//   for (...) ps.add(sample);          // C floats per sample, in sample order
//   ps.store(t, pixel);                // moments and n; store(t, pixel, ctx) also writes mean_corr / discriminator
//
// and put the states of several slots of one pixel together before the store: ps.merge(other) where one thread holds both,
// merge_lanes<G>(ps) across the lanes of a wave and merge_waves<NW>(ps, lds) across the waves of a workgroup (all below).
// A thread that holds a partial state of a pixel it does NOT own -- another wave holds more samples of the same pixel -- must not
// store(): it writes the state as a record, ps.write_record(rec), and the host hands the (pixel, record) pairs to
// statmc_combine_records (include/statmc.h), which merges them into the film in record order.
// The result is bit for bit what statmc_accumulate leaves after the same samples (one launch or several: the state is the
// same), and store(t, pixel, ctx) writes what the accumulation's pre-pass epilogue writes.  This header is the one
// definition of that arithmetic: libstatmc_hip.so's kernels include it too.
//
// The bits do not depend on the including translation unit's floating-point flags: every function body starts with
// `#pragma clang fp contract(off)` (HIP's default -ffp-contract=fast-honor-pragmas would otherwise fuse d * (d - dN) + m2 and
// change m2), and fast-math / finite-math-only builds are refused below (the pre-pass writes inf and NaN on purpose).  A
// build that replaces the correctly rounded fp32 division (-fno-hip-fp32-correctly-rounded-divide-sqrt) changes the
// pre-pass's variance and is not supported either.
#ifndef STATMC_DEVICE_API_HPP
#define STATMC_DEVICE_API_HPP

#if defined(__FAST_MATH__) || (defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__)
#error "statmc_device_api.hpp needs IEEE fp32 semantics: compile without -ffast-math / -ffinite-math-only (the pre-pass relies on inf and NaN)"
#endif

#include <hip/hip_runtime.h>

#include "statmc.h"

namespace statmc {
namespace device {

// d / n for an integer-valued divisor n in [1, 2^24): `r` is 1/n refined from v_rcp_f32 by one
// Newton step (shared by every division by the same count: all channels, both Welford chains),
// then one residual correction of the quotient (Markstein); 3 + 3 instructions instead of ~10 per
// division.  What it returns, for finite d:
//   - the IEEE quotient wherever that quotient is a normal number or zero (tests/test_gpu_parity.py:
//     test_exact_division_by_count and _any_count sweep every count against `/`);
//   - within one step of 2^-149 of it where it is subnormal: the residual is then rounded at the
//     subnormal spacing, and 4 of 80 000 directed operands with a subnormal quotient come out one
//     step off (the first: 1.5504638832552652e-38 / 448), on the hardware as in an exact emulation
//     of the sequence (test_exact_division_directed_operands).
// d = +-inf gives NaN, not inf: the residual is fma(-inf, n, inf).  An infinite sample therefore
// leaves NaN in mean and film_mean where the reference's division leaves inf (include/statmc.h).
__device__ __forceinline__ float refined_rcp(float nf) {
#pragma clang fp contract(off)
    const float y0 = __builtin_amdgcn_rcpf(nf);
    const float e = __builtin_fmaf(-nf, y0, 1.f);
    return __builtin_fmaf(e, y0, y0);
}
__device__ __forceinline__ float div_by_count(float d, float nf, float r) {
#pragma clang fp contract(off)
    const float q0 = d * r;
    const float rem = __builtin_fmaf(-q0, nf, d);
    return __builtin_fmaf(rem, r, q0);
}

// The running state of one element (pixel x channel): Box-Cox moments and the raw-sample chain (transform types).
struct ElemState {
    float mean, m2, m3, fmean, fm2;
};

// One sample into one element; nf = the element's count INCLUDING this sample, r = refined_rcp(nf).
template <int MAXM, bool TRANSFORM>
__device__ __forceinline__ void add_sample(ElemState &st, float nf, float r, float smp) {
#pragma clang fp contract(off)
    // estimator.h:215 -- boxCox(sample, .5f) = (pow(v, .5) - 1) / .5; v_sqrt_f32 (1 ulp) stands
    // in for pow(v, .5), itself only faithfully rounded in the reference's libm.
    const float v = TRANSFORM ? (__builtin_amdgcn_sqrtf(smp) - 1.f) / .5f : smp;
    const float d = v - st.mean;
    const float dN = div_by_count(d, nf, r);
    if (MAXM >= 3) {
        const float d2 = d * d;
        const float dN2 = dN * dN;
        st.mean += dN;
        st.m2 += d * (d - dN);
        st.m3 += -3.f * dN * st.m2 + d * (d2 - dN2);
    } else if (MAXM == 2) {
        st.mean += dN;
        st.m2 += d * (d - dN);
    } else {
        st.mean += dN;
    }
    if (TRANSFORM) {  // estimator.h:217-225
        const float fd = smp - st.fmean;
        const float fdN = div_by_count(fd, nf, r);
        st.fmean += fdN;
        st.fm2 += fd * (fd - fdN);
    }
}

// ------------------------------------------------------------------ pre-pass
// t = 1 in Welch mode (the pair looks its quantile up itself); exclude: n < 2 takes the pixel out of every window
__device__ __forceinline__ void prepass_elem(int ni, float t, float mu, float s2sum, float s3sum,
                                             float &mc, float &dc, bool exclude_small_n = false) {
#pragma clang fp contract(off)
    const float nf = (float)ni;
    if (ni >= 2 && s2sum > 0.f) {
        const float var = s2sum / (nf - 1.f);
        const float mu3 = s3sum / nf;
        mc = mu + mu3 / (6.f * var * nf);
        dc = (t * t) * (var / nf);
    } else if (ni < 2 && exclude_small_n) {
        mc = __builtin_nanf("");
        dc = __builtin_nanf("");
    } else {
        mc = mu;
        dc = ni >= 2 ? 0.f : __builtin_inff();
    }
}

// The quantile the pre-pass multiplies with: the context's table (statmc_get_prepass_context) indexed by dof - 1, larger dof
// reusing the last of its 4096 entries, +inf for dof < 1 -- the lookup of the library's own pre-pass.
__device__ __forceinline__ float t_quantile(const statmc_prepass_context &ctx, int dof) {
#pragma clang fp contract(off)
    if (dof < 1) return __builtin_inff();
    if (dof > 4096) dof = 4096;
    return ctx.t_table[dof - 1];
}

// ------------------------------------------------------------------ combine
// Two independently accumulated states of one element -> the state of the union of their samples: part B (nB samples) into
// part A (nA samples).  The formulas, their exact cases and the fp32 operation order are the ones stated in include/statmc.h
// (statmc_combine_statistics); this is their one definition: statmc_combine_statistics, statmc_combine_many and
// PixelStats::merge all run it.
struct CombineCounts {
    int nA, nB;
    float fA, fB, nf, r;   // (float)nA, (float)nB, (float)(nA + nB) and its refined reciprocal
};
__device__ __forceinline__ CombineCounts combine_counts(int nA, int nB) {
#pragma clang fp contract(off)
    CombineCounts w;
    w.nA = nA;
    w.nB = nB;
    w.fA = (float)nA;
    w.fB = (float)nB;
    w.nf = (float)(nA + nB);
    w.r = refined_rcp(w.nf);
    return w;
}
// per element: nB == 0 keeps A's bits, otherwise nA == 0 takes B's, otherwise the formula
__device__ __forceinline__ float combine_pick(const CombineCounts &w, float a, float b, float f) {
    return w.nB == 0 ? a : (w.nA == 0 ? b : f);
}
// The mean (and, with M2, the m2) line of one chain -- the moments, or the raw-sample chain film_mean / film_m2.  qt = q * t
// and, with WANT_U, u = delta / n are what the m3 line needs.
template <bool M2, bool WANT_U>
__device__ __forceinline__ void combine_mean_m2(const CombineCounts &w, float mA, float mB, float m2A, float m2B, float &mean,
                                                float &m2, float &qt, float &u) {
#pragma clang fp contract(off)
    const float d = mB - mA;
    const float t = div_by_count(d * w.fB, w.nf, w.r);   // delta nB / n
    const float q = d * w.fA;                            // delta nA
    if (WANT_U) u = div_by_count(d, w.nf, w.r);          // delta / n
    qt = q * t;
    mean = combine_pick(w, mA, mB, mA + t);
    if (M2) m2 = combine_pick(w, m2A, m2B, (m2A + m2B) + qt);
}
// The m3 line: m2A / m2B are both sides' m2 from BEFORE the combine, qt and u come from combine_mean_m2<true, true>.
__device__ __forceinline__ float combine_m3(const CombineCounts &w, float m2A, float m2B, float m3A, float m3B, float qt, float u) {
#pragma clang fp contract(off)
    const float f = ((m3A + m3B) + qt * ((w.fA - w.fB) * u)) + (3.f * u) * (w.fA * m2B - w.fB * m2A);
    return combine_pick(w, m3A, m3B, f);
}
// Part B into part A for one element: the first MAXM moments and the first FILM (0..2) fields of the raw-sample chain.
template <int MAXM, int FILM>
__device__ __forceinline__ void combine_elem(ElemState &a, const ElemState &b, const CombineCounts &w) {
#pragma clang fp contract(off)
    float mean, m2 = a.m2, qt, u;
    if (MAXM >= 3) {
        combine_mean_m2<true, true>(w, a.mean, b.mean, a.m2, b.m2, mean, m2, qt, u);
        a.m3 = combine_m3(w, a.m2, b.m2, a.m3, b.m3, qt, u);
    } else if (MAXM == 2) {
        combine_mean_m2<true, false>(w, a.mean, b.mean, a.m2, b.m2, mean, m2, qt, u);
    } else {
        combine_mean_m2<false, false>(w, a.mean, b.mean, 0.f, 0.f, mean, m2, qt, u);
    }
    a.mean = mean;
    a.m2 = m2;
    if (FILM >= 2) {
        combine_mean_m2<true, false>(w, a.fmean, b.fmean, a.fm2, b.fm2, mean, m2, qt, u);
        a.fmean = mean;
        a.fm2 = m2;
    } else if (FILM == 1) {
        combine_mean_m2<false, false>(w, a.fmean, b.fmean, 0.f, 0.f, mean, m2, qt, u);
        a.fmean = mean;
    }
}

// ------------------------------------------------------------------ one pixel of one (type, bounce), one thread
// The semantics of statmc_accumulate for one pixel: load its state, fold samples in order, store.  C = channels (1 or 3),
// MAXM = max_moment (1..3), TRANSFORM = the type's Box-Cox flag -- the three fields of the statmc_stat_type, fixed at
// compile time here.  Plain scalar loads and stores: any pixel, any alignment.  One thread owns a pixel between load() and
// store(); two threads folding into the same pixel at once lose samples.  A kernel that keeps several samples of a pixel in
// flight gives every slot a PixelStats of its own (a default state: n = 0, all moments 0 -- clear()) and merges them before
// the store: a.merge(b) is statmc_combine_statistics for this pixel, bit for bit, with a as part A and b as part B.  The
// bits of a reduction depend on the order of its merges (fp32 addition is not associative): a left fold in slot order,
// s[0].merge(s[1]); s[0].merge(s[2]); ..., leaves what statmc_combine_many leaves from the same parts in that order.
template <int C, int MAXM, bool TRANSFORM>
struct PixelStats;
template <int C, int MAXM, bool TRANSFORM, class F>
__device__ __forceinline__ void map_state(PixelStats<C, MAXM, TRANSFORM> &ps, F f);   // (below: the reductions)

template <int C, int MAXM, bool TRANSFORM>
struct PixelStats {
    static_assert(C == 1 || C == 3, "a stat type has 1 or 3 channels");
    static_assert(MAXM >= 1 && MAXM <= 3, "max_moment is 1, 2 or 3");
    ElemState st[C];
    int n;

    __device__ __forceinline__ void load(const statmc_stat_type &t, long long pixel) {
#pragma clang fp contract(off)
        n = t.n[pixel];
#pragma unroll
        for (int c = 0; c < C; c++) {
            const long long e = pixel * C + c;
            st[c].mean = t.mean[e];
            st[c].m2 = MAXM >= 2 ? t.m2[e] : 0.f;
            st[c].m3 = MAXM >= 3 ? t.m3[e] : 0.f;
            st[c].fmean = TRANSFORM ? t.film_mean[e] : 0.f;
            st[c].fm2 = TRANSFORM ? t.film_m2[e] : 0.f;
        }
    }
    // the state of no samples
    __device__ __forceinline__ void clear() {
        n = 0;
#pragma unroll
        for (int c = 0; c < C; c++) st[c].mean = st[c].m2 = st[c].m3 = st[c].fmean = st[c].fm2 = 0.f;
    }
    // `other` -- the same pixel, samples of its own -- into this state: *this is part A, other part B, n becomes the sum.
    // other.n == 0 keeps this state's bits, otherwise n == 0 takes other's.  Counts must sum below 2^24.
    __device__ __forceinline__ void merge(const PixelStats &other) {
#pragma clang fp contract(off)
        const CombineCounts w = combine_counts(n, other.n);
#pragma unroll
        for (int c = 0; c < C; c++) combine_elem<MAXM, TRANSFORM ? 2 : 0>(st[c], other.st[c], w);
        n += other.n;
    }
    // one sample: sample[0 .. C)
    __device__ __forceinline__ void add(const float *sample) {
#pragma clang fp contract(off)
        n += 1;
        const float nf = (float)n;
        const float r = refined_rcp(nf);
#pragma unroll
        for (int c = 0; c < C; c++) add_sample<MAXM, TRANSFORM>(st[c], nf, r, sample[c]);
    }
    // the moments and n (Merge*Tile casts the tile's count to int32 as well, estimator.cpp:347,380)
    __device__ __forceinline__ void store(const statmc_stat_type &t, long long pixel) const {
#pragma clang fp contract(off)
#pragma unroll
        for (int c = 0; c < C; c++) {
            const long long e = pixel * C + c;
            t.mean[e] = st[c].mean;
            if (MAXM >= 2) t.m2[e] = st[c].m2;
            if (MAXM >= 3) t.m3[e] = st[c].m3;
            if (TRANSFORM) {
                t.film_mean[e] = st[c].fmean;
                t.film_m2[e] = st[c].fm2;
            }
        }
        t.n[pixel] = n;
    }
    // ... and the pre-pass of the stored moments into t.mean_corr / t.discriminator (both required; max_moment 3), under the
    // spec and significance level `ctx` was queried for: the bits of the accumulation's epilogue and of statmc_prepass.
    __device__ __forceinline__ void store(const statmc_stat_type &t, long long pixel, const statmc_prepass_context &ctx) const {
#pragma clang fp contract(off)
        static_assert(MAXM >= 3, "the pre-pass reads m2 and m3: max_moment 3");
        store(t, pixel);
        const float tq = (ctx.flags & 1) ? 1.f : t_quantile(ctx, n - 1);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const long long e = pixel * C + c;
            float m, d;
            prepass_elem(n, tq, st[c].mean, st[c].m2, st[c].m3, m, d, (ctx.flags & 2) != 0);
            t.mean_corr[e] = m;
            t.discriminator[e] = d;
        }
    }
    // The state as a record that travels (statmc_gather_states / statmc_combine_records, include/statmc.h): state_dwords<C, MAXM,
    // TRANSFORM>() dwords at rec, 4-byte aligned -- n, then per channel the fields the instantiation has, map_state's list and
    // order, every float as its bits.  A kernel whose thread holds a partial state of a pixel it does not own writes it with
    // write_record next to the pixel's index and hands both to statmc_combine_records instead of store(); read_record is the
    // inverse (fields the instantiation lacks become 0, as after load()).  Neither looks at the count: a record with n <= 0 is one
    // the library passes over.
    __device__ __forceinline__ void write_record(int32_t *rec) const {
#pragma clang fp contract(off)
        PixelStats copy = *this;
        map_state(copy, [&rec](int v) {
            *rec++ = v;
            return v;
        });
    }
    __device__ __forceinline__ void read_record(const int32_t *rec) {
#pragma clang fp contract(off)
        clear();
        map_state(*this, [&rec](int) { return *rec++; });
    }
};

// ------------------------------------------------------------------ reductions without global memory
// The states of one pixel held by several lanes of a wave (merge_lanes) or by the same lane of several waves of a workgroup
// (merge_waves), put together with PixelStats::merge -- combine_counts / combine_elem above: there is no second copy of the
// formulas.  Both run the SAME balanced tree over the slots 0 .. K - 1, the lower slot always as part A:
//
//   for stride = 1, 2, 4, ... < K:
//       for every slot j with j % (2 * stride) == 0:   slot[j].merge(slot[j + stride])      // A = slot j, B = slot j + stride
//
// and leave the result in slot 0.  That is the definition: the result is, bit for bit, K states combined by two-part
// statmc_combine_statistics calls in exactly that order (dst = part j, src = part j + stride).  It is NOT the left fold in
// slot order that statmc_combine_many computes (s[0].merge(s[1]); s[0].merge(s[2]); ...): fp32 addition is not associative,
// and for K > 2 the two orders differ in the last bits.  A slot without samples holds clear(): it keeps the other side's bits.
// Counts must sum below 2^24, as for merge.
//
// merge_lanes<G> and then merge_waves<NW> on the states the slot-0 lanes hold is one tree over NW * G slots, slot index
// w * G + j (wave w, slot j of the lane group): the lane levels are the tree's first log2(G) levels, the wave levels the rest.

// every dword of a state through f, in place -- n first, then per channel the fields the instantiation has: the one list of
// what a state is made of when it travels
template <int C, int MAXM, bool TRANSFORM, class F>
__device__ __forceinline__ void map_state(PixelStats<C, MAXM, TRANSFORM> &ps, F f) {
#pragma clang fp contract(off)
    ps.n = f(ps.n);
#pragma unroll
    for (int c = 0; c < C; c++) {
        ElemState &e = ps.st[c];
        e.mean = __int_as_float(f(__float_as_int(e.mean)));
        if (MAXM >= 2) e.m2 = __int_as_float(f(__float_as_int(e.m2)));
        if (MAXM >= 3) e.m3 = __int_as_float(f(__float_as_int(e.m3)));
        if (TRANSFORM) {
            e.fmean = __int_as_float(f(__float_as_int(e.fmean)));
            e.fm2 = __int_as_float(f(__float_as_int(e.fm2)));
        }
    }
}

// One level of merge_lanes: the state of lane (l ^ D) into this lane's.  The dwords cross the wave by __shfl_xor
// (ds_bpermute_b32) at every distance: DPP quad_perm (1, 2) and ds_swizzle (4, 8) measured level with it and
// v_permlane16_swap / v_permlane32_swap (16, 32) slower -- the merge behind each exchange is a few hundred VALU instructions,
// the exchange sixteen dwords at most.
template <int D, int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void merge_lane_level(PixelStats<C, MAXM, TRANSFORM> &ps) {
#pragma clang fp contract(off)
    PixelStats<C, MAXM, TRANSFORM> other = ps;
    map_state(other, [](int v) { return __shfl_xor(v, D, 64); });
    ps.merge(other);
}

// The lanes of a wave.  The wave's 64 lanes form 64 / G groups of G consecutive lanes; lane l is slot l % G of group l / G,
// and every slot holds a state of the group's pixel.  After the call SLOT 0 of every group holds the merged state (the tree
// above with K = G); what the other slots hold is unspecified -- do not store it.
// ALL 64 lanes of the wave execute the call, in uniform control flow: a cross-lane read from an inactive lane is undefined.  A
// lane whose pixel lies past the film does not return early: it carries a cleared state and skips only its load and store.
template <int G, int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void merge_lanes(PixelStats<C, MAXM, TRANSFORM> &ps) {
#pragma clang fp contract(off)
    static_assert(G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "G lanes per group: 2, 4, 8, 16, 32 or 64");
    if constexpr (G > 1) merge_lane_level<1>(ps);
    if constexpr (G > 2) merge_lane_level<2>(ps);
    if constexpr (G > 4) merge_lane_level<4>(ps);
    if constexpr (G > 8) merge_lane_level<8>(ps);
    if constexpr (G > 16) merge_lane_level<16>(ps);
    if constexpr (G > 32) merge_lane_level<32>(ps);
}

// The dwords of one state: n and, per channel, the fields the instantiation has.
template <int C, int MAXM, bool TRANSFORM>
constexpr int state_dwords() {
    return 1 + C * (MAXM + (TRANSFORM ? 2 : 0));
}
// The LDS scratch merge_waves<NW> needs, in bytes: one plane of 64 dwords per field and staging wave (wave 0 never stages).
template <int NW, int C, int MAXM, bool TRANSFORM>
constexpr int merge_waves_lds_bytes() {
    return state_dwords<C, MAXM, TRANSFORM>() * (NW - 1) * 64 * 4;
}

// The waves of a workgroup, through LDS.  A one-dimensional workgroup of NW waves (blockDim.x == 64 * NW): lane l of wave w
// holds slot w of item l.  After the call WAVE 0 holds the merged states (the tree above with K = NW); what the other waves
// hold is unspecified.  `scratch`: merge_waves_lds_bytes<NW, C, MAXM, TRANSFORM>() bytes of LDS, 4-byte aligned, laid out
// [field][wave - 1][lane], one dword per lane and access: consecutive lanes, consecutive banks.
// The call contains workgroup barriers: EVERY wave of the workgroup calls it, in uniform control flow, whether or not its items
// lie inside the film.  It starts with a barrier, so the scratch may come straight from another use (a previous merge_waves
// included); it does not end with one.
template <int NW, int C, int MAXM, bool TRANSFORM>
__device__ __forceinline__ void merge_waves(PixelStats<C, MAXM, TRANSFORM> &ps, float *scratch) {
#pragma clang fp contract(off)
    static_assert(NW == 2 || NW == 4 || NW == 8 || NW == 16, "NW waves per workgroup: 2, 4, 8 or 16");
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    // A wave stages into its own planes at the one level where it is part B; the waves that read at that level are part A
    // there and stage only at a later level, into other planes: one barrier per level, between the stores and the loads.
    __syncthreads();
#pragma unroll
    for (int stride = 1; stride < NW; stride *= 2) {
        if ((wave & (2 * stride - 1)) == stride) {
            int *plane = reinterpret_cast<int *>(scratch) + (wave - 1) * 64 + lane;
            map_state(ps, [&plane](int v) {
                *plane = v;
                plane += (NW - 1) * 64;
                return v;
            });
        }
        __syncthreads();
        if ((wave & (2 * stride - 1)) == 0) {
            const int *plane = reinterpret_cast<const int *>(scratch) + (wave + stride - 1) * 64 + lane;
            PixelStats<C, MAXM, TRANSFORM> other = ps;
            map_state(other, [&plane](int) {
                const int v = *plane;
                plane += (NW - 1) * 64;
                return v;
            });
            ps.merge(other);
        }
    }
}

}  // namespace device
}  // namespace statmc

#endif  // STATMC_DEVICE_API_HPP
