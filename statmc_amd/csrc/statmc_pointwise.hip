// statmc_pointwise.hip -- the HBM-bound kernels of the statistics path (gfx950).
//
//   prepass        (n, mean, m2, m3) -> Johnson-corrected mean + discriminator
//   mean_vars      film_m2 / ((n-1) n)            (Estimator::CalculateMeanVars)
//   accumulate     sample stream -> running moments (StatTile::Add*Sample* + Merge*Tile)
//   merge_tiles    reference-layout AoS tiles -> planar images (Estimator::Merge*Tile)
//   film_update    Film::Pixel AoS -> interleaved RGB "film" image (Film::UpdateImage)
//   tile_moments   tile-local pooled moments by wavefront-level Welford/Chan merges
//
// Layout choice.  The reference images are interleaved (cv::Mat of Vec3f) and stay that way.
// Every statistic on this path is element-wise per channel, with only the sample count n shared
// by the channels of a pixel, so the kernels walk an image as a flat array of
// width*height*channels scalars and give each lane 4 consecutive PIXELS (channels x float4 per
// plane, one int4 of counts): all traffic is 16 B per lane, whatever the channel count (no
// float3 gathers), and n never crosses lanes.
//
// Arithmetic is written in the exact operation order of oracle/statmc_oracle.c and the file is
// compiled with -ffp-contract=off, so everything except sqrt-vs-pow in the Box-Cox transform
// rounds identically to the CPU restatement.

#include <type_traits>

#include "statmc_device.h"

#include "../../include/statmc_device_api.hpp"
#include "statmc_accumulate_fold.h"
#include "t_quantiles.h"

namespace statmc {

// the per-sample arithmetic and the pre-pass of one element: one definition, shared with device code outside the library
using device::CombineCounts;
using device::ElemState;
using device::add_sample;
using device::div_by_count;
using device::prepass_elem;
using device::refined_rcp;

// Sample rows in flight per lane (x2: current + next group) per kind of stat type: RGB with the Box-Cox transform, RGB,
// 1-channel.  The measured optimum (tools/experiments/build_variant.sh A/Bs source revisions).
constexpr int kAccURgbT = 3, kAccURgb = 3, kAccUF = 6;
// element pairs folded stage by stage together (RGB types: 6 pairs per lane and sample)
constexpr int kAccPairGroup = 3;
// waves per SIMD the film-major kernel is compiled for (3: 168 VGPRs, 346 spills, slower)
constexpr int kAccWaves = 2;
// RGB sample planes stream through LDS-DMA (global_load_lds_dwordx4, non-temporal): a wave's sample row is 3 KiB of
// contiguous memory, three 1-KiB transfers land it in a wave-private ring of kAccDmaD rows, every lane reads its own
// 48 B back.  tools/microbench/hbm_read_ldsdma.hip: 7.0 TB/s against 6.26 for the same walk with loads into registers
// (which for a 48-B lane stride coalesce only through the cache and must not be non-temporal); 1-channel planes keep
// their non-temporal register loads (6.8 TB/s against 6.3 - 6.6 through LDS-DMA).  Ring depth: 3 rows -- 240 VGPRs, two
// waves per SIMD; with 5 the compiler hoists all five row reads (256 VGPRs + AGPR copies), occupancy drops to one wave
// per SIMD and every type loses.
constexpr int kAccDmaD = 3;                 // sample rows in flight per wave (RGB types)
constexpr int kAccTilesDmaD = 3;            // ring depth of the tile-fed kernel
// (The state planes are written once per launch and not read again before the next one, but non-temporal stores do not
// pay: tools/microbench/acc_model.hip -- the stores are 1 % of the bytes and 9 % of the time of a one-type walk, streaming
// ones cost a quarter less there; in the kernel the radiance type alone gains 3 %, the full mix nothing.)
constexpr int acc_ring_floats(int d) { return d * 3 * 256; }                                  // per wave: D rows of 64 lanes x 12 floats
constexpr size_t acc_lds_bytes(int d) { return (size_t)4 * acc_ring_floats(d) * sizeof(float); }   // four waves per workgroup
template <int N> __device__ __forceinline__ void acc_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Student-t tables, uploaded once by statmc_setup() (hipMemcpyToSymbol).
__device__ float g_tq[STATMC_TQ_N_TABLES][STATMC_TQ_N_DOF];
// fl(t * t) of every entry: what the Welch pair test of the pair-symmetric kernel multiplies with (the oracle forms
// (t * t) * s; the product t * t rounds the same here as there).  Indexed by the degrees of freedom themselves, 0 .. 4096:
// entry 0 repeats entry 1, which is where nu < 1 and a NaN nu land (the oracle's `nu >= 1 ? ... : 1`) after the
// hardware's unsigned conversion.
__device__ float g_tq2[STATMC_TQ_N_TABLES][STATMC_TQ_N_DOF + 1];

hipError_t upload_t_table(int table, const float *host_4096) {
    if (hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_tq), host_4096, sizeof(float) * STATMC_TQ_N_DOF, sizeof(float) * STATMC_TQ_N_DOF * table); e != hipSuccess)
        return e;
    static thread_local float sq[STATMC_TQ_N_DOF + 1];
    for (int i = 0; i < STATMC_TQ_N_DOF; i++) {
        volatile float t = host_4096[i];     // one rounded product, never contracted or widened
        sq[i + 1] = t * t;
    }
    sq[0] = sq[1];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tq2), sq, sizeof(sq), sizeof(sq) * table);
}

hipError_t upload_t_tables() {
    for (int t = 0; t < STATMC_TQ_N_TABLES; t++)
        if (hipError_t e = upload_t_table(t, statmc_tq_tables[t]); e != hipSuccess) return e;
    return hipSuccess;
}
const float *t_table_sq_device_ptr(int table) {
    float *base = nullptr;
    if (hipGetSymbolAddress(reinterpret_cast<void **>(&base), HIP_SYMBOL(g_tq2)) != hipSuccess) return nullptr;
    return base + (size_t)table * (STATMC_TQ_N_DOF + 1);
}
const float *t_table_device_ptr(int table) {
    float *base = nullptr;
    if (hipGetSymbolAddress(reinterpret_cast<void **>(&base), HIP_SYMBOL(g_tq)) != hipSuccess) return nullptr;
    return base + (size_t)table * STATMC_TQ_N_DOF;
}

// table = alpha_index + 3 * sides (t_quantiles.h)
__device__ __forceinline__ float t_quantile(int table, int dof) {
    if (dof < 1) return __builtin_inff();
    if (dof > STATMC_TQ_N_DOF) dof = STATMC_TQ_N_DOF;
    return g_tq[table][dof - 1];
}
// the quantile the pre-pass epilogues hand prepass_elem for a pixel of n samples (flags: AccumulateType::pre_flags)
__device__ __forceinline__ float prepass_quantile(int table, int flags, int n) { return (flags & 1) ? 1.f : t_quantile(table, n - 1); }

constexpr int kBlock = 256;

static inline int grid_for(long long work_items, int cap = 256 * 16) {
    long long b = (work_items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// ------------------------------------------------------------------ pre-pass
// (prepass_elem: include/statmc_device_api.hpp)
template <bool VEC4>
__global__ __launch_bounds__(kBlock) void prepass_kernel(PrepassArgs a) {
    const long long n_groups = (a.n_elems + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n_groups;
         g += (long long)gridDim.x * kBlock) {
        const long long e0 = g << 2;
        if (VEC4 && e0 + 4 <= a.n_elems) {
            const float4 mu = *reinterpret_cast<const float4 *>(a.mean + e0);
            const float4 s2 = *reinterpret_cast<const float4 *>(a.m2 + e0);
            const float4 s3 = *reinterpret_cast<const float4 *>(a.m3 + e0);
            float4 mc, dc;
            const float *pmu = &mu.x, *ps2 = &s2.x, *ps3 = &s3.x;
            float *pmc = &mc.x, *pdc = &dc.x;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ni = a.n[(e0 + j) / a.channels];
                prepass_elem(ni, a.welch ? 1.f : t_quantile(a.table, ni - 1), pmu[j], ps2[j], ps3[j], pmc[j], pdc[j], a.small_n_exclude);
            }
            *reinterpret_cast<float4 *>(a.mean_corr + e0) = mc;
            *reinterpret_cast<float4 *>(a.disc + e0) = dc;
        } else {
            for (long long e = e0; e < a.n_elems && e < e0 + 4; e++) {
                const int ni = a.n[e / a.channels];
                float mc, dc;
                prepass_elem(ni, a.welch ? 1.f : t_quantile(a.table, ni - 1), a.mean[e], a.m2[e], a.m3[e], mc, dc, a.small_n_exclude);
                a.mean_corr[e] = mc;
                a.disc[e] = dc;
            }
        }
    }
}

hipError_t launch_prepass(const PrepassArgs &a, hipStream_t s) {
    const bool vec = aligned16(a.mean) && aligned16(a.m2) && aligned16(a.m3) && aligned16(a.mean_corr) &&
                     aligned16(a.disc);
    const int grid = grid_for((a.n_elems + 3) / 4);
    if (vec)
        hipLaunchKernelGGL(prepass_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL(prepass_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ pre-pass + pack
// The multi-GPU block path needs the five filter inputs of the owned block as one 15-channel block +
// halo image (statmc_filter.hip: pack_inputs_kernel).  Doing the pre-pass in the same pass saves the
// round trip of mean_corr / disc through HBM (184 -> 136 B per pixel, or 160 with the two by-products
// still written out) and a launch.  Same prepass_elem, same bits.
struct f3p {
    float x, y, z;
};
__global__ __launch_bounds__(kBlock) void prepass_pack_kernel(PrepassPackArgs a) {
    const long long n_px = (long long)a.src_w * a.src_h;
    for (long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x; i0 < n_px; i0 += (long long)gridDim.x * kBlock) {
        const int y0 = (int)(i0 / a.src_w), x = (int)(i0 - (long long)y0 * a.src_w);
        const int y = y0 + (y0 >= a.split_row ? a.skip_rows : 0);   // the second of two row ranges
        const long long i = (long long)y * a.src_w + x;
        const int ni = a.n[i];
        const float t = a.welch ? 1.f : t_quantile(a.table, ni - 1);
        const f3p mu = reinterpret_cast<const f3p *>(a.mean)[i], s2 = reinterpret_cast<const f3p *>(a.m2)[i],
                  s3 = reinterpret_cast<const f3p *>(a.m3)[i];
        f3p mc, dc;
        prepass_elem(ni, t, mu.x, s2.x, s3.x, mc.x, dc.x, a.small_n_exclude);
        prepass_elem(ni, t, mu.y, s2.y, s3.y, mc.y, dc.y, a.small_n_exclude);
        prepass_elem(ni, t, mu.z, s2.z, s3.z, mc.z, dc.z, a.small_n_exclude);
        if (a.mean_corr) reinterpret_cast<f3p *>(a.mean_corr)[i] = mc;
        if (a.disc) reinterpret_cast<f3p *>(a.disc)[i] = dc;
        float *px = a.packed + ((long long)(y + a.dst_y0) * a.dst_w + (x + a.dst_x0)) * a.ch;
        f3p *dst = reinterpret_cast<f3p *>(px);
        const f3p zero = {0.f, 0.f, 0.f};
        dst[0] = mc;
        dst[1] = dc;
        dst[2] = reinterpret_cast<const f3p *>(a.colour)[i];
        dst[3] = a.g0 ? reinterpret_cast<const f3p *>(a.g0)[i] : zero;
        dst[4] = a.g1 ? reinterpret_cast<const f3p *>(a.g1)[i] : zero;
        if (a.ch >= 17) {
            px[15] = a.s0 ? a.s0[i] : 0.f;
            px[16] = a.s1 ? a.s1[i] : 0.f;
            if (a.ch == 18) px[17] = __int_as_float(ni);
        } else if (a.ch == 16) {
            px[15] = __int_as_float(ni);
        }
    }
}

hipError_t launch_prepass_pack(const PrepassPackArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(prepass_pack_kernel, dim3(grid_for((long long)a.src_w * a.src_h)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ mean vars
__global__ __launch_bounds__(kBlock) void mean_vars_kernel(MeanVarsArgs a) {
    const long long n_elems = (long long)a.width * a.height * a.channels;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < n_elems;
         e += (long long)gridDim.x * kBlock) {
        const long long px = e / a.channels;
        const long long npx = a.row_n_quirk ? (px / a.width) * a.width : px;  // estimator.cpp:540,558
        const float nf = (float)a.n[npx];
        a.film_var[e] = a.film_m2[e] / ((nf - 1.f) * nf);
    }
}

hipError_t launch_mean_vars(const MeanVarsArgs &a, hipStream_t s) {
    const long long n_elems = (long long)a.width * a.height * a.channels;
    hipLaunchKernelGGL(mean_vars_kernel, dim3(grid_for(n_elems)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ accumulate
// One lane owns 4 consecutive PIXELS of one stat type (4*C consecutive scalar elements = C
// float4 per image plane, one int4 of counts) and walks the batch's samples in order (sample s
// of pixel p, channel c is at samples[s*n_elems + p*C + c]), so the update sequence per element
// is the reference's (estimator.h:162-226).  Owning whole pixels keeps the count n private to
// the lane (no cross-lane read/write race on n).  blockIdx.y selects the stat type.
// (ElemState, refined_rcp, div_by_count, add_sample: include/statmc_device_api.hpp, the definition a renderer's own kernel
// includes as well)

// (PairState, add_sample2 -- the same update on two elements at once --, load_plane, store_plane, store_counts: statmc_accumulate_fold.h,
// shared with statmc_counted.hip)
// Optional epilogue (round 6): the pre-pass of the moments just written, from the registers that hold them -- the same
// prepass_elem as prepass_kernel, hence the same bits -- instead of a launch that reads 40 B per pixel back.  NC as above: one
// count, one quantile.  (The caller reads pre_mc, pre_dc, table and flags out of its descriptor BEFORE its first store: see
// accumulate_lane.)
template <int C, int NC>
__device__ __forceinline__ void store_prepass(float *pre_mc, float *pre_dc, const PairState *st, const int (&n_out)[NC], int table, int flags) {
    float tq[NC];
#pragma unroll
    for (int p = 0; p < NC; p++) tq[p] = prepass_quantile(table, flags, n_out[p]);
#pragma unroll
    for (int k = 0; k < C; k++) {
        vfloat4 mc, dc;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = 4 * k + j, px = NC > 1 ? e / C : 0;
            float m, d;
            prepass_elem(n_out[px], tq[px], st[e >> 1].mean[e & 1], st[e >> 1].m2[e & 1], st[e >> 1].m3[e & 1], m, d, (flags & 2) != 0);
            mc[j] = m;
            dc[j] = d;
        }
        *reinterpret_cast<vfloat4 *>(pre_mc + 4 * k) = mc;
        *reinterpret_cast<vfloat4 *>(pre_dc + 4 * k) = dc;
    }
}

// The LDS-DMA ring of a wave, its protocol written once: D sample rows in flight, every row T transfers that `issue(s, slot)`
// requests; row s has landed when at most T (D - 1) transfers issued after it are outstanding (VMEM operations of a wave complete
// in order; nothing else touches memory inside the walk).  `take_and_fold(s, slot, refill)` reads the lane's piece of the slot,
// waits for those LDS reads (a slot is refilled once every lane has read its piece), calls refill() and folds sample s.
// primed: the caller has requested the first D rows already (acc_ring_prime, ahead of its state loads).
template <int D, typename Issue>
__device__ __forceinline__ void acc_ring_prime(int S, Issue issue) {
#pragma unroll
    for (int d = 0; d < D; d++)
        if (d < S) issue(d, d);
}
template <int D, int T, typename Issue, typename TakeFold>
__device__ __forceinline__ void acc_ring_walk(int S, bool primed, Issue issue, TakeFold take_and_fold) {
    static_assert(T * (D - 1) <= 63, "the counted wait must fit vmcnt");
    // every earlier access of the wave to memory (the state loads; a primed ring's first D rows, requested ahead of them) has
    // completed before the counted waits start
    acc_wait_vmcnt<0>();
    if (!primed) acc_ring_prime<D>(S, issue);
    const int S_full = S >= D ? S - D + 1 : 0;          // samples s < S_full have D - 1 later rows in flight behind them
    // One row per trip, the slot a run-time index (round 5): unrolled by D with compile-time slots the compiler hoisted the
    // LDS reads of all D rows to the top of the body -- D x 12 registers, which is what capped the ring at three rows
    // (240 VGPRs; 5 rows: 256 + AGPR copies, one wave per SIMD).  The body is ~200 instructions; the loop costs nothing.
    int slot = 0;
#pragma unroll 1
    for (int s = 0; s < S; s++) {
        if (s < S_full) acc_wait_vmcnt<T * (D - 1)>(); else acc_wait_vmcnt<0>();   // the last D - 1 rows: nothing is issued behind them
        take_and_fold(s, slot, [&] { if (s + D < S) issue(s + D, slot); });
        slot = slot + 1 == D ? 0 : slot + 1;
    }
}
// Every lane issues all three transfers of an RGB row, whatever part of the row exists: the waits of the walk COUNT transfers
// (vmcnt), so their number per row must not depend on n_active.  A piece beyond the row's end re-reads the row's first 16 bytes
// (memory that exists) into a part of the slot nobody reads.  Piece k of lane `lane`, in floats from the row's start:
__device__ __forceinline__ int acc_row_piece(int k, int lane, int n_active) { return 256 * k + 4 * lane < 12 * n_active ? 256 * k + 4 * lane : 0; }

// The lane's 4 consecutive pixels starting at film pixel p0 (16-B aligned planes): load the
// state, fold S samples in order, store.  Sample s of the lane's elements is at sp + s * stride
// (4*C consecutive floats): stride = n_elems for sample-major film planes, = tile pixels * C for
// the tile-major arena of accumulate_tiles.
// UMUL: prefetch depth multiplier (tile-fed path, types whose state is small enough to afford the registers)
// DMA (C == 3 only): the sample rows arrive by LDS-DMA in the wave's ring.  That walk is COOPERATIVE -- the 16-byte piece a
// lane fetches belongs to another lane's pixels -- so the whole wave calls in: lane l owns the 4-pixel group at
// sp_wave + 12 l floats, `active` says whether that group exists, `n_active` (wave-uniform) how many lanes' groups do
// (they are the first n_active lanes).  Without DMA an inactive lane returns at once.
// ST: what the arena holds -- float, or _Float16 (statmc_accumulate_formats): the lane's piece of a half row is 8 C bytes at
// 8-byte alignment, widened with one v_cvt_f32_f16 per element on its way into the same q[C] (every finite half is an fp32
// value, subnormals included: the fold sees what it would see had the caller widened the arena).  Register loads, or (DMA, C == 3: the
// tile walk) the ring below.
typedef _Float16 vhalf4 __attribute__((ext_vector_type(4)));
template <int C, int MAXM, bool TRANSFORM, int UMUL = 1, int DMA = 0, typename ST = float>
__device__ __forceinline__ void accumulate_lane(const AccumulateType &t, long long p0_in, const ST *sp,
                                                long long stride, int S, float *ring = nullptr, bool active = true, int n_active = 64,
                                                bool dma_first = false) {
    constexpr bool kDma = DMA > 0 && C == 3;
    constexpr bool kHalf = !std::is_same<ST, float>::value;
    constexpr int kD = DMA > 0 ? DMA : 1;               // ring depth: sample rows in flight
    if constexpr (!kDma) {
        if (!active) return;
    }
    const long long p0 = active ? p0_in : 0;   // an inactive lane of the cooperative walk touches no state: its loads read group 0, it stores nothing
    // LDS-DMA walk: the geometry of the wave's sample rows.  (dma_first: the first D rows requested BEFORE the state loads, so
    // that the two latencies a wave pays before its first fold overlap instead of adding up -- measured in round 4 at 4 .. 256
    // samples per pixel, 720p / 1080p / 4K: within +- 0.5 % of requesting them behind the state, profiles/r04_acc_launch.log;
    // kept as a switch of the A/B hook, off.)
    // Half RGB rows (the tile walk): a row is 24 bytes per lane, 1536 for a full wave, so a 3-KiB slot holds the rows of TWO
    // consecutive samples s = 2 p and s + 1 and the ring's unit is the pair p: [0, 1024) the head of row s, [1024, 2048) the head of
    // row s + 1, [2048, 2560) the 512-byte tail of row s fetched by lanes 0 - 31 and [2560, 3072) the tail of row s + 1 fetched by
    // lanes 32 - 63 of ONE transfer (the source address is per lane, the destination base + 16 bytes per lane).  Three transfers
    // per pair, issued by every lane; the protocol is acc_ring_walk's, over pairs.  An odd last sample has no partner: the
    // partner's addresses name row s again.  The caller guarantees 16-byte aligned rows and an even n_active, so a row is a
    // whole number of 16-byte pieces and a piece beyond its end is clamped to the row's first one (acc_row_piece's rule).
    [[maybe_unused]] int dma_piece[3] = {0, 0, 0};                 // fp32: floats; half: bytes -- [0] the head piece, [1] the tail piece
    [[maybe_unused]] const float *dma_row0 = nullptr;
    [[maybe_unused]] const char *dma_row0_half = nullptr;
    [[maybe_unused]] const int dma_units = kHalf ? (S + 1) >> 1 : S;     // what the ring walks: sample pairs, or samples
    auto dma_issue = [&](int s, int slot) {
        float *dst = ring + slot * 768;
        if constexpr (kHalf) {
            const char *r0 = dma_row0_half + (long long)(2 * s) * stride * 2;
            const char *r1 = 2 * s + 1 < S ? r0 + stride * 2 : r0;
            const char *tail = (threadIdx.x & 32) ? r1 : r0;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(r0 + dma_piece[0]), (__attribute__((address_space(3))) void *)(dst), 16, 0, 2);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(r1 + dma_piece[0]), (__attribute__((address_space(3))) void *)(dst + 256), 16, 0, 2);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(tail + dma_piece[1]), (__attribute__((address_space(3))) void *)(dst + 512), 16, 0, 2);
        } else {
            const float *src = dma_row0 + (long long)s * stride;
#pragma unroll
            for (int k = 0; k < 3; k++)
                __builtin_amdgcn_global_load_lds(src + dma_piece[k], (__attribute__((address_space(3))) void *)(dst + 256 * k), 16, 0, 2);
        }
    };
    if constexpr (kDma) {
        const int lane = threadIdx.x & 63;
        if constexpr (kHalf) {
            dma_row0_half = reinterpret_cast<const char *>(sp) - 24 * lane;                  // the wave's row of sample 0, as below
            const int row_bytes = 24 * n_active, head = 16 * lane, tail = 1024 + 16 * (lane & 31);
            dma_piece[0] = head < row_bytes ? head : 0;
            dma_piece[1] = tail < row_bytes ? tail : 0;
        } else {
            dma_row0 = reinterpret_cast<const float *>(sp) - 12 * lane;                      // the wave's row of sample 0 (lane l sits 12 l floats in; the same value in every lane)
#pragma unroll
            for (int k = 0; k < 3; k++) dma_piece[k] = acc_row_piece(k, lane, n_active);
        }
        if (dma_first) acc_ring_prime<kD>(dma_units, dma_issue);
    }
    constexpr int NE = 4 * C;  // elements per lane
    const long long e0 = p0 * C;
    // (the epilogue's descriptor fields, read BEFORE the first store: read behind the stores they keep the by-value kernel argument
    // in a private copy -- 2 KB of scratch per lane and 17 more VGPRs, accumulation 3.67 -> 4.60 ms; measured, round 6)
    float *const pre_mc = MAXM >= 3 ? t.mean_corr : nullptr;
    float *const pre_dc = MAXM >= 3 ? t.disc : nullptr;
    const int pre_table = t.pre_table, pre_flags = t.pre_flags;
    PairState st[NE / 2];   // element pairs (2 i, 2 i + 1) of the lane's 4 C consecutive elements
    const int4 n4 = *reinterpret_cast<const int4 *>(t.n + p0);
    const int n0[4] = {n4.x, n4.y, n4.z, n4.w};
    load_plane<C>(st, &PairState::mean, t.mean + e0);
    load_plane<C, MAXM >= 2>(st, &PairState::m2, t.m2 + e0);
    load_plane<C, MAXM >= 3>(st, &PairState::m3, t.m3 + e0);
    load_plane<C, TRANSFORM>(st, &PairState::fmean, t.film_mean + e0);
    load_plane<C, TRANSFORM>(st, &PairState::fm2, t.film_m2 + e0);
    // Software-pipelined sample walk: the loads of the next U samples are issued before
    // the current U are folded into the moments, so 2U sample rows per lane are in flight
    // (the compiler would otherwise drain each unrolled body before loading again).
    // C = 3: the three 16-B loads of a lane interleave across the wave (48-B lane stride);
    // they only coalesce through the cache, so they must be plain loads (non-temporal ones
    // re-fetch the shared lines: 4.8 vs 6.4 TB/s, tools/microbench/hbm_read.hip).  C = 1
    // streams with non-temporal loads.
    constexpr int U = UMUL * (C == 3 ? (TRANSFORM ? kAccURgbT : kAccURgb) : kAccUF);
    auto load_sample = [&](vfloat4 (&dst)[C], const ST *src) {
        if constexpr (kHalf) {
            vhalf4 h[C];
#pragma unroll
            for (int k = 0; k < C; k++)
                h[k] = C == 1 ? __builtin_nontemporal_load(reinterpret_cast<const vhalf4 *>(src + 4 * k))
                              : *reinterpret_cast<const vhalf4 *>(src + 4 * k);
#pragma unroll
            for (int k = 0; k < C; k++) dst[k] = __builtin_convertvector(h[k], vfloat4);
        } else {
#pragma unroll
            for (int k = 0; k < C; k++)
                dst[k] = C == 1 ? __builtin_nontemporal_load(reinterpret_cast<const vfloat4 *>(src + 4 * k))
                                : *reinterpret_cast<const vfloat4 *>(src + 4 * k);
        }
    };
    // SAME: the lane's 4 pixels hold the same count (every film whose pixels have seen the
    // same number of samples, i.e. all but adaptively sampled ones) -> one count conversion and
    // one refined reciprocal per sample instead of four (a fifth of the kernel's VALU work).
    auto fold_sample = [&](const vfloat4 (&q)[C], int s, auto same) {
        if constexpr (decltype(same)::value) {
            const float nf0 = (float)(n0[0] + s + 1);
            const float rc0 = refined_rcp(nf0);
            v2f nf2[NE / 2], rc2[NE / 2], smp2[NE / 2];
#pragma unroll
            for (int i = 0; i < NE / 2; i++) {   // elements 2 i and 2 i + 1
                nf2[i] = v2f{nf0, nf0};
                rc2[i] = v2f{rc0, rc0};
                smp2[i] = v2f{q[i >> 1][2 * (i & 1)], q[i >> 1][2 * (i & 1) + 1]};
            }
            constexpr int G = C == 3 ? kAccPairGroup : 2;
#pragma unroll
            for (int g = 0; g < NE / 2; g += G) add_sample2<G, MAXM, TRANSFORM>(st + g, nf2 + g, rc2 + g, smp2 + g);
        } else {
            // ragged counts (adaptively sampled films): element by element, one reciprocal per pixel
            float nf[4], rc[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                nf[p] = (float)(n0[p] + s + 1);
                rc[p] = refined_rcp(nf[p]);
            }
#pragma unroll
            for (int j = 0; j < NE; j++) {
                ElemState e = {st[j >> 1].mean[j & 1], st[j >> 1].m2[j & 1], st[j >> 1].m3[j & 1], st[j >> 1].fmean[j & 1], st[j >> 1].fm2[j & 1]};
                add_sample<MAXM, TRANSFORM>(e, nf[j / C], rc[j / C], q[j >> 2][j & 3]);
                st[j >> 1].mean[j & 1] = e.mean;
                if (MAXM >= 2) st[j >> 1].m2[j & 1] = e.m2;
                if (MAXM >= 3) st[j >> 1].m3[j & 1] = e.m3;
                if (TRANSFORM) { st[j >> 1].fmean[j & 1] = e.fmean; st[j >> 1].fm2[j & 1] = e.fm2; }
            }
        }
    };
    auto walk_samples = [&](auto same) {
        vfloat4 cur[U][C], nxt[U][C];
        const int S_main = S - S % U;
        if (S_main > 0) {
#pragma unroll
            for (int u = 0; u < U; u++) load_sample(cur[u], sp + (long long)u * stride);
        }
        for (int s = 0; s < S_main; s += U) {
            const ST *np = sp + (long long)(s + U) * stride;
            if (s + U < S_main) {
#pragma unroll
                for (int u = 0; u < U; u++) load_sample(nxt[u], np + (long long)u * stride);
            }
#pragma unroll
            for (int u = 0; u < U; u++) fold_sample(cur[u], s + u, same);
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < C; k++) cur[u][k] = nxt[u][k];
        }
        for (int s = S_main; s < S; s++) {  // remainder (S not a multiple of U)
            vfloat4 q[C];
            load_sample(q, sp + (long long)s * stride);
            fold_sample(q, s, same);
        }
    };
    // The same walk with the sample rows arriving by LDS-DMA (C == 3): kD rows in flight in the wave's ring, three transfers each
    // (acc_ring_walk); every lane reads its own 48 B back.
    auto walk_samples_dma = [&](auto same) {
        const int lane = threadIdx.x & 63;
        if constexpr (kHalf) {
            // the lane's 24 bytes of a row as three 8-byte pieces, each wholly in a head or a tail (1024 is a multiple of 8):
            // row r of the pair has its head at 1024 r and its tail at 2048 + 512 r
            int at[C], step[C];
#pragma unroll
            for (int k = 0; k < C; k++) {
                const int b = 24 * lane + 8 * k;
                at[k] = b < 1024 ? b : 1024 + b;
                step[k] = b < 1024 ? 1024 : 512;
            }
            acc_ring_walk<kD, 3>(dma_units, dma_first, dma_issue, [&](int p, int slot, auto refill) {
                const char *mine = reinterpret_cast<const char *>(ring + slot * 768);
                vhalf4 h[2][C];
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int k = 0; k < C; k++) h[r][k] = *reinterpret_cast<const vhalf4 *>(mine + at[k] + r * step[k]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the slot is refilled
                refill();
                vfloat4 q[C];
#pragma unroll
                for (int k = 0; k < C; k++) q[k] = __builtin_convertvector(h[0][k], vfloat4);
                fold_sample(q, 2 * p, same);
                if (2 * p + 1 < S) {
#pragma unroll
                    for (int k = 0; k < C; k++) q[k] = __builtin_convertvector(h[1][k], vfloat4);
                    fold_sample(q, 2 * p + 1, same);
                }
            });
        } else {
            acc_ring_walk<kD, 3>(S, dma_first, dma_issue, [&](int s, int slot, auto refill) {
                vfloat4 q[C];
                const float *mine = ring + slot * 768 + 12 * lane;
#pragma unroll
                for (int k = 0; k < C; k++) q[k] = *reinterpret_cast<const vfloat4 *>(mine + 4 * k);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the slot is refilled
                refill();
                fold_sample(q, s, same);
            });
        }
    };
    // wave-uniform choice: the fast walk only when every active lane qualifies
    const bool lane_same = !active || (n0[0] == n0[1] && n0[1] == n0[2] && n0[2] == n0[3]);
    if constexpr (kDma) {
        if (__builtin_amdgcn_ballot_w64(!lane_same) == 0) walk_samples_dma(std::true_type{});
        else walk_samples_dma(std::false_type{});
        if (!active) return;                                // nothing of an inactive lane is stored
    } else {
        if (__builtin_amdgcn_ballot_w64(!lane_same) == 0) walk_samples(std::true_type{});
        else walk_samples(std::false_type{});
    }
    store_plane<C>(t.mean + e0, st, &PairState::mean);
    store_plane<C, MAXM >= 2>(t.m2 + e0, st, &PairState::m2);
    store_plane<C, MAXM >= 3>(t.m3 + e0, st, &PairState::m3);
    store_plane<C, TRANSFORM>(t.film_mean + e0, st, &PairState::fmean);
    store_plane<C, TRANSFORM>(t.film_m2 + e0, st, &PairState::fm2);
    const int n_out[4] = {n0[0] + S, n0[1] + S, n0[2] + S, n0[3] + S};
    store_counts(t.n + p0, n_out);
    if constexpr (MAXM >= 3) {
        if (pre_mc != nullptr) store_prepass<C>(pre_mc + e0, pre_dc + e0, st, n_out, pre_table, pre_flags);
    }
}

// One pixel, scalar accesses: unaligned images, ragged ends, tiles whose rows do not split into
// 4-pixel groups.  Sample s of channel c is at sp[s * stride + c].
template <int C, int MAXM, bool TRANSFORM, typename ST = float>
__device__ __forceinline__ void accumulate_pixel(const AccumulateType &t, long long p, const ST *sp,
                                                 long long stride, int S) {
    const int n0 = t.n[p];
    float *const pre_mc = MAXM >= 3 ? t.mean_corr : nullptr;      // (read before the first store: see accumulate_lane)
    float *const pre_dc = MAXM >= 3 ? t.disc : nullptr;
    const int pre_table = t.pre_table, pre_flags = t.pre_flags;
    for (int c = 0; c < C; c++) {
        const long long e = p * C + c;
        ElemState st = {t.mean[e], MAXM >= 2 ? t.m2[e] : 0.f, MAXM >= 3 ? t.m3[e] : 0.f,
                        TRANSFORM ? t.film_mean[e] : 0.f, TRANSFORM ? t.film_m2[e] : 0.f};
        for (int s = 0; s < S; s++) {
            const float nf = (float)(n0 + s + 1);
            add_sample<MAXM, TRANSFORM>(st, nf, refined_rcp(nf), (float)sp[(long long)s * stride + c]);
        }
        t.mean[e] = st.mean;
        if (MAXM >= 2) t.m2[e] = st.m2;
        if (MAXM >= 3) t.m3[e] = st.m3;
        if (TRANSFORM) {
            t.film_mean[e] = st.fmean;
            t.film_m2[e] = st.fm2;
        }
        if (MAXM >= 3 && pre_mc != nullptr) {   // (the optional pre-pass epilogue, as in accumulate_lane)
            const int ni = n0 + S;
            float m, d;
            prepass_elem(ni, prepass_quantile(pre_table, pre_flags, ni), st.mean, st.m2, st.m3, m, d, (pre_flags & 2) != 0);
            pre_mc[e] = m;
            pre_dc[e] = d;
        }
    }
    t.n[p] = n0 + S;
}

// Film-major batch: one lane owns 4 consecutive PIXELS of one stat type and walks the batch's
// samples in order (sample s of pixel p, channel c is at samples[s*n_elems + p*C + c]).
template <int C, int MAXM, bool TRANSFORM, bool VEC, int UMUL, int DMA, typename ST = float>
__device__ __forceinline__ void accumulate_type(const AccumulateType &t, long long blk, long long nblk, float *ring, bool dma_first) {
    const ST *const samples = reinterpret_cast<const ST *>(t.samples);   // (t.stride and t.n_elems count elements, whatever their width)
    const long long n_px = t.n_elems / C;
    const long long n_groups = (n_px + 3) >> 2;
    const long long n_full = VEC ? (n_px >> 2) : 0;          // complete 4-pixel groups: the vector path's share
    const int lane = threadIdx.x & 63;
    // wave-uniform walk over the groups: the waves of a workgroup take 64 consecutive groups each (the LDS-DMA walk of the
    // RGB types is cooperative: every lane of a wave with at least one complete group calls in)
    for (long long gw = blk * kBlock + (threadIdx.x & ~63); gw < n_groups; gw += nblk * kBlock) {
        const long long g = gw + lane, p0 = g << 2;
        const bool active = g < n_full;
        const long long left = n_full - gw;
        const int n_active = left >= 64 ? 64 : left > 0 ? (int)left : 0;
        if constexpr (VEC) {    // (VEC = false: no complete group, by construction and not by what the compiler can prove of n_full)
            if (n_active > 0)
                accumulate_lane<C, MAXM, TRANSFORM, (!TRANSFORM && MAXM == 1) ? UMUL : 1, DMA, ST>(t, p0, samples + p0 * C, t.stride, t.n_samples,
                                                                                                    ring, active, n_active, dma_first);
        }
        if (!active && g < n_groups) {   // unaligned images, the ragged last group
            for (long long p = p0; p < n_px && p < p0 + 4; p++)
                accumulate_pixel<C, MAXM, TRANSFORM, ST>(t, p, samples + p * C, t.stride, t.n_samples);
        }
    }
}

// From a run-time descriptor to the compile-time shape of its walk: f(C, MAXM, TRANSFORM), each an integral constant.  The
// film-major, the 16-bit and the tile-fed kernels all come through here.
template <typename F>
__device__ __forceinline__ void acc_dispatch_type(const AccumulateType &t, F f) {
    auto moments = [&](auto c) {
        if (t.transform) {
            if (t.max_moment >= 3) f(c, std::integral_constant<int, 3>{}, std::true_type{});
            else if (t.max_moment == 2) f(c, std::integral_constant<int, 2>{}, std::true_type{});
            else f(c, std::integral_constant<int, 1>{}, std::true_type{});
        } else {
            if (t.max_moment >= 3) f(c, std::integral_constant<int, 3>{}, std::false_type{});
            else if (t.max_moment == 2) f(c, std::integral_constant<int, 2>{}, std::false_type{});
            else f(c, std::integral_constant<int, 1>{}, std::false_type{});
        }
    };
    if (t.channels == 3) moments(std::integral_constant<int, 3>{});
    else moments(std::integral_constant<int, 1>{});
}
// (the film-major kernels' use of it)
template <bool VEC, int UMUL, int DMA, typename ST = float>
__device__ __forceinline__ void accumulate_dispatch(const AccumulateType &t, long long blk, long long nblk, float *ring, bool dma_first) {
    acc_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
        accumulate_type<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, VEC, UMUL, DMA, ST>(t, blk, nblk, ring, dma_first);
    });
}

// Default grid: stat types are interleaved over a large 1-D grid (block b works on type
// b % n_types) so that the ALU-heavy radiance blocks (Box-Cox + third moment + raw-sample
// Welford) and the purely bandwidth-bound feature blocks are resident together.
// Resident grid (a.resident_blocks > 0, experiment hook): that many workgroups in total; each
// walks every stat type, starting at a different one, with a grid-stride loop.  Measured use:
// running this bandwidth-bound kernel beside the VALU-bound window filter of the previous
// iteration on a second stream gains <= 15 % (the two contend for VALU issue), so bench.py
// keeps the kernels back to back.
// (The three shapes stay written out, each with its own call of the walk, and accumulate_half_kernel keeps its own copy of the first
// two: one function handing a workgroup its (type, blk, nblk), called from ONE loop in both kernels, makes accumulate_kernel a third
// of the code -- 51 412 -> 17 262 instructions with the ring, 66 492 -> 22 322 without -- and the register walk slower: 1080p, 64
// samples per launch, per-type kernel, loads into registers 1.113 / 1.112 ms before against 1.155 - 1.157 with it, prefetch x 2
// 1.119 / 1.118 against 1.153 - 1.158; the LDS-DMA walk level, 1.031 - 1.045 against 1.030 - 1.036.  profiles/accumulate_onebody.jsonl)
template <bool VEC, int UMUL, int DMA, int OCC = kAccWaves>
__global__ __launch_bounds__(kBlock, OCC) void accumulate_kernel(AccumulateArgs a) {
    extern __shared__ __attribute__((aligned(16))) float acc_lds[];
    // the wave's LDS-DMA ring (RGB types, vector path); DMA = false (debug hook, A/B) keeps every type on register loads
    float *ring = DMA ? acc_lds + (threadIdx.x >> 6) * acc_ring_floats(DMA) : nullptr;
    if (a.resident_blocks > 0) {
        for (int i = 0; i < a.n_types; i++) {
            // (workgroup b starts with type b % n_types, so that every type is walked by a fifth of the grid at any time; every workgroup
            // starting with the same type: 3.92 against 3.75 ms; the eight workgroups of a dispatch round -- one per XCD -- with the same
            // type: no difference; profiles/r06_ab_resident_start.log)
            const AccumulateType t = a.t[((int)blockIdx.x + i) % a.n_types];   // (by value: see below)
            accumulate_dispatch<VEC, UMUL, DMA>(t, blockIdx.x, gridDim.x, ring, a.dma_first != 0);
        }
        return;
    }
    if (a.grid_mode == 1) {
        // One pass per workgroup: block b serves stat type b % n_types, groups [256 (b / n_types), + 256) -- every
        // workgroup of a type does the same amount of work, none walks a second, ragged stride.  The dispatcher hands the
        // blocks out in order, so the resident mix always holds every type and the launch ends within one workgroup's time.
        const int ti = blockIdx.x % a.n_types;
        // (a COPY of the descriptor, not a reference into the by-value kernel argument: with the pre-pass epilogue's fields in use a
        // reference made the compiler keep the whole 2-KB argument in a private copy -- scratch 2032 B per lane, + 17 VGPRs, the
        // accumulation 3.67 -> 4.60 ms; round 6)
        const AccumulateType t = a.t[ti];
        const long long blk = blockIdx.x / a.n_types, nblk = gridDim.x / a.n_types;
        accumulate_dispatch<VEC, UMUL, DMA>(t, blk, nblk, ring, a.dma_first != 0);
        return;
    }
    // Workgroups are dealt to the stat types in rounds of n_slots, each type holding a number of
    // slots proportional to its cost (bytes per pixel, radiance weighted up for its ALU work), so
    // that all types finish together instead of leaving the expensive one to run on alone.
    const int slot = blockIdx.x % a.n_slots, round = blockIdx.x / a.n_slots, n_rounds = gridDim.x / a.n_slots;
    const int ti = a.slot_type[slot];
    const AccumulateType t = a.t[ti];
    const long long blk = (long long)round * a.type_slots[ti] + a.slot_rank[slot];
    const long long nblk = (long long)n_rounds * a.type_slots[ti];
    accumulate_dispatch<VEC, UMUL, DMA>(t, blk, nblk, ring, a.dma_first != 0);
}

// Launches in which at least one type's arena is IEEE half (statmc_accumulate_formats; a.half_mask: bit i = type i) and which the
// type-fused walk below does not take: a kernel of its own, so that accumulate_kernel stays the code object it was.  Register
// loads for every type, the two launch shapes that need no slot table: a resident grid walking every type, or one pass per
// workgroup with the types round-robin.  VEC = false: every pixel through accumulate_pixel (unaligned arenas, pixel counts
// that are no multiple of 4).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void accumulate_half_kernel(AccumulateArgs a) {
    const bool resident = a.resident_blocks > 0;
    const int n_walks = resident ? a.n_types : 1;
    for (int i = 0; i < n_walks; i++) {
        const int ti = ((int)blockIdx.x + i) % a.n_types;
        const AccumulateType t = a.t[ti];                                      // (a copy: see accumulate_kernel)
        const long long blk = resident ? blockIdx.x : blockIdx.x / a.n_types, nblk = resident ? gridDim.x : gridDim.x / a.n_types;
        if ((a.half_mask >> ti) & 1) accumulate_dispatch<VEC, 1, 0, _Float16>(t, blk, nblk, nullptr, false);
        else accumulate_dispatch<VEC, 1, 0>(t, blk, nblk, nullptr, false);
    }
}

// ------------------------------------------------------------------ accumulate, every stat type of a pixel group in one walk
// The type-fused walk: a lane owns its 4-pixel group in EVERY stat type of the launch -- the radiance type (RGB, Box-Cox, three
// moments), K mean-only RGB types and M mean-only 1-channel types -- and folds sample s of all of them before sample s + 1 of
// any.  Every element still sees its own samples in order through the same add_sample2 stages, so the bits are those of
// accumulate_lane type after type.  What changes is the mix a wave runs: the radiance arithmetic issues while the wave's own
// feature rows are in flight (the per-type walk leaves a lone VALU-bound wave per SIMD in its radiance walk and an idle VALU in
// its feature walks), the count conversion and the refined reciprocal are formed once per sample instead of once per type, and
// a pixel group pays one chain of state-load, first-row and store latencies instead of one per type.
// Sample rows: all by LDS-DMA, one wave-private ring slot per sample -- three 1-KiB transfers per RGB type, one per 1-channel type
// (lane l fetches its own 16 bytes there), so the prefetch of no type lives in registers.  The rows are awaited by COUNT, hence
// a fixed issue order and a number of transfers per row that does not depend on how many lanes of the wave hold a group.
#ifndef STATMC_ACC_FUSED_D
#define STATMC_ACC_FUSED_D 3
#endif
constexpr int kAccFusedD = STATMC_ACC_FUSED_D;          // sample rows in flight per wave (2 against 3)
constexpr int kAccFusedTypes = 5;
struct AccumulateFusedArgs {
    AccumulateType t[kAccFusedTypes];   // the radiance type, the K mean-only RGB types, the M mean-only 1-channel types
    long long n_groups;                 // 4-pixel groups of the film (every type has the same pixels)
    int n_samples;                      // ... and the same batch length
};
// The wave's ring slot holds one sample row of every type.  FMT 0, every type fp32 (the kernels above all): 768 dwords per RGB type,
// the radiance type first, then 256 per 1-channel type.
// 16-bit arenas (statmc_accumulate_formats), FMT: 1 the feature types half and the radiance type fp32, 2 every type half.  A wave's
// half row is half as long -- 1 536 B of an RGB type, 512 B of a 1-channel type -- and
// arrives in 16-byte pieces like the fp32 rows: the first 1 KiB of an RGB row is one transfer of the wave; what is left of it and a
// 1-channel row are 512-B UNITS, 32 lanes' worth, and two units share one transfer (lanes 0 .. 31 fetch one, lanes 32 .. 63 the
// other: the source address of an LDS-DMA transfer is per lane, its destination is not).  An odd last unit is fetched twice, its
// second copy into 512 B nobody reads.  No lane sits a transfer out: a branch around an LDS-DMA builtin is not safe (the compiler
// threads such branches as if the transfer were a per-lane load), and the counted waits want every transfer issued anyway.
// Slot, in dwords: [radiance fp32: 768 (FMT 1)] [first KiB of every half RGB row: 256 each] [units: 128 each, a pair per transfer].
// This asks more of the arena than the register loads do: 16-byte aligned rows, i.e. a 16-byte aligned arena and a pixel count that
// is a multiple of 8 (plan_accumulate), and a wave that holds all its 64 groups -- the film's last, partial wave takes
// the register loads of accumulate_fused_ragged.  Rows and strides are counted in dwords, so the rows stay `const float *`.
constexpr bool acc_fused_is_half(int fmt, int i) { return fmt == 2 || (fmt == 1 && i >= 1); }
constexpr int acc_fused_head_offset(int fmt, int i) { return fmt == 2 ? 256 * i : 768 + 256 * (i - 1); }      // half RGB type i: its first KiB
constexpr int acc_fused_unit0(int fmt, int k) { return fmt == 2 ? 256 * (1 + k) : 768 + 256 * k; }
constexpr int acc_fused_unit_of(int fmt, int i) { return i - (fmt == 1 ? 1 : 0); }                            // half type i: its unit (RGB: the row's tail)
constexpr int acc_fused_units(int fmt, int k, int m) { return 1 + k + m - (fmt == 1 ? 1 : 0); }
constexpr int acc_fused_slot_dwords(int fmt, int k, int m) {
    return fmt == 0 ? 768 * (1 + k) + 256 * m : acc_fused_unit0(fmt, k) + 256 * ((acc_fused_units(fmt, k, m) + 1) / 2);
}
constexpr int acc_fused_transfers(int fmt, int k, int m) {
    return fmt == 0 ? 3 * (1 + k) + m : (fmt == 1 ? 3 : 1) + k + (acc_fused_units(fmt, k, m) + 1) / 2;
}
// ring depth: the half rows' shorter slots are spent on rows in flight, about the bytes per CU the fp32 ring holds (132 KiB for the
// 11-channel set): six all-half slots (6 KiB each per wave) are 144 KiB, five mixed ones (7 KiB) 140 KiB; T (D - 1) stays below 64
constexpr int acc_fused_depth(int fmt) { return fmt == 0 ? kAccFusedD : fmt == 2 ? 6 : 5; }
constexpr size_t acc_fused_ring_bytes(int fmt, int k, int m) {      // per workgroup: four waves
    return (size_t)4 * acc_fused_depth(fmt) * acc_fused_slot_dwords(fmt, k, m) * sizeof(float);
}
static_assert(acc_fused_ring_bytes(1, 2, 2) <= 160 * 1024 && acc_fused_ring_bytes(2, 2, 2) <= 160 * 1024, "the ring of a workgroup must fit the CU's LDS");

// A wave whose lanes do not all hold one count per group in every type (adaptively sampled films): today's walk, type after
// type, in the wave's ring -- the same bits, no second ragged code.
template <int K, int M, int D, int FMT = 0>
__device__ __forceinline__ void accumulate_fused_ragged(const AccumulateFusedArgs &a, long long gw, int n_active, float *ring) {
    // (the descriptors below are picked by comparisons, never by a run-time index into the kernel argument -- see accumulate_kernel on
    // what that costs; with at most two types of a kind "the first or the last" names them all)
    static_assert(K >= 0 && K <= 2 && M >= 0 && M <= 2, "a.t[1] / a.t[K] and a.t[1 + K] / a.t[K + M] name every feature type only up to two of a kind");
    constexpr int kFit = D * acc_fused_slot_dwords(FMT, K, M) / 768;       // rows of one RGB type the wave's ring holds
    constexpr int FD = FMT != 0 ? 0 : kFit < kAccDmaD ? kFit : kAccDmaD;   // (launches with 16-bit arenas: register loads, whatever the type's format)
    typedef typename std::conditional<FMT == 2, _Float16, float>::type ST0;
    typedef typename std::conditional<FMT != 0, _Float16, float>::type STF;
    const int lane = threadIdx.x & 63;
    const long long p0 = (gw + lane) << 2;
    const bool active = lane < n_active;
    const int S = a.n_samples;
    {
        const AccumulateType t = a.t[0];    // (copies, not references into the kernel argument: see accumulate_kernel)
        accumulate_lane<3, 3, true, 1, FD, ST0>(t, p0, reinterpret_cast<const ST0 *>(t.samples) + p0 * 3, t.stride, S, ring, active, n_active, false);
    }
    if constexpr (K > 0) {
#pragma unroll 1
        for (int i = 0; i < K; i++) {
            const AccumulateType t = i == 0 ? a.t[1] : a.t[K];
            accumulate_lane<3, 1, false, 1, FD, STF>(t, p0, reinterpret_cast<const STF *>(t.samples) + p0 * 3, t.stride, S, ring, active, n_active, false);
        }
    }
    if constexpr (M > 0) {
#pragma unroll 1
        for (int i = 0; i < M; i++) {
            const AccumulateType t = i == 0 ? a.t[1 + K] : a.t[K + M];
            accumulate_lane<1, 1, false, 1, FD, STF>(t, p0, reinterpret_cast<const STF *>(t.samples) + p0, t.stride, S, ring, active, n_active, false);
        }
    }
}

// The wave's 64 groups from group gw on (the first n_active of them exist; wave-uniform arguments).
template <int K, int M, int D, int FMT = 0>
__device__ __forceinline__ void accumulate_fused_wave(const AccumulateFusedArgs &a, long long gw, int n_active, float *ring) {
    constexpr int NT = 1 + K + M;
    constexpr int SLOT = acc_fused_slot_dwords(FMT, K, M);
    constexpr int T = acc_fused_transfers(FMT, K, M);       // transfers per sample row
    constexpr int KA = K > 0 ? K : 1, MA = M > 0 ? M : 1;
    const int lane = threadIdx.x & 63;
    const bool active = lane < n_active;
    const long long p0 = active ? (gw + lane) << 2 : 0;     // an inactive lane reads group 0 and stores nothing
    const int S = a.n_samples;
    // counts first: which walk the wave takes
    int nb[NT];
    bool lane_same = true, lane_one = true;
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int4 n4 = *reinterpret_cast<const int4 *>(a.t[i].n + p0);
        nb[i] = n4.x;
        lane_same = lane_same && n4.x == n4.y && n4.y == n4.z && n4.z == n4.w;
        lane_one = lane_one && n4.x == nb[0];
    }
    if (__builtin_amdgcn_ballot_w64(active && !lane_same) != 0 || (FMT != 0 && n_active < 64)) {
        accumulate_fused_ragged<K, M, D, FMT>(a, gw, n_active, ring);
        return;
    }
    // (the descriptors' fields, all read before the first store: see accumulate_lane)
    float *const r_mean = a.t[0].mean, *const r_m2 = a.t[0].m2, *const r_m3 = a.t[0].m3, *const r_fmean = a.t[0].film_mean,
                 *const r_fm2 = a.t[0].film_m2, *const pre_mc = a.t[0].mean_corr, *const pre_dc = a.t[0].disc;
    const int pre_table = a.t[0].pre_table, pre_flags = a.t[0].pre_flags;
    int32_t *n_ptr[NT];
    float *f_mean[NT];
    const float *row[NT];       // the wave's next sample row to request, per type
    long long stride[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
        n_ptr[i] = a.t[i].n;
        f_mean[i] = a.t[i].mean;
        // (a half row and its stride in dwords: half the elements -- the pixel count is a multiple of 4)
        row[i] = a.t[i].samples + (((gw << 2) * (i <= K ? 3 : 1)) >> (acc_fused_is_half(FMT, i) ? 1 : 0));
        stride[i] = a.t[i].stride >> (acc_fused_is_half(FMT, i) ? 1 : 0);
    }
    // (every lane issues every transfer of a row, whatever part of the row exists: acc_row_piece; a 1-channel row likewise)
    int piece3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) piece3[k] = acc_row_piece(k, lane, n_active);
    const int piece1 = active ? 4 * lane : 0;
    auto issue = [&](int, int slot) {      // (the rows are requested in order: row[] moves on by itself)
        float *dst = ring + slot * SLOT;
        if constexpr (FMT != 0) {
            // (full waves only; FMT 0 keeps the statements below, with their offsets written as they always were)
            constexpr int NU = acc_fused_units(FMT, K, M), U0 = acc_fused_unit0(FMT, K);
            const float *unit[NU + 1];
#pragma unroll
            for (int i = 0; i < NT; i++) {
                if (!acc_fused_is_half(FMT, i)) {       // the fp32 radiance row of a mixed launch
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        __builtin_amdgcn_global_load_lds(row[i] + 256 * k + 4 * lane, (__attribute__((address_space(3))) void *)(dst + 256 * k), 16, 0, 2);
                } else if (i <= K) {
                    __builtin_amdgcn_global_load_lds(row[i] + 4 * lane, (__attribute__((address_space(3))) void *)(dst + acc_fused_head_offset(FMT, i)), 16, 0, 2);
                    unit[acc_fused_unit_of(FMT, i)] = row[i] + 256;
                } else {
                    unit[acc_fused_unit_of(FMT, i)] = row[i];
                }
                row[i] += stride[i];
            }
            unit[NU] = unit[NU - 1];
#pragma unroll
            for (int u = 0; u < NU; u += 2)
                __builtin_amdgcn_global_load_lds((lane < 32 ? unit[u] : unit[u + 1] - 128) + 4 * lane,
                                                 (__attribute__((address_space(3))) void *)(dst + U0 + 128 * u), 16, 0, 2);
            return;
        }
#pragma unroll
        for (int i = 0; i < NT; i++) {
            if (i <= K) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    __builtin_amdgcn_global_load_lds(row[i] + piece3[k], (__attribute__((address_space(3))) void *)(dst + 768 * i + 256 * k), 16, 0, 2);
            } else {
                __builtin_amdgcn_global_load_lds(row[i] + piece1, (__attribute__((address_space(3))) void *)(dst + 768 * (1 + K) + 256 * (i - 1 - K)), 16, 0, 2);
            }
            row[i] += stride[i];
        }
    };
    // state: radiance 5 planes, every feature type its mean
    const long long e3 = p0 * 3;
    PairState st[6], fr[KA][6], f1[MA][2];
    load_plane<3>(st, &PairState::mean, r_mean + e3);
    load_plane<3>(st, &PairState::m2, r_m2 + e3);
    load_plane<3>(st, &PairState::m3, r_m3 + e3);
    load_plane<3>(st, &PairState::fmean, r_fmean + e3);
    load_plane<3>(st, &PairState::fm2, r_fm2 + e3);
#pragma unroll
    for (int i = 0; i < K; i++) load_plane<3>(fr[i], &PairState::mean, f_mean[1 + i] + e3);
#pragma unroll
    for (int i = 0; i < M; i++) load_plane<1>(f1[i], &PairState::mean, f_mean[1 + K + i] + p0);
    // ONE: every type of the wave starts from the same count (all but films whose radiance has seen samples the features have
    // not): one count conversion and one refined reciprocal per sample for all of them, else one per type.
    auto walk = [&](auto one) {
        acc_ring_walk<D, T>(S, false, issue, [&](int s, int slot, auto refill) {
            const float *mine = ring + slot * SLOT;
            vfloat4 q[1 + K][3], q1[MA];
            if constexpr (FMT != 0) {
                // a half piece is read as it lies (8-byte LDS reads: lane l's 6 dwords of an RGB row start 6 l dwords into it, before
                // or behind the row's first KiB) and widened once the slot is free again
                constexpr int U0 = acc_fused_unit0(FMT, K);
                vhalf4 h[1 + K][3], h1[MA];
#pragma unroll
                for (int i = 0; i <= K; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (acc_fused_is_half(FMT, i)) {
                            const int o = 6 * lane + 2 * k;
                            const int at = o < 256 ? acc_fused_head_offset(FMT, i) + o : U0 + 128 * acc_fused_unit_of(FMT, i) + o - 256;
                            h[i][k] = *reinterpret_cast<const vhalf4 *>(mine + at);
                        } else {
                            q[i][k] = *reinterpret_cast<const vfloat4 *>(mine + 12 * lane + 4 * k);
                        }
                    }
#pragma unroll
                for (int i = 0; i < M; i++) h1[i] = *reinterpret_cast<const vhalf4 *>(mine + U0 + 128 * acc_fused_unit_of(FMT, 1 + K + i) + 2 * lane);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the slot is refilled
#pragma unroll
                for (int i = 0; i <= K; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        if (acc_fused_is_half(FMT, i)) q[i][k] = __builtin_convertvector(h[i][k], vfloat4);
#pragma unroll
                for (int i = 0; i < M; i++) q1[i] = __builtin_convertvector(h1[i], vfloat4);
            } else {
#pragma unroll
            for (int i = 0; i <= K; i++)
#pragma unroll
                for (int k = 0; k < 3; k++) q[i][k] = *reinterpret_cast<const vfloat4 *>(mine + 768 * i + 12 * lane + 4 * k);
#pragma unroll
            for (int i = 0; i < M; i++) q1[i] = *reinterpret_cast<const vfloat4 *>(mine + 768 * (1 + K) + 256 * i + 4 * lane);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the slot is refilled
            }
            refill();
            v2f nf[NT], rc[NT];
            if constexpr (decltype(one)::value) {
                const float nf0 = (float)(nb[0] + s + 1);
                const float rc0 = refined_rcp(nf0);
#pragma unroll
                for (int i = 0; i < NT; i++) { nf[i] = v2f{nf0, nf0}; rc[i] = v2f{rc0, rc0}; }
            } else {
#pragma unroll
                for (int i = 0; i < NT; i++) {
                    const float nfi = (float)(nb[i] + s + 1);
                    const float rci = refined_rcp(nfi);
                    nf[i] = v2f{nfi, nfi};
                    rc[i] = v2f{rci, rci};
                }
            }
            // the feature types first (their temporaries are few), then the radiance type
#pragma unroll
            for (int i = 0; i < M; i++) {
                const v2f nf2[2] = {nf[1 + K + i], nf[1 + K + i]}, rc2[2] = {rc[1 + K + i], rc[1 + K + i]};
                const v2f smp2[2] = {v2f{q1[i][0], q1[i][1]}, v2f{q1[i][2], q1[i][3]}};
                add_sample2<2, 1, false>(f1[i], nf2, rc2, smp2);
            }
            auto fold3 = [&](PairState *state, int i, auto radiance) {
                const v2f nf3[3] = {nf[i], nf[i], nf[i]}, rc3[3] = {rc[i], rc[i], rc[i]};
                v2f smp2[6];
#pragma unroll
                for (int j = 0; j < 6; j++) smp2[j] = v2f{q[i][j >> 1][2 * (j & 1)], q[i][j >> 1][2 * (j & 1) + 1]};
#pragma unroll
                for (int g = 0; g < 6; g += kAccPairGroup) {
                    if constexpr (decltype(radiance)::value) add_sample2<kAccPairGroup, 3, true>(state + g, nf3, rc3, smp2 + g);
                    else add_sample2<kAccPairGroup, 1, false>(state + g, nf3, rc3, smp2 + g);
                }
            };
#pragma unroll
            for (int i = 0; i < K; i++) fold3(fr[i], 1 + i, std::false_type{});
            fold3(st, 0, std::true_type{});
        });
    };
    if (__builtin_amdgcn_ballot_w64(active && !lane_one) == 0) walk(std::true_type{});
    else walk(std::false_type{});
    if (!active) return;                                    // nothing of an inactive lane is stored
    store_plane<3>(r_mean + e3, st, &PairState::mean);
    store_plane<3>(r_m2 + e3, st, &PairState::m2);
    store_plane<3>(r_m3 + e3, st, &PairState::m3);
    store_plane<3>(r_fmean + e3, st, &PairState::fmean);
    store_plane<3>(r_fm2 + e3, st, &PairState::fm2);
#pragma unroll
    for (int i = 0; i < K; i++) store_plane<3>(f_mean[1 + i] + e3, fr[i], &PairState::mean);
#pragma unroll
    for (int i = 0; i < M; i++) store_plane<1>(f_mean[1 + K + i] + p0, f1[i], &PairState::mean);
    // every group of this walk holds one count per type: one count to store, and one quantile for the radiance type's optional
    // pre-pass epilogue
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int n_out[1] = {nb[i] + S};
        store_counts(n_ptr[i] + p0, n_out);
    }
    if (pre_mc != nullptr) {
        const int n_out[1] = {nb[0] + S};
        store_prepass<3>(pre_mc + e3, pre_dc + e3, st, n_out, pre_table, pre_flags);
    }
}

// A resident grid: every workgroup walks 256-group units with a grid stride, its four waves 64 consecutive groups each, every
// pass covering every type.  One wave per SIMD (the ring of the 11-channel set at three rows is 132 KiB per workgroup).
template <int K, int M, int D, int FMT>
__device__ __forceinline__ void accumulate_fused_grid(const AccumulateFusedArgs &a) {
    extern __shared__ __attribute__((aligned(16))) float acc_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *ring = acc_lds + wave * (D * acc_fused_slot_dwords(FMT, K, M));
    for (long long gw = (long long)blockIdx.x * kBlock + wave * 64; gw < a.n_groups; gw += (long long)gridDim.x * kBlock) {
        const long long left = a.n_groups - gw;
        accumulate_fused_wave<K, M, D, FMT>(a, gw, left >= 64 ? 64 : (int)left, ring);
    }
}
template <int K, int M, int D>
__global__ __launch_bounds__(kBlock, 1) void accumulate_fused_kernel(AccumulateFusedArgs a) {
    accumulate_fused_grid<K, M, D, 0>(a);
}
// The same grid for launches with 16-bit arenas: a kernel of its own, so that the fp32 one above stays the code object it was.
template <int K, int M, int FMT>
__global__ __launch_bounds__(kBlock, 1) void accumulate_fused_half_kernel(AccumulateFusedArgs a) {
    accumulate_fused_grid<K, M, acc_fused_depth(FMT), FMT>(a);
}

// The launches the fused walk serves: exactly one RGB type with the transform and three moments, K <= 2 mean-only RGB types,
// M <= 2 mean-only 1-channel types, K + M >= 1, in any order; the same pixels and the same batch length in every type.
static bool accumulate_fused_plan(const AccumulateArgs &a, AccumulateFusedArgs &f, int &K, int &M, int *order) {
    K = M = 0;
    if (a.n_types < 2 || a.n_types > kAccFusedTypes) return false;
    const long long n_px = a.t[0].n_elems / a.t[0].channels;
    const int S = a.t[0].n_samples;
    if (S < 1 || n_px < 4 || n_px % 4 != 0) return false;
    int rad = -1, rgb[2] = {0, 0}, f1[2] = {0, 0};
    for (int i = 0; i < a.n_types; i++) {
        const AccumulateType &t = a.t[i];
        if (t.n_elems / t.channels != n_px || t.n_samples != S) return false;
        if (t.channels == 3 && t.transform && t.max_moment >= 3) {
            if (rad >= 0) return false;
            rad = i;
        } else if (!t.transform && t.max_moment == 1 && t.channels == 3) {
            if (K == 2) return false;
            rgb[K++] = i;
        } else if (!t.transform && t.max_moment == 1 && t.channels == 1) {
            if (M == 2) return false;
            f1[M++] = i;
        } else {
            return false;
        }
    }
    if (rad < 0 || K + M < 1) return false;
    f = AccumulateFusedArgs{};
    f.t[0] = a.t[rad];
    for (int i = 0; i < K; i++) f.t[1 + i] = a.t[rgb[i]];
    for (int i = 0; i < M; i++) f.t[1 + K + i] = a.t[f1[i]];
    f.n_groups = n_px / 4;
    f.n_samples = S;
    order[0] = rad;                 // f.t[j] is a.t[order[j]]
    for (int i = 0; i < K; i++) order[1 + i] = rgb[i];
    for (int i = 0; i < M; i++) order[1 + K + i] = f1[i];
    return true;
}

// The vector path of one stat type: every plane it has is 16-byte aligned, the pre-pass epilogue's images too, and, in a film-major
// launch, the element count and the sample stride keep every sample plane so.  A half arena wants 8 bytes and whole 4-pixel groups
// (n_elems % (4 channels)); an fp32 one is asked for n_elems % 4, which says the same of every count the C ABI can hand over
// (pixels x channels, channels 1 or 3), also of an fp32 type beside half ones.  A tile-fed launch checks its rows tile by tile.
bool acc_type_vectorizable(const AccumulateType &t, bool half_arena, bool film_major) {
    const long long whole = half_arena ? 4 * t.channels : 4;
    return (half_arena ? (reinterpret_cast<uintptr_t>(t.samples) & 7) == 0 : aligned16(t.samples)) && aligned16(t.n) && aligned16(t.mean) &&
           (t.max_moment < 2 || aligned16(t.m2)) && (t.max_moment < 3 || aligned16(t.m3)) &&
           (!t.transform || (aligned16(t.film_mean) && aligned16(t.film_m2))) &&
           (!t.mean_corr || (aligned16(t.mean_corr) && aligned16(t.disc))) &&
           (!film_major || (t.n_elems % whole == 0 && t.stride % whole == 0));
}

// The fused kernels ask for more dynamic LDS than a launch may have by default: allowed once per kernel, device and thread.
template <void (*KERNEL)(AccumulateFusedArgs)>
static hipError_t launch_big_lds(size_t lds, const AccumulateFusedArgs &f, unsigned blocks, hipStream_t s) {
    static thread_local unsigned long long allowed = 0;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !((allowed >> dev) & 1)) {
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) allowed |= 1ull << dev;
    }
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(kBlock), lds, s, f);
    return hipGetLastError();
}
template <int FMT, int K, int M>
static hipError_t launch_accumulate_fused_km(const AccumulateFusedArgs &f, unsigned blocks, hipStream_t s) {
    if constexpr (FMT == 0) return launch_big_lds<&accumulate_fused_kernel<K, M, kAccFusedD>>(acc_fused_ring_bytes(FMT, K, M), f, blocks, s);
    else return launch_big_lds<&accumulate_fused_half_kernel<K, M, FMT>>(acc_fused_ring_bytes(FMT, K, M), f, blocks, s);
}
template <int FMT>
static hipError_t launch_accumulate_fused(const AccumulateFusedArgs &f, int K, int M, unsigned blocks, hipStream_t s) {
    switch (3 * K + M) {
    case 1: return launch_accumulate_fused_km<FMT, 0, 1>(f, blocks, s);
    case 2: return launch_accumulate_fused_km<FMT, 0, 2>(f, blocks, s);
    case 3: return launch_accumulate_fused_km<FMT, 1, 0>(f, blocks, s);
    case 4: return launch_accumulate_fused_km<FMT, 1, 1>(f, blocks, s);
    case 5: return launch_accumulate_fused_km<FMT, 1, 2>(f, blocks, s);
    case 6: return launch_accumulate_fused_km<FMT, 2, 0>(f, blocks, s);
    case 7: return launch_accumulate_fused_km<FMT, 2, 1>(f, blocks, s);
    case 8: return launch_accumulate_fused_km<FMT, 2, 2>(f, blocks, s);
    }
    return hipErrorInvalidValue;
}

static thread_local unsigned g_last_acc_grid = 0;
static thread_local int g_last_acc_fused = 0, g_last_acc_loader = 0;
unsigned last_accumulate_grid() { return g_last_acc_grid; }   // workgroups of the calling thread's last film-major launch (tests)
int last_accumulate_fused() { return g_last_acc_fused; }      // ... and whether it ran the type-fused walk
int last_accumulate_loader() { return g_last_acc_loader; }    // ... and how its 16-bit arenas were read: 0 none, 1 vector path, 2 element by element

// Slots of the capped grid per type ~ relative cost: 4 B x channels per sample, x 1.3 for transform types: 4 / 3 / 1 slots
// (rgb transform / rgb / float).
static int acc_type_slots(const AccumulateType &t) {
    const int w = (t.channels * (t.transform ? 4 : 3) + 2) / 3;
    return w < 1 ? 1 : w;
}
// The capped grid's slot table: the slots of different types interleaved (round-robin over types) so that neighbours differ.
static void acc_fill_slots(AccumulateArgs &a) {
    a.n_slots = 0;
    for (int i = 0; i < a.n_types; i++) a.type_slots[i] = acc_type_slots(a.t[i]);
    for (int r = 0, left = 1; left && a.n_slots < kMaxSlots; r++) {
        left = 0;
        for (int i = 0; i < a.n_types && a.n_slots < kMaxSlots; i++)
            if (r < a.type_slots[i]) {
                a.slot_type[a.n_slots] = (unsigned char)i;
                a.slot_rank[a.n_slots] = (unsigned char)r;
                a.n_slots++;
                left = 1;
            }
    }
}

// Every rule of the film-major launch, from the argument alone (no HIP call, no global state: tests/cpp/test_accumulate_plan.cpp
// runs it without a GPU and tests/golden/accumulate_plan.json pins what it answers).  The measurements behind each rule:
// DESIGN.md 4.1 and, under the names given here, HISTORY.md 4.1f.
AccumulatePlan plan_accumulate(const AccumulateArgs &a, AccumulateFusedArgs *fused_out) {
    AccumulatePlan p{};
    const bool any_half = a.half_mask != 0;
    // The vector path: every type passes acc_type_vectorizable.  rows16: what the fused half walk's LDS-DMA rows want beyond
    // that -- 16-byte aligned half rows, i.e. a 16-byte aligned arena and a multiple of 8 pixels.
    bool vec = true, rows16 = true;
    long long max_groups = 1;
    int max_s = 0, n_slots = 0;
    for (int i = 0; i < a.n_types; i++) {
        const AccumulateType &t = a.t[i];
        const bool half = (a.half_mask >> i) & 1;
        vec = vec && acc_type_vectorizable(t, half, true);
        rows16 = rows16 && (!half || (aligned16(t.samples) && t.n_elems % (8 * t.channels) == 0 && t.stride % (8 * t.channels) == 0));
        const long long groups = (t.n_elems / t.channels + 3) / 4;
        if (groups > max_groups) max_groups = groups;
        if (t.n_samples > max_s) max_s = t.n_samples;
        n_slots += acc_type_slots(t);
    }
    if (n_slots > kMaxSlots) n_slots = kMaxSlots;
    const long long units = (max_groups + kBlock - 1) / kBlock;     // workgroups that cover the largest type once
    p.vec = vec ? 1 : 0;
    p.loader = any_half ? (vec ? 1 : 2) : 0;
    p.umul = 1;
    // A resident grid of the per-type kernel: the number asked for (statmc_debug_accumulate_resident_blocks), or, fp32 arenas
    // only, one workgroup per CU on 1080p-sized films ([2^18, 3 x 2^18) groups) from 256 samples per launch up with placed
    // buffers, where the film's groups fill the workgroups' last walk to 97 % at least (HISTORY.md 4.1f, "one workgroup per CU").
    p.resident_blocks = a.resident_blocks > 0 ? a.resident_blocks : 0;
    if (!any_half && a.resident_blocks == 0 && a.grid_mode < 0 && a.apart && a.cus > 0 && max_s >= 256 && max_groups >= (1 << 18) && max_groups < 3 * (1 << 18)) {
        const double walks = (double)max_groups / ((double)a.cus * kBlock);
        if (walks / ceil(walks) >= 0.97) p.resident_blocks = a.cus;
    }
    // The type-fused walk: never with statmc_debug_accumulate_fused(-1), statmc_debug_accumulate_resident_blocks(-1), the LDS-DMA
    // walk switched off or off the vector path; min(CUs, units) workgroups, or the resident grid's number.
    // fp32 arenas, by shape (a.fused = 0): wherever the resident grid above stands, and from 128 samples per launch up on films of
    // 960 x 540 to 1920 x 1080 ([128 000, 2^19) groups), whatever the allocator; a.fused = 1: every eligible launch (DESIGN.md 4.1,
    // HISTORY.md 4.1e and 4.1f, "the type-fused walk").
    // 16-bit arenas: whenever the rows are 16-byte aligned and the feature types are half, the radiance type in either format
    // (DESIGN.md 4.1d); every other mix of formats takes the per-type half kernel.
    if (a.fused >= 0 && a.resident_blocks >= 0 && vec && a.dma && (!any_half || rows16)) {
        const bool by_shape = a.fused == 0 && a.resident_blocks == 0 && a.grid_mode < 0 && a.cus > 0 &&
                              (p.resident_blocks > 0 || (max_s >= 128 && max_groups >= 128000 && max_groups < (1 << 19)));
        AccumulateFusedArgs f;
        int K = 0, M = 0, order[kAccFusedTypes];
        if ((any_half || by_shape || a.fused == 1) && accumulate_fused_plan(a, f, K, M, order)) {
            bool features_half = true;
            for (int j = 1; j < 1 + K + M; j++) features_half = features_half && ((a.half_mask >> order[j]) & 1);
            if (!any_half || features_half) {
                p.kernel = any_half ? kAccFusedHalf : kAccFused;
                p.K = K;
                p.M = M;
                p.fmt = !any_half ? 0 : ((a.half_mask >> order[0]) & 1) ? 2 : 1;
                p.grid = p.resident_blocks > 0 ? (unsigned)p.resident_blocks : (unsigned)(a.cus > 0 && a.cus < units ? a.cus : units);
                p.lds = acc_fused_ring_bytes(p.fmt, K, M);
                if (fused_out) *fused_out = f;
                return p;
            }
        }
    }
    // The per-type half kernel (register loads, no slot table): the resident grid asked for, or one pass per workgroup.
    if (any_half) {
        p.kernel = kAccPerTypeHalf;
        p.grid_mode = 1;
        p.grid = p.resident_blocks > 0 ? (unsigned)p.resident_blocks : (unsigned)(units * a.n_types);
        return p;
    }
    // The per-type fp32 kernel's shape where no resident grid stands.  0, the capped grid: every type holds slots in proportion
    // to its cost, grid-stride walk.  1: every workgroup makes ONE pass, types round-robin -- short batches, which are bound by
    // the chain of latencies a workgroup pays per pass (up to 8 samples, up to 16 on films below 2^20 groups: HISTORY.md 4.1f,
    // "launch shape"); with placed buffers also films from 2^20 groups up and batches from 128 samples up, so that only 17 - 127
    // samples on smaller films keep the capped grid ("launch shape, placed buffers").
    p.kernel = kAccPerType;
    p.grid_mode = a.grid_mode;
    if (a.grid_mode < 0) {
        const bool big = max_groups >= (1 << 20);
        if (a.apart) p.grid_mode = (max_s <= 16 || big || max_s >= 128) ? 1 : 0;
        else p.grid_mode = (max_s <= 8 || (max_s <= 16 && !big)) ? 1 : 0;
    }
    const int rounds = (grid_for(max_groups, 256 * 8) * a.n_types + n_slots - 1) / n_slots;
    p.grid = p.resident_blocks > 0 ? (unsigned)p.resident_blocks : p.grid_mode == 1 ? (unsigned)(units * a.n_types) : (unsigned)(rounds * n_slots);
    // the LDS-DMA ring (a.dma, default) and the deeper prefetch of the mean-only types (a.umul = 2, A/B) exist on the vector path only
    if (vec && a.dma) {
        p.dma = kAccDmaD;
        p.lds = acc_lds_bytes(kAccDmaD);
    } else if (vec && a.umul == 2) {
        p.umul = 2;
    }
    return p;
}

hipError_t launch_accumulate(const AccumulateArgs &a_in, hipStream_t s) {
    AccumulateFusedArgs f;
    const AccumulatePlan p = plan_accumulate(a_in, &f);
    AccumulateArgs a = a_in;
    a.resident_blocks = p.resident_blocks;
    a.grid_mode = p.grid_mode;
    if (p.kernel == kAccPerType && p.resident_blocks == 0 && p.grid_mode != 1) acc_fill_slots(a);
    g_last_acc_grid = p.grid;
    g_last_acc_fused = p.kernel == kAccFused || p.kernel == kAccFusedHalf;
    g_last_acc_loader = p.loader;
    const dim3 grid(p.grid), block(kBlock);
    switch (p.kernel) {
    case kAccPerType:
        if (p.dma) hipLaunchKernelGGL((accumulate_kernel<true, 1, kAccDmaD>), grid, block, p.lds, s, a);
        else if (p.umul == 2) hipLaunchKernelGGL((accumulate_kernel<true, 2, 0>), grid, block, 0, s, a);
        else if (p.vec) hipLaunchKernelGGL((accumulate_kernel<true, 1, 0>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((accumulate_kernel<false, 1, 0>), grid, block, 0, s, a);
        break;
    case kAccPerTypeHalf:
        if (p.vec) hipLaunchKernelGGL((accumulate_half_kernel<true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((accumulate_half_kernel<false>), grid, block, 0, s, a);
        break;
    case kAccFused: return launch_accumulate_fused<0>(f, p.K, p.M, p.grid, s);
    case kAccFusedHalf: return p.fmt == 2 ? launch_accumulate_fused<2>(f, p.K, p.M, p.grid, s) : launch_accumulate_fused<1>(f, p.K, p.M, p.grid, s);
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ accumulate, tile by tile
// The same update fed the way StatPathIntegrator::Render produces samples (statpath.cpp:132-190,
// 355-388): every tile of the film (16 x 16 there) hands over the samples of one iteration as one
// block [S_tile][tile_h][tile_w][C] of a per-type arena, S_tile the same for every pixel of the
// tile but free to differ between tiles.  One wave per (tile, type): a 16 x 16 tile is exactly
// 64 lanes x 4 pixels, a sample plane of the block is one contiguous 1 / 3 KiB read of the wave.
// ST: what the type's arena holds (statmc_accumulate_tiles_formats) -- float, or _Float16 through the half loaders of
// accumulate_lane / accumulate_pixel (register loads); off, stride and the walk count elements of either width.  vec: the
// type's images (and arena) are aligned for the vector path.
template <int C, int MAXM, bool TRANSFORM, int UMUL, int DMA, typename ST = float>
__device__ __forceinline__ void accumulate_tile(const AccumulateType &t, const AccumulateTilesArgs &a, bool vec, int x0, int y0,
                                                int tw, int th, long long off, int S, float *ring) {
    const int lane = threadIdx.x & 63;
    const int npx = tw * th;
    const ST *base = reinterpret_cast<const ST *>(t.samples) + off * C;
    const long long stride = (long long)npx * C;
    // rows split into 16-B aligned 4-pixel groups: tile width, tile origin, image width and the
    // block's offset are all multiples of 4 (and the images themselves 16-B aligned: vec)
    bool fast = vec && ((tw | x0 | a.width) & 3) == 0 && (off & 3) == 0;
    // half RGB rows by LDS-DMA: 16-byte pieces of 16-byte aligned rows -- a 16-byte aligned block and a multiple of 8 pixels
    // (every 16 x 16 tile and its 8-wide or 8-high parts).  Other blocks go element by element in that kernel: the register walk
    // beside the ring would cost it the second wave per SIMD.
    if constexpr (DMA > 0 && C == 3 && !std::is_same<ST, float>::value) fast = fast && (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (npx & 7) == 0;
    if (fast) {
        const int n_g = npx >> 2;
        for (int gw = 0; gw < n_g; gw += 64) {   // wave-uniform: the LDS-DMA walk of the RGB types is cooperative
            const int g = gw + lane;
            const bool active = g < n_g;
            const int i = g << 2, row = i / tw, col = i - row * tw;
            const long long p0 = (long long)(y0 + row) * a.width + x0 + col;
            // deeper prefetch only where the state is one plane (mean-only feature types): the registers are there
            accumulate_lane<C, MAXM, TRANSFORM, (!TRANSFORM && MAXM == 1) ? UMUL : 1, DMA, ST>(t, p0, base + (long long)i * C, stride, S, ring, active,
                                                                                                n_g - gw >= 64 ? 64 : n_g - gw, a.dma_first != 0);
        }
    } else {
        for (int i = lane; i < npx; i += 64) {
            const int row = i / tw, col = i - row * tw;
            const long long p = (long long)(y0 + row) * a.width + x0 + col;
            accumulate_pixel<C, MAXM, TRANSFORM, ST>(t, p, base + (long long)i * C, stride, S);
        }
    }
}

template <int UMUL, int DMA>
__global__ __launch_bounds__(kBlock) void accumulate_tiles_kernel(AccumulateTilesArgs a) {
    extern __shared__ __attribute__((aligned(16))) float acc_lds[];
    float *ring = DMA ? acc_lds + (threadIdx.x >> 6) * acc_ring_floats(DMA) : nullptr;
    // a.order = 2 (the default since round 5): a workgroup = four consecutive tiles of ONE type, workgroups round-robin over the
    // types -- the four waves' state rows are 768 contiguous bytes (192 with the types of ONE tile per workgroup, order 0, where
    // the neighbouring tile's rows are another workgroup's, usually on another XCD: every line of the moments fetched into two L2s):
    // + 2 - 6 % at 4 .. 64 samples per tile, 1080p and 4K (profiles/r05_tiles_order.log); CUs still hold every type at any time
    const long long n_items = a.order == 2 ? (((long long)a.n_tiles + 3) >> 2) * 4 * a.n_types : (long long)a.n_tiles * a.n_types;
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    // a.order = 0 (rounds 2 - 4; A/B): item = (tile, type), types innermost: the waves of a workgroup work on the types of one
    // tile, so ALU-heavy radiance items and bandwidth-only feature items share every CU
    // (a.order = 1, experiment: tiles innermost -- neighbouring waves read neighbouring blocks of one type's arena)
    // Round 6, two experiments on why this walk trails the film-major kernel at 4 - 16 samples per tile (same HBM
    // bytes, same L2 hits and misses, 1.28 x the wave cycles: profiles/r06_tiles_pmc_S4.log), both measured and removed:
    // the NEXT item's tile record (bounds, sample count, arena offset) fetched before the current item starts -- 0.627 -> 0.632 of the
    // HBM peak at 4 samples, nothing above (profiles/r06_tiles_prefetch.log); the four waves of a workgroup TOGETHER on four adjacent
    // tiles, a band of four rows each (moments in 768-byte runs instead of 192-byte ones) -- 0.675 -> 0.648 at 4 samples, 0.720 -> 0.685
    // at 8, slower at every length (profiles/r06_tiles_quad.log).  Neither the latency of the record nor the shape of the accesses, then.
    for (long long item = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += n_waves) {
        int tile = __builtin_amdgcn_readfirstlane(a.order ? (int)(item % a.n_tiles) : (int)(item / a.n_types));
        int ti = __builtin_amdgcn_readfirstlane(a.order ? (int)(item / a.n_tiles) : (int)(item % a.n_types));
        if (a.order == 2) {
            const long long q = item >> 2;
            ti = __builtin_amdgcn_readfirstlane((int)(q % a.n_types));
            tile = __builtin_amdgcn_readfirstlane((int)(q / a.n_types) * 4 + (int)(item & 3));
            if (tile >= a.n_tiles) continue;
        }
        const int x0 = a.tile_bounds[4 * tile], y0 = a.tile_bounds[4 * tile + 1];
        const int x1 = a.tile_bounds[4 * tile + 2], y1 = a.tile_bounds[4 * tile + 3];
        const int S = a.tile_samples[tile];
        if (S <= 0 || x1 <= x0 || y1 <= y0) continue;
        const AccumulateType &t = a.t[ti];
        acc_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
            accumulate_tile<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, UMUL, DMA>(t, a, a.vec != 0, x0, y0, x1 - x0, y1 - y0, a.tile_offsets[tile], S, ring);
        });
    }
}

// Launches in which at least one type's arena is IEEE half (statmc_accumulate_tiles_formats; a.half_mask: bit i = type i): a
// kernel of its own, so that accumulate_tiles_kernel stays the code object it was.  The format of an item's type is a
// wave-uniform choice in front of the type dispatch.  A half type's rows come through the half loaders of accumulate_lane /
// accumulate_pixel and widen exactly, so the fold sees what it would see had the caller widened the arena.  DMA > 0: the RGB
// rows of the launch, fp32 and half, arrive by LDS-DMA in the wave's ring (a half slot holds two samples: accumulate_lane);
// DMA = 0 (statmc_debug_accumulate_dma(0)): every row by register loads, 8-byte pieces for half.  The vector path is a type's own here (a.vec: bit i = type i), since a half arena asks for 8-byte alignment only.
template <int UMUL, int DMA>
__global__ __launch_bounds__(kBlock) void accumulate_tiles_half_kernel(AccumulateTilesArgs a) {
    extern __shared__ __attribute__((aligned(16))) float acc_lds[];
    float *ring = DMA ? acc_lds + (threadIdx.x >> 6) * acc_ring_floats(DMA) : nullptr;
    // (the item walk of accumulate_tiles_kernel, a.order as there: its own copy -- handing both kernels one function for it
    // changes the fp32 kernels' code, 23 511 -> 23 287 instructions without the ring, 18 398 -> 18 181 with it)
    const long long n_items = a.order == 2 ? (((long long)a.n_tiles + 3) >> 2) * 4 * a.n_types : (long long)a.n_tiles * a.n_types;
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    for (long long item = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += n_waves) {
        int tile = __builtin_amdgcn_readfirstlane(a.order ? (int)(item % a.n_tiles) : (int)(item / a.n_types));
        int ti = __builtin_amdgcn_readfirstlane(a.order ? (int)(item / a.n_tiles) : (int)(item % a.n_types));
        if (a.order == 2) {
            const long long q = item >> 2;
            ti = __builtin_amdgcn_readfirstlane((int)(q % a.n_types));
            tile = __builtin_amdgcn_readfirstlane((int)(q / a.n_types) * 4 + (int)(item & 3));
            if (tile >= a.n_tiles) continue;
        }
        const int x0 = a.tile_bounds[4 * tile], y0 = a.tile_bounds[4 * tile + 1];
        const int x1 = a.tile_bounds[4 * tile + 2], y1 = a.tile_bounds[4 * tile + 3];
        const int S = a.tile_samples[tile];
        if (S <= 0 || x1 <= x0 || y1 <= y0) continue;
        const AccumulateType &t = a.t[ti];
        const bool vec = (a.vec >> ti) & 1;
        if ((a.half_mask >> ti) & 1) {
            acc_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
                accumulate_tile<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, UMUL, DMA, _Float16>(t, a, vec, x0, y0, x1 - x0, y1 - y0, a.tile_offsets[tile], S, ring);
            });
        } else {
            acc_dispatch_type(t, [&](auto c, auto maxm, auto transform) {
                accumulate_tile<decltype(c)::value, decltype(maxm)::value, decltype(transform)::value, UMUL, DMA>(t, a, vec, x0, y0, x1 - x0, y1 - y0, a.tile_offsets[tile], S, ring);
            });
        }
    }
}

hipError_t launch_accumulate_tiles(const AccumulateTilesArgs &a_in, hipStream_t s) {
    AccumulateTilesArgs a = a_in;
    int vec_mask = 0;
    for (int i = 0; i < a.n_types; i++)
        if (acc_type_vectorizable(a.t[i], (a.half_mask >> i) & 1, false)) vec_mask |= 1 << i;
    // fp32 launches: all types or none (the ring is the launch's); the half kernel: a bit per type
    a.vec = a.half_mask != 0 ? vec_mask : vec_mask == (1 << a.n_types) - 1 ? 1 : 0;
    const long long items = a.order == 2 ? (((long long)a.n_tiles + 3) >> 2) * 4 * a.n_types : (long long)a.n_tiles * a.n_types;
    // one wave per item; films up to ~ 4 Mpixels: at most 8 workgroups per CU, walking the items with a grid stride; larger ones
    // (4K: 32 400 tiles): every wave ONE item, the dispatcher hands the workgroups out -- + 1 - 4 % at 4 .. 64 samples per tile there,
    // - 1 - 2 % at 1080p (profiles/r05_tiles_first.log; the film-major launch has the same rule, plan_accumulate)
    const bool big = a.n_tiles >= 16384;
    const int grid = grid_for(items * 64, a.wg_per_cu > 0 ? 256 * a.wg_per_cu : big ? (1 << 30) : 256 * 8);
    if (a.half_mask != 0) {   // (the ring serves the launch's RGB types, fp32 and half; a launch without one asks for no LDS)
        bool rgb = false;
        for (int i = 0; i < a.n_types; i++) rgb = rgb || a.t[i].channels == 3;
        if (!rgb) a.dma = 0;
        if (a.dma && a.umul == 2) hipLaunchKernelGGL((accumulate_tiles_half_kernel<2, kAccTilesDmaD>), dim3(grid), dim3(kBlock), acc_lds_bytes(kAccTilesDmaD), s, a);
        else if (a.dma) hipLaunchKernelGGL((accumulate_tiles_half_kernel<1, kAccTilesDmaD>), dim3(grid), dim3(kBlock), acc_lds_bytes(kAccTilesDmaD), s, a);
        else if (a.umul == 2) hipLaunchKernelGGL((accumulate_tiles_half_kernel<2, 0>), dim3(grid), dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((accumulate_tiles_half_kernel<1, 0>), dim3(grid), dim3(kBlock), 0, s, a);
        return hipGetLastError();
    }
    // (the DMA walk needs the vector path: a.vec; the scalar path of unaligned images never touches the ring)
    if (a.vec && a.dma && a.umul == 2) hipLaunchKernelGGL((accumulate_tiles_kernel<2, kAccTilesDmaD>), dim3(grid), dim3(kBlock), acc_lds_bytes(kAccTilesDmaD), s, a);
    else if (a.vec && a.dma) hipLaunchKernelGGL((accumulate_tiles_kernel<1, kAccTilesDmaD>), dim3(grid), dim3(kBlock), acc_lds_bytes(kAccTilesDmaD), s, a);
    else if (a.umul == 2) hipLaunchKernelGGL((accumulate_tiles_kernel<2, 0>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((accumulate_tiles_kernel<1, 0>), dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ merge tiles
// AoS StatTilePixel<T> (estimator.h:104-124): uint64 n at byte 0, then mean, m2, m3, filmMean,
// filmM2 (T each) from byte 8; sizeof = 64 (T = float) / 128 (T = Vec3).
template <int C>
__global__ __launch_bounds__(kBlock) void merge_tiles_kernel(MergeTilesArgs a) {
    const int t = blockIdx.y;
    const int x0 = a.tile_bounds[4 * t], y0 = a.tile_bounds[4 * t + 1];
    const int x1 = a.tile_bounds[4 * t + 2], y1 = a.tile_bounds[4 * t + 3];
    const int tw = x1 - x0, npx = tw * (y1 - y0);
    constexpr int kStride = C == 1 ? 64 : 128;
    const unsigned char *base = static_cast<const unsigned char *>(a.tile_pixels) + a.tile_offsets[t] * kStride;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < npx; i += gridDim.x * kBlock) {
        const int x = x0 + i % tw, y = y0 + i / tw;  // estimator.h:44-48
        if (x >= a.width || y >= a.height) continue;
        const long long off = (long long)y * a.width + x;
        const unsigned char *px = base + (long long)i * kStride;
        const unsigned long long cnt = *reinterpret_cast<const unsigned long long *>(px);
        const float *f = reinterpret_cast<const float *>(px + 8);
        a.n[off] = (int32_t)cnt;
#pragma unroll
        for (int c = 0; c < C; c++) {
            a.mean[off * C + c] = f[c];
            a.m2[off * C + c] = f[C + c];
            a.m3[off * C + c] = f[2 * C + c];
            if (a.transform) {  // MergeTransformTile only (estimator.cpp:385-386)
                a.film_mean[off * C + c] = f[3 * C + c];
                a.film_m2[off * C + c] = f[4 * C + c];
            }
        }
    }
}

hipError_t launch_merge_tiles(const MergeTilesArgs &a, int n_tiles, int max_tile_pixels, hipStream_t s) {
    const dim3 grid((max_tile_pixels + kBlock - 1) / kBlock, n_tiles);
    if (a.channels == 3)
        hipLaunchKernelGGL(merge_tiles_kernel<3>, grid, dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL(merge_tiles_kernel<1>, grid, dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ film update
// One lane per Film::Pixel (32 B AoS = two 16-B loads), interleaved RGB out.  film.cpp:188-222.
__device__ __forceinline__ void xyz_to_rgb(const float xyz[3], float rgb[3]) {  // spectrum.h:66-70
    rgb[0] = 3.240479f * xyz[0] - 1.537150f * xyz[1] - 0.498535f * xyz[2];
    rgb[1] = -0.969256f * xyz[0] + 1.875991f * xyz[1] + 0.041556f * xyz[2];
    rgb[2] = 0.055648f * xyz[0] - 0.204043f * xyz[1] + 1.057311f * xyz[2];
}

__global__ __launch_bounds__(kBlock) void film_update_kernel(const float4 *pixels, long long n, float splat_scale,
                                                             float scale, float *rgb_out) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const float4 a = pixels[2 * i], b = pixels[2 * i + 1];  // {xyz, weight}, {splat xyz, pad}
        const float xyz[3] = {a.x, a.y, a.z}, sxyz[3] = {b.x, b.y, b.z};
        float o[3], s[3];
        xyz_to_rgb(xyz, o);
        if (a.w != 0.f) {
            const float inv = 1.f / a.w;
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = __builtin_fmaxf(0.f, o[c] * inv);
        }
        xyz_to_rgb(sxyz, s);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            o[c] += splat_scale * s[c];
            o[c] *= scale;
            rgb_out[3 * i + c] = o[c];
        }
    }
}

hipError_t launch_film_update(const void *pixels, long long n, float splat_scale, float scale, float *rgb, hipStream_t s) {
    hipLaunchKernelGGL(film_update_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, static_cast<const float4 *>(pixels), n,
                       splat_scale, scale, rgb);
    return hipGetLastError();
}

// ------------------------------------------------------------------ tile moments
// One wavefront per (tile, channel): each lane folds its share of the tile's pixels with
// Welford's update, then the 64 partial (count, mean, M2) triples are merged pairwise with
// Chan's formula through wave shuffles.
__device__ __forceinline__ void chan_merge(float &na, float &ma, float &sa, float nb, float mb, float sb) {
    const float n = na + nb;
    if (n > 0.f) {
        const float d = mb - ma;
        const float f = nb / n;
        ma = ma + d * f;
        sa = sa + sb + d * d * na * f;
        na = n;
    }
}

__global__ __launch_bounds__(64) void tile_moments_kernel(TileMomentsArgs a) {
    const int tx = blockIdx.x, ty = blockIdx.y, c = blockIdx.z;
    const int lane = threadIdx.x;
    const int ts = a.tile_size, tpx = ts * ts;
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int i = lane; i < tpx; i += 64) {
        const int x = tx * ts + i % ts, y = ty * ts + i / ts;
        if (x < a.width && y < a.height) {
            const float v = a.values[((long long)y * a.width + x) * a.channels + c];
            cnt += 1.f;
            const float d = v - mean;
            mean += d / cnt;
            m2 += d * (v - mean);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float nb = __shfl_xor(cnt, off, 64), mb = __shfl_xor(mean, off, 64), sb = __shfl_xor(m2, off, 64);
        chan_merge(cnt, mean, m2, nb, mb, sb);
    }
    if (lane == 0) {
        float *o = a.out + (((long long)ty * a.tiles_x + tx) * a.channels + c) * 3;
        o[0] = cnt;
        o[1] = mean;
        o[2] = m2;
    }
}

hipError_t launch_tile_moments(const TileMomentsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(tile_moments_kernel, dim3(a.tiles_x, a.tiles_y, a.channels), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ combine
// Two independently accumulated states of the same pixels -> the state of the union of their samples (Chan et al. 1979,
// Pebay 2008); part A is dst, part B src.  The fp32 operation order, per element, is the one stated in include/statmc.h
// (statmc_combine_statistics).  One lane owns 4 consecutive pixels, as in the accumulation, and runs every entry of the
// call over them in entry order: the ABI puts the entries that borrow counts first, so they read the counts before the
// owning entry -- later in the same lane -- writes n = nA + nB.  HBM-bound: C float4 per plane and one int4 of counts per
// lane when every plane is 16-byte aligned (the last, partial group and unaligned planes take the scalar path).
template <int C, bool VEC>
__device__ __forceinline__ void comb_load(const float *p, long long px0, int npx, float (&v)[4 * C]) {
    if (VEC) {
#pragma unroll
        for (int k = 0; k < C; k++) {
            const float4 x = reinterpret_cast<const float4 *>(p + px0 * C)[k];
            v[4 * k] = x.x;
            v[4 * k + 1] = x.y;
            v[4 * k + 2] = x.z;
            v[4 * k + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * C; j++) v[j] = j < npx * C ? p[px0 * C + j] : 0.f;
    }
}
template <int C, bool VEC>
__device__ __forceinline__ void comb_store(float *p, long long px0, int npx, const float (&v)[4 * C]) {
    if (VEC) {
#pragma unroll
        for (int k = 0; k < C; k++)
            reinterpret_cast<float4 *>(p + px0 * C)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4 * C; j++)
            if (j < npx * C) p[px0 * C + j] = v[j];
    }
}
template <bool VEC>
__device__ __forceinline__ void comb_load_n(const int32_t *p, long long px0, int npx, int (&v)[4]) {
    if (VEC) {
        const int4 x = *reinterpret_cast<const int4 *>(p + px0);
        v[0] = x.x;
        v[1] = x.y;
        v[2] = x.z;
        v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = j < npx ? p[px0 + j] : 0;
    }
}

// (combine_counts, combine_mean_m2, combine_m3: include/statmc_device_api.hpp -- the per-element arithmetic, the definition a
// renderer's own kernel merges with as well)

// mean (and m2) of one chain: the mean / m2 lines of the formula.  qt and u (u only with WANT_U) are kept for m3.
template <int C, bool VEC, bool M2, bool WANT_U>
__device__ __forceinline__ void comb_chain(float *dm, const float *sm, float *dm2, const float *sm2, long long px0, int npx,
                                           const CombineCounts (&w)[4], float (&mA)[4 * C], float (&m2A)[4 * C], float (&m2B)[4 * C],
                                           float (&qt)[4 * C], float (&u)[4 * C]) {
    float mB[4 * C], o[4 * C];
    comb_load<C, VEC>(dm, px0, npx, mA);
    comb_load<C, VEC>(sm, px0, npx, mB);
    if (M2) {
        comb_load<C, VEC>(dm2, px0, npx, m2A);
        comb_load<C, VEC>(sm2, px0, npx, m2B);
    }
#pragma unroll
    for (int j = 0; j < 4 * C; j++)
        device::combine_mean_m2<M2, WANT_U>(w[j / C], mA[j], mB[j], m2A[j], m2B[j], mA[j], o[j], qt[j], u[j]);
    comb_store<C, VEC>(dm, px0, npx, mA);
    if (M2) {
        comb_store<C, VEC>(dm2, px0, npx, o);
        if (!WANT_U) {   // no m3 to come: the combined m2 is what the caller keeps
#pragma unroll
            for (int j = 0; j < 4 * C; j++) m2A[j] = o[j];
        }
    }
}

template <int C, bool VEC>
__device__ __forceinline__ void combine_entry(const CombineEntry &e, long long px0, int npx) {
    int nA[4], nB[4];
    comb_load_n<VEC>(e.cnt_dst, px0, npx, nA);
    comb_load_n<VEC>(e.cnt_src, px0, npx, nB);
    CombineCounts w[4];
#pragma unroll
    for (int p = 0; p < 4; p++) w[p] = device::combine_counts(nA[p], nB[p]);
    float mA[4 * C], m2A[4 * C], m2B[4 * C], qt[4 * C], u[4 * C];
    if (e.d[kCombM3]) {
        comb_chain<C, VEC, true, true>(e.d[kCombMean], e.s[kCombMean], e.d[kCombM2], e.s[kCombM2], px0, npx, w, mA, m2A, m2B, qt, u);
        float m3A[4 * C], m3B[4 * C];
        comb_load<C, VEC>(e.d[kCombM3], px0, npx, m3A);
        comb_load<C, VEC>(e.s[kCombM3], px0, npx, m3B);
#pragma unroll
        for (int j = 0; j < 4 * C; j++) {
            const CombineCounts &wp = w[j / C];
            m3A[j] = device::combine_m3(wp, m2A[j], m2B[j], m3A[j], m3B[j], qt[j], u[j]);
            m2A[j] = device::combine_pick(wp, m2A[j], m2B[j], (m2A[j] + m2B[j]) + qt[j]);
        }
        comb_store<C, VEC>(e.d[kCombM3], px0, npx, m3A);
        if (e.mean_corr) {   // the pre-pass of the combined moments: prepass_kernel's prepass_elem, the same bits
            float mc[4 * C], dc[4 * C];
#pragma unroll
            for (int j = 0; j < 4 * C; j++) {
                const int p = j / C, ni = nA[p] + nB[p];
                prepass_elem(ni, prepass_quantile(e.pre_table, e.pre_flags, ni), mA[j], m2A[j], m3A[j], mc[j], dc[j],
                             (e.pre_flags & 2) != 0);
            }
            comb_store<C, VEC>(e.mean_corr, px0, npx, mc);
            comb_store<C, VEC>(e.disc, px0, npx, dc);
        }
    } else if (e.d[kCombM2]) {
        comb_chain<C, VEC, true, false>(e.d[kCombMean], e.s[kCombMean], e.d[kCombM2], e.s[kCombM2], px0, npx, w, mA, m2A, m2B, qt, u);
    } else {
        comb_chain<C, VEC, false, false>(e.d[kCombMean], e.s[kCombMean], nullptr, nullptr, px0, npx, w, mA, m2A, m2B, qt, u);
    }
    if (e.d[kCombFilmM2])
        comb_chain<C, VEC, true, false>(e.d[kCombFilmMean], e.s[kCombFilmMean], e.d[kCombFilmM2], e.s[kCombFilmM2], px0, npx, w, mA,
                                        m2A, m2B, qt, u);
    else if (e.d[kCombFilmMean])
        comb_chain<C, VEC, false, false>(e.d[kCombFilmMean], e.s[kCombFilmMean], nullptr, nullptr, px0, npx, w, mA, m2A, m2B, qt, u);
    if (e.write_n) {
        if (VEC) {
            *reinterpret_cast<int4 *>(e.cnt_dst + px0) = make_int4(nA[0] + nB[0], nA[1] + nB[1], nA[2] + nB[2], nA[3] + nB[3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < npx) e.cnt_dst[px0 + p] = nA[p] + nB[p];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void combine_stats_kernel(CombineArgs a) {
    const long long n_groups = (a.n_px + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n_groups; g += (long long)gridDim.x * kBlock) {
        const long long px0 = g << 2;
        const int npx = a.n_px - px0 < 4 ? (int)(a.n_px - px0) : 4;
        for (int i = 0; i < a.n_entries; i++) {
            const CombineEntry &e = a.e[i];
            if (VEC && npx == 4) {
                if (e.channels == 3) combine_entry<3, true>(e, px0, 4);
                else combine_entry<1, true>(e, px0, 4);
            } else {
                if (e.channels == 3) combine_entry<3, false>(e, px0, npx);
                else combine_entry<1, false>(e, px0, npx);
            }
        }
    }
}

hipError_t launch_combine(const CombineArgs &a, hipStream_t s) {
    const int grid = grid_for((a.n_px + 3) / 4);
    if (a.vec)
        hipLaunchKernelGGL(combine_stats_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL(combine_stats_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ combine, K parts
// statmc_combine_many: the left fold of n_sources combines, in one pass over memory.  One lane owns 4 consecutive pixels
// and walks the entries in the ABI's order (the entries that do not write counts first), as above; per entry it loads the
// dst planes and counts once, folds source after source in registers and stores once.  The source planes are read once and
// never again, but they are plain loads: with the nt bit the same kernel streamed at 0.59-0.62 of the HBM peak instead of
// 0.63-0.65.  The loads of the next sources are requested before the arithmetic on source k (a ring of
// register sets, the loop unrolled by its size), so a lane has whole sources in flight behind the one it works on.
typedef float cm_f32x4 __attribute__((ext_vector_type(4)));
typedef int cm_i32x4 __attribute__((ext_vector_type(4)));

template <int C, int M>
struct CombManySrc {
    int n[4];
    float v[M][4 * C];
};

template <int C, int M, bool VEC>
__device__ __forceinline__ void comb_many_load(const void *const *sp, long long px0, int npx, CombManySrc<C, M> &s) {
    const int32_t *cn = static_cast<const int32_t *>(sp[0]);
    if (VEC) {
        const cm_i32x4 x = *reinterpret_cast<const cm_i32x4 *>(cn + px0);   // counts: read again by the entries that share them
        s.n[0] = x.x;
        s.n[1] = x.y;
        s.n[2] = x.z;
        s.n[3] = x.w;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const cm_f32x4 *p = reinterpret_cast<const cm_f32x4 *>(static_cast<const float *>(sp[1 + m]) + px0 * C);
#pragma unroll
            for (int k = 0; k < C; k++) {
                const cm_f32x4 y = p[k];
                s.v[m][4 * k] = y.x;
                s.v[m][4 * k + 1] = y.y;
                s.v[m][4 * k + 2] = y.z;
                s.v[m][4 * k + 3] = y.w;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) s.n[j] = j < npx ? cn[px0 + j] : 0;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const float *p = static_cast<const float *>(sp[1 + m]) + px0 * C;
#pragma unroll
            for (int j = 0; j < 4 * C; j++) s.v[m][j] = j < npx * C ? p[j] : 0.f;
        }
    }
}

// source `s` (part B) into the running state (part A); nA becomes the running count
template <int C, int M>
__device__ __forceinline__ void comb_many_fold(int (&nA)[4], float (&A)[M][4 * C], const CombManySrc<C, M> &s) {
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const CombineCounts w = device::combine_counts(nA[p], s.n[p]);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int j = p * C + c;
            ElemState a, b;
            a.mean = A[0][j];
            b.mean = s.v[0][j];
            a.m2 = M >= 2 ? A[1][j] : 0.f;
            b.m2 = M >= 2 ? s.v[1][j] : 0.f;
            a.m3 = M >= 3 ? A[2][j] : 0.f;
            b.m3 = M >= 3 ? s.v[2][j] : 0.f;
            a.fmean = a.fm2 = b.fmean = b.fm2 = 0.f;
            device::combine_elem<M, 0>(a, b, w);
            A[0][j] = a.mean;
            if (M >= 2) A[1][j] = a.m2;
            if (M >= 3) A[2][j] = a.m3;
        }
        nA[p] += s.n[p];
    }
}

template <int C, int M, bool VEC>
__device__ __forceinline__ void combine_many_entry(const CombineManyEntry &e, const void *const *src, int n_sources, long long px0,
                                                   int npx) {
    // D register sets: D - 1 sources in flight behind the one being folded.  A chain of one plane moves 64 B per lane and
    // source, too little to keep a CU's share of HBM busy from one request: the fewer planes, the deeper the ring.
    constexpr int D = M == 1 ? 4 : M == 2 ? 3 : 2;
    CombManySrc<C, M> s[D];
    int nA[4];
    float A[M][4 * C];
    comb_load_n<VEC>(e.cnt_dst, px0, npx, nA);
#pragma unroll
    for (int m = 0; m < M; m++) comb_load<C, VEC>(e.d[m], px0, npx, A[m]);
#pragma unroll
    for (int j = 0; j < D - 1; j++)
        if (j < n_sources) comb_many_load<C, M, VEC>(src + j * kCombManySrcPtrs, px0, npx, s[j]);
    // The steady state has no branch between a request and the fold before it: the wait in front of a fold then counts the
    // loads requested after the ones it needs and leaves them in flight (a conditional request makes it a wait for all).
    int k = 0;
    for (; k + 2 * D - 1 <= n_sources; k += D) {
#pragma unroll
        for (int j = 0; j < D; j++) {
            comb_many_load<C, M, VEC>(src + (k + j + D - 1) * kCombManySrcPtrs, px0, npx, s[(j + D - 1) % D]);
            comb_many_fold<C, M>(nA, A, s[j]);
        }
    }
    // the last sources, fewer than 2 D - 1: k .. k + D - 2 are requested already
#pragma unroll
    for (int j = 0; j < 2 * D - 2; j++) {
        if (k + j < n_sources) {
            if (k + j + D - 1 < n_sources)
                comb_many_load<C, M, VEC>(src + (k + j + D - 1) * kCombManySrcPtrs, px0, npx, s[(j + D - 1) % D]);
            comb_many_fold<C, M>(nA, A, s[j % D]);
        }
    }
#pragma unroll
    for (int m = 0; m < M; m++) comb_store<C, VEC>(e.d[m], px0, npx, A[m]);
    if (M == 3 && e.mean_corr) {   // the pre-pass of the final moments: prepass_kernel's prepass_elem, the same bits
        const int table = e.pre & 255, flags = e.pre >> 8;
        float mc[4 * C], dc[4 * C];
#pragma unroll
        for (int j = 0; j < 4 * C; j++) {
            const int ni = nA[j / C];
            prepass_elem(ni, prepass_quantile(table, flags, ni), A[0][j], A[M >= 2 ? 1 : 0][j], A[M >= 3 ? 2 : 0][j], mc[j],
                         dc[j], (flags & 2) != 0);
        }
        comb_store<C, VEC>(e.mean_corr, px0, npx, mc);
        comb_store<C, VEC>(e.disc, px0, npx, dc);
    }
    if (e.write_n) {
        if (VEC) {
            *reinterpret_cast<int4 *>(e.cnt_dst + px0) = make_int4(nA[0], nA[1], nA[2], nA[3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < npx) e.cnt_dst[px0 + p] = nA[p];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void combine_many_dispatch(const CombineManyEntry &e, const void *const *src, int n_sources, long long px0,
                                                      int npx) {
    if (e.channels == 3) {
        if (e.moments == 3) combine_many_entry<3, 3, VEC>(e, src, n_sources, px0, npx);
        else if (e.moments == 2) combine_many_entry<3, 2, VEC>(e, src, n_sources, px0, npx);
        else combine_many_entry<3, 1, VEC>(e, src, n_sources, px0, npx);
    } else {
        if (e.moments == 3) combine_many_entry<1, 3, VEC>(e, src, n_sources, px0, npx);
        else if (e.moments == 2) combine_many_entry<1, 2, VEC>(e, src, n_sources, px0, npx);
        else combine_many_entry<1, 1, VEC>(e, src, n_sources, px0, npx);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void combine_many_kernel(CombineManyArgs a) {
    const long long n_groups = (a.n_px + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n_groups; g += (long long)gridDim.x * kBlock) {
        const long long px0 = g << 2;
        const int npx = a.n_px - px0 < 4 ? (int)(a.n_px - px0) : 4;
        for (int i = 0; i < a.n_entries; i++) {
            const CombineManyEntry e = a.e[i];   // a copy, not a reference into the by-value argument
            const void *const *src = a.src + (long long)i * a.n_sources * kCombManySrcPtrs;
            if (VEC && npx == 4) combine_many_dispatch<true>(e, src, a.n_sources, px0, 4);
            else combine_many_dispatch<false>(e, src, a.n_sources, px0, npx);
        }
    }
}

hipError_t launch_combine_many(const CombineManyArgs &a, hipStream_t s) {
    const int grid = grid_for((a.n_px + 3) / 4);
    if (a.vec)
        hipLaunchKernelGGL(combine_many_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL(combine_many_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc
