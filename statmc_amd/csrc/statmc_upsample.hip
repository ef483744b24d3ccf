// statmc_upsample.hip -- statmc_upsample_filtered (include/statmc.h): the filtered image of a film pooled k x k, brought back onto
// the fine film by a statistics-gated joint upsampling.  Per fine pixel the four coarse pixels whose block centres surround it are
// weighed by a bilinear tent times the filter's own G-buffer range term, and take part only where they pass the filter's own
// membership test against the fine pixel.  DESIGN.md 4.2h.
//
// One launch per buffer streams the fine film once: mean_corr + discriminator + colour + G-buffers in, the filtered image out.  A lane
// owns four consecutive fine pixels; the coarse operands -- 1 / k^2 of the fine bytes, each read by the k x k to 2k x 2k fine pixels
// around it -- come through the cache, pixel by pixel.  No workspace, no LDS, no wait on another workgroup.
#include "statmc_device.h"
#include "statmc_upsample_args.h"

namespace statmc {

namespace {

__device__ __forceinline__ bool up_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool up_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

template <int C>
struct UpFine {
    float mc[C], disc[C], col[C];
    float g[kUpsampleMaxG][3];
};

// One fine pixel of the definition.  Every operation rounds once (no contraction); the fmaf are the oracle's (pair_member and the
// feature distance of oracle_filter_spec_run); `/` is the correctly rounded IEEE quotient; the exponential is the hardware's, exactly
// 1 at e == 0.
template <int C>
__device__ __forceinline__ void upsample_pixel(const UpsampleArgs &a, int x, int y, const UpFine<C> &f, float (&out)[C]) {
#pragma clang fp contract(off)
    bool valid = true;
#pragma unroll
    for (int c = 0; c < C; c++) valid &= up_finite(f.mc[c]) && !up_nan(f.disc[c]) && up_finite(f.col[c]);
#pragma unroll
    for (int g = 0; g < kUpsampleMaxG; g++)
        if (g < a.n_g) {
            valid &= up_finite(f.g[g][0]);
            if (a.gc[g] == 3) valid &= up_finite(f.g[g][1]) && up_finite(f.g[g][2]);
        }
    float sum_w = 0.f, acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.f;
    if (valid) {
        const int k = 1 << (a.shift - 1), mask = (1 << a.shift) - 1;
        const int tx = 2 * x + 1 - k, ty = 2 * y + 1 - k;
        const int X0 = tx >> a.shift, Y0 = ty >> a.shift;   // arithmetic shifts: the floor, -1 in the first half-block
        const int ax = tx & mask, ay = ty & mask;
        const float wx[2] = {(float)(mask + 1 - ax) * a.inv_2k, (float)ax * a.inv_2k};
        const float wy[2] = {(float)(mask + 1 - ay) * a.inv_2k, (float)ay * a.inv_2k};
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                int X = X0 + i, Y = Y0 + j;
                if (X < 0 || X >= a.wc || Y < 0 || Y >= a.hc) {
                    if (!a.clamp) continue;
                    X = min(max(X, 0), a.wc - 1), Y = min(max(Y, 0), a.hc - 1);
                }
                const long long q = (long long)Y * a.wc + X;
                float qmc[C], qd[C], qcol[C];
                bool qv = true;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    qmc[c] = a.c_mean_corr[q * C + c], qd[c] = a.c_disc[q * C + c], qcol[c] = a.c_colour[q * C + c];
                    qv &= up_finite(qmc[c]) && !up_nan(qd[c]) && up_finite(qcol[c]);
                }
                float e = 0.f;
#pragma unroll
                for (int g = 0; g < kUpsampleMaxG; g++)
                    if (g < a.n_g) {
                        const float *G = a.c_g[g];
                        float dist2;
                        if (a.gc[g] == 3) {
                            const float q0 = G[q * 3], q1 = G[q * 3 + 1], q2 = G[q * 3 + 2];
                            qv &= up_finite(q0) && up_finite(q1) && up_finite(q2);
                            const float d0 = f.g[g][0] - q0, d1 = f.g[g][1] - q1, d2 = f.g[g][2] - q2;
                            dist2 = d0 * d0;
                            dist2 = fmaf(d1, d1, dist2);
                            dist2 = fmaf(d2, d2, dist2);
                        } else {
                            const float q0 = G[q];
                            qv &= up_finite(q0);
                            const float d0 = f.g[g][0] - q0;
                            dist2 = d0 * d0;
                        }
                        e = fmaf(a.dr[g], dist2, e);
                    }
                // pair_member: p supplies D_p, Q supplies D_q
                bool all = true;
                float lhs_sum = 0.f, rhs_sum = 0.f;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float d = f.mc[c] - qmc[c];
                    const float Dp = f.disc[c], Dq = qd[c];
                    float lhs, rhs;
                    if (a.gate == STATMC_GATE_CENTRE) {
                        lhs = d * d, rhs = Dp;
                    } else if (a.gate == STATMC_GATE_ASYMMETRIC) {
                        lhs = fmaf(d, d, -Dq), rhs = Dp;
                    } else {
                        lhs = fmaf(d, d, -(Dp + Dq)), rhs = 0.f;
                    }
                    all &= lhs <= rhs;
                    lhs_sum = c == 0 ? lhs : lhs_sum + lhs;
                    rhs_sum = c == 0 ? rhs : rhs_sum + rhs;
                }
                const bool member = a.channel_rule == STATMC_CHANNELS_JOINT ? lhs_sum <= rhs_sum : all;
                if (!qv || !member) continue;
                const float w = (wx[i] * wy[j]) * __expf(e);
                sum_w = sum_w + w;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float t = w * qcol[c];
                    acc[c] = acc[c] + t;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) out[c] = sum_w > 0.f ? acc[c] / sum_w : f.col[c];
}

template <int CH>
__device__ __forceinline__ void up_load_quad_plane(const float *plane, long long p0, float (&t)[4 * CH]) {
#pragma unroll
    for (int i = 0; i < CH; i++) {
        const float4 v = reinterpret_cast<const float4 *>(plane + p0 * CH)[i];
        t[4 * i] = v.x, t[4 * i + 1] = v.y, t[4 * i + 2] = v.z, t[4 * i + 3] = v.w;
    }
}

// One lane per aligned quad of fine pixels of the flat film (a quad may straddle two rows).  A quad that lies inside the launch's range
// with all four pixels in the ROI moves as dwordx4 where every fine plane is 16-byte aligned (3 C + the G-buffers' channels loads, C
// stores); the ROI's edges, the film's last quad and unaligned planes go element by element through the same upsample_pixel.
template <int C>
__global__ __launch_bounds__(kUpsampleBlock) void upsample_kernel(UpsampleArgs a) {
    const long long p0 = a.p_begin + ((long long)blockIdx.x * kUpsampleBlock + threadIdx.x) * kUpsampleQuad;
    if (p0 >= a.p_end) return;
    const int y0 = (int)(p0 / a.width), x0 = (int)(p0 - (long long)y0 * a.width);
    const bool rows_whole = a.rx0 == 0 && a.rx1 == a.width;
    if (a.vec && rows_whole && y0 >= a.ry0 && p0 + kUpsampleQuad <= a.p_end) {
        float mc[4 * C], disc[4 * C], col[4 * C], g[kUpsampleMaxG][12] = {}, res[4 * C];
        up_load_quad_plane<C>(a.mean_corr, p0, mc);
        up_load_quad_plane<C>(a.disc, p0, disc);
        up_load_quad_plane<C>(a.colour, p0, col);
#pragma unroll
        for (int b = 0; b < kUpsampleMaxG; b++)
            if (b < a.n_g) {
                if (a.gc[b] == 3) {
                    up_load_quad_plane<3>(a.g[b], p0, g[b]);
                } else {
                    float t[4];
                    up_load_quad_plane<1>(a.g[b], p0, t);
#pragma unroll
                    for (int q = 0; q < 4; q++) g[b][3 * q] = t[q];
                }
            }
        int x = x0, y = y0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            UpFine<C> f;
#pragma unroll
            for (int c = 0; c < C; c++) f.mc[c] = mc[q * C + c], f.disc[c] = disc[q * C + c], f.col[c] = col[q * C + c];
#pragma unroll
            for (int b = 0; b < kUpsampleMaxG; b++)
#pragma unroll
                for (int c = 0; c < 3; c++) f.g[b][c] = g[b][3 * q + c];
            float o[C];
            upsample_pixel<C>(a, x, y, f, o);
#pragma unroll
            for (int c = 0; c < C; c++) res[q * C + c] = o[c];
            if (++x == a.width) x = 0, y++;
        }
#pragma unroll
        for (int i = 0; i < C; i++)
            reinterpret_cast<float4 *>(a.out + p0 * C)[i] = make_float4(res[4 * i], res[4 * i + 1], res[4 * i + 2], res[4 * i + 3]);
        return;
    }
    int x = x0, y = y0;
    for (long long p = p0; p < p0 + kUpsampleQuad && p < a.p_end; p++) {
        if (y >= a.ry0 && x >= a.rx0 && x < a.rx1) {
            UpFine<C> f;
#pragma unroll
            for (int c = 0; c < C; c++) f.mc[c] = a.mean_corr[p * C + c], f.disc[c] = a.disc[p * C + c], f.col[c] = a.colour[p * C + c];
#pragma unroll
            for (int b = 0; b < kUpsampleMaxG; b++) {
                f.g[b][0] = f.g[b][1] = f.g[b][2] = 0.f;
                if (b < a.n_g) {
                    if (a.gc[b] == 3) {
                        f.g[b][0] = a.g[b][p * 3], f.g[b][1] = a.g[b][p * 3 + 1], f.g[b][2] = a.g[b][p * 3 + 2];
                    } else {
                        f.g[b][0] = a.g[b][p];
                    }
                }
            }
            float o[C];
            upsample_pixel<C>(a, x, y, f, o);
#pragma unroll
            for (int c = 0; c < C; c++) a.out[p * C + c] = o[c];
        }
        if (++x == a.width) x = 0, y++;
    }
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)upsample_grid(a);
    if (a.channels == 3) hipLaunchKernelGGL(upsample_kernel<3>, dim3(grid), dim3(kUpsampleBlock), 0, s, a);
    else hipLaunchKernelGGL(upsample_kernel<1>, dim3(grid), dim3(kUpsampleBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace statmc
