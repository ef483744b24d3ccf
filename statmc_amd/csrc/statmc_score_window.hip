// statmc_score_window.hip -- statmc_score_window (include/statmc.h): the maximum or minimum of a score image's keys over a square
// window, on the device, in one launch.  DESIGN.md 4.2f.
//
// A workgroup owns a kWindowTile x kWindowTile tile of outputs (statmc_score_window_args.h):
//   1. stage: the tile and its halo of `radius` keys to every side go to LDS array A as keys (select_key), taps outside the film
//      as the identity of the operation (0 for MAX, 0xFFFFFFFF for MIN);
//   2. row pass: along every row of A, window_double leaves M_w[i] = op(k[i .. i + w - 1]) for the largest power of two w <= 2 r + 1,
//      and op(M_w[i], M_w[i + 2 r + 1 - w]) -- two overlapping halves, exact because op is idempotent -- goes to array B,
//      transposed: B's rows are the tile's columns;
//   3. column pass: the same two steps along B's rows, the last one straight into `out`.
// window_double is the doubling scheme, in place: level w turns M_w into M_2w[i] = op(M_w[i], M_w[i + w]), log2(2 r + 1) levels of
// two reads and one write per key.  A wave owns whole rows and reads all of a row's operands before it writes any, so no level needs
// a second array; a barrier separates the levels.  Every LDS access is one dword with the lanes on consecutive addresses, or -- the
// transposed write and the last read -- on addresses multiples of an odd pitch apart: 32 lanes on 32 banks for the write, at most
// two on a bank for the read.
// Maxima and minima of integers: no order of evaluation reaches a bit.
#include "statmc_device.h"
#include "statmc_score_window_args.h"

namespace statmc {

namespace {

constexpr int kWindowWaves = kWindowBlock / 64;
constexpr int kWindowRowChunks = 2;              // a row of either array is at most 2 x 64 keys (statmc_score_window_args.h)
constexpr int kWindowRowsPerStep = 2;            // rows a wave has in flight
constexpr int kWindowOutQuads = kWindowTile / kWindowQuad + 1;   // aligned quads of the film's linear index that touch a tile's row

template <int OP>
__device__ __forceinline__ uint32_t window_op(uint32_t a, uint32_t b) {
    return OP == STATMC_SCORE_WINDOW_MIN ? (a < b ? a : b) : (a > b ? a : b);
}

// The doubling levels, in place, on `rows` rows of `len` keys at `pitch`; the whole workgroup calls this behind a barrier.  On
// return (behind a barrier again) m[i] = op over the w keys from i on, for every i with i + w <= len, w the largest power of two
// <= n; returns w.  Level w writes only the entries that stay meaningful, i + 2 w <= len: they read M_w[i] and M_w[i + w], both
// meaningful.  A lane reads both operands of all its entries of a row, then writes: the entries it overwrites are other lanes'
// operands of the same level, and a wave's LDS accesses run in program order.
template <int OP>
__device__ __forceinline__ int window_double(uint32_t *m, int rows, int len, int pitch, int n) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int w = 1;
    for (; 2 * w <= n; w *= 2) {
        for (int j0 = wave; j0 < rows; j0 += kWindowWaves * kWindowRowsPerStep) {
            uint32_t v[kWindowRowsPerStep][kWindowRowChunks];
            bool on[kWindowRowsPerStep][kWindowRowChunks];
#pragma unroll
            for (int u = 0; u < kWindowRowsPerStep; u++) {
                const int j = j0 + u * kWindowWaves;
                const uint32_t *row = m + j * pitch;
#pragma unroll
                for (int c = 0; c < kWindowRowChunks; c++) {
                    const int i = lane + 64 * c;
                    on[u][c] = j < rows && i + 2 * w <= len;
                    v[u][c] = on[u][c] ? window_op<OP>(row[i], row[i + w]) : 0u;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // every read of the step ahead of its writes
#pragma unroll
            for (int u = 0; u < kWindowRowsPerStep; u++) {
                uint32_t *row = m + (j0 + u * kWindowWaves) * pitch;
#pragma unroll
                for (int c = 0; c < kWindowRowChunks; c++)
                    if (on[u][c]) row[lane + 64 * c] = v[u][c];
            }
        }
        __syncthreads();
    }
    return w;
}

template <int OP>
__global__ __launch_bounds__(kWindowBlock) void score_window_kernel(ScoreWindowArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t window_lds[];
    const int r = a.radius, side = window_side(r), pitch_b = window_pitch_b(r), n = 2 * r + 1;
    uint32_t *A = window_lds;                    // [side][side]
    uint32_t *B = window_lds + side * side;      // [kWindowTile][pitch_b]
    const int x0 = (int)blockIdx.x * kWindowTile, y0 = (int)blockIdx.y * kWindowTile;
    const long long n_px = (long long)a.width * a.height;
    constexpr uint32_t ident = window_identity(OP);

    // 1. stage.  A row of A is `side` consecutive pixels of the film's linear index (the part inside the film), cut into the aligned
    // quads of that index: with a 16-byte aligned image a quad inside the film moves as one dwordx4 whatever the row's own alignment;
    // its pixels outside the row's span are dropped.  Every entry of A is written once, the taps outside the film as the identity.
    {
        const uint32_t *bits = reinterpret_cast<const uint32_t *>(a.score);
        const int quads = (side + 2 * (kWindowQuad - 1)) / kWindowQuad;   // that touch `side` pixels from any phase on
        for (int idx = (int)threadIdx.x; idx < side * quads; idx += kWindowBlock) {
            const int row = idx / quads, t = idx - row * quads;
            const int gy = y0 - r + row;
            const bool row_in = gy >= 0 && gy < a.height;
            const long long lin_lo = (long long)gy * a.width + (x0 - r);           // of A's column 0; outside the film it is only arithmetic
            const long long q0 = (lin_lo & ~(long long)(kWindowQuad - 1)) + kWindowQuad * t;
            const int c0 = (int)(q0 - lin_lo);                                     // A's column of the quad's first pixel, -3 at the least
            bool take[kWindowQuad];
            bool any = false;
#pragma unroll
            for (int e = 0; e < kWindowQuad; e++) {
                const int c = c0 + e, gx = x0 - r + c;
                take[e] = row_in && c >= 0 && c < side && gx >= 0 && gx < a.width;
                any = any || take[e];
            }
            uint32_t b[kWindowQuad] = {0u, 0u, 0u, 0u};
            if (any) {
                if (a.vec_in && q0 >= 0 && q0 + kWindowQuad <= n_px) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(bits + q0);
                    b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < kWindowQuad; e++)
                        if (take[e]) b[e] = bits[q0 + e];
                }
            }
#pragma unroll
            for (int e = 0; e < kWindowQuad; e++) {
                const int c = c0 + e;
                if (c >= 0 && c < side) A[row * side + c] = take[e] ? select_key(b[e]) : ident;
            }
        }
    }
    __syncthreads();

    // 2. the row pass: B[x][j] = op over A[j][x .. x + 2 r]
    const int w = window_double<OP>(A, side, side, side, n);
    for (int idx = (int)threadIdx.x; idx < side * kWindowTile; idx += kWindowBlock) {
        const int j = idx / kWindowTile, x = idx - j * kWindowTile;
        B[x * pitch_b + j] = window_op<OP>(A[j * side + x], A[j * side + x + n - w]);
    }
    __syncthreads();

    // 3. the column pass, and out: the tile's rows cut into aligned quads like the staged ones; a quad wholly inside the tile's row
    // moves as one dwordx4 with a 16-byte aligned out.
    window_double<OP>(B, kWindowTile, side, pitch_b, n);
    {
        uint32_t *out_bits = reinterpret_cast<uint32_t *>(a.out);
        const int tw = min(kWindowTile, a.width - x0), th = min(kWindowTile, a.height - y0);
        for (int idx = (int)threadIdx.x; idx < kWindowTile * kWindowOutQuads; idx += kWindowBlock) {
            const int j = idx / kWindowOutQuads, t = idx - j * kWindowOutQuads;
            if (j >= th) continue;
            const long long lin_lo = (long long)(y0 + j) * a.width + x0;
            const long long q0 = (lin_lo & ~(long long)(kWindowQuad - 1)) + kWindowQuad * t;
            const int c0 = (int)(q0 - lin_lo);
            uint32_t v[kWindowQuad];
            bool ok[kWindowQuad];
            bool all = true;
#pragma unroll
            for (int e = 0; e < kWindowQuad; e++) {
                const int c = c0 + e;
                ok[e] = c >= 0 && c < tw;
                all = all && ok[e];
                v[e] = ok[e] ? window_op<OP>(B[c * pitch_b + j], B[c * pitch_b + j + n - w]) : 0u;
            }
            if (all && a.vec_out) {
                *reinterpret_cast<uint4 *>(out_bits + q0) = make_uint4(v[0], v[1], v[2], v[3]);
                continue;
            }
            // (from the last pixel down: in ascending order the compiler folds this path's last store into the quad's, which then
            // leaves as a dwordx3 and a dword)
#pragma unroll
            for (int e = kWindowQuad - 1; e >= 0; e--)
                if (ok[e]) out_bits[q0 + e] = v[e];
        }
    }
}

}  // namespace

hipError_t launch_score_window(const ScoreWindowArgs &a, hipStream_t s) {
    const dim3 grid(a.tiles_x, a.tiles_y);
    if (a.op == STATMC_SCORE_WINDOW_MIN)
        hipLaunchKernelGGL(score_window_kernel<STATMC_SCORE_WINDOW_MIN>, grid, dim3(kWindowBlock), a.lds_bytes, s, a);
    else
        hipLaunchKernelGGL(score_window_kernel<STATMC_SCORE_WINDOW_MAX>, grid, dim3(kWindowBlock), a.lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace statmc
