// statmc_tile_select.hip -- statmc_score_tile_select and statmc_gate_tiles (include/statmc.h): per T x T tile of a score image up to
// four exact order statistics in one launch, and a per-tile decision brought back to the pixels.  DESIGN.md 4.2k.
//
// The select.  A tile belongs to a TEAM of lanes of one workgroup, as in statmc_score_tiles.hip: 16 lanes for T = 8 (four tiles per
// wave), a wave for T = 16, the workgroup for T = 32 and 64.  Nothing is shared between workgroups: no workspace, no global atomic.
//   - The loads are score_tiles_kernel's: a lane takes ALIGNED quads of the film's linear index that touch a row of its tile, as one
//     dwordx4 where the image is 16-byte aligned, element by element otherwise, and gives the elements of the neighbouring tiles the
//     key 0xFFFFFFFF, which no candidate exceeds: they are never counted.
//   - The keys stay in registers (kSlots quads per lane).  All ranks descend together over the 31 key bits: per bit a lane compares
//     its keys with the ranks' candidates and adds into 16-bit fields -- a tile has at most 4096 pixels --, two ranks to a 32-bit
//     word; the team adds the words up by shuffles, with T >= 32 the four waves' sums meet in LDS (two buffers, one barrier a bit).
//     A candidate with at most `rank` keys under it is kept; the last count kept is n_below, one more count gives n_equal.
// The gate.  A tile pass -- a lane per tile reads and writes closed[t] itself --, then a pixel pass over aligned quads.
#include "statmc_device.h"
#include "statmc_tile_select_args.h"

namespace statmc {

namespace {

constexpr int kTileSelectBlock = 256;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // an element outside the tile

template <int WIDTH>
__device__ __forceinline__ uint32_t team_add(uint32_t v) {
#pragma unroll
    for (int off = WIDTH / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, WIDTH);
    return v;
}

template <int T, int TEAM>
__global__ __launch_bounds__(kTileSelectBlock) void tile_select_kernel(TileSelectArgs a) {
    constexpr int kTeams = kTileSelectBlock / TEAM;   // tiles of a workgroup
    constexpr int kQuads = T / 4 + 1;                 // aligned quads that can touch a tile's row
    constexpr int kItems = T * kQuads;                // (row, quad) pairs of a tile
    constexpr int kSlots = (kItems + TEAM - 1) / TEAM;   // quads a lane holds
    constexpr int SUB = TEAM < 64 ? TEAM : 64;        // the lanes of a team that shuffles reach
    constexpr int kWaves = TEAM > 64 ? TEAM / 64 : 0; // 0: the team lies within a wave
    static_assert(kTileSelectBlock % TEAM == 0 && (SUB & (SUB - 1)) == 0, "teams tile the workgroup");
    static_assert(kWaves == 0 || kTeams == 1, "a team of several waves is the workgroup");
    __shared__ uint32_t meet[2][2][kWaves ? kWaves : 1];

    const int team = (int)threadIdx.x / TEAM, lane = (int)threadIdx.x % TEAM;
    const long long tile = (long long)blockIdx.x * kTeams + team;
    const bool live = tile < a.n_tiles;
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(a.score);
    const int tx = (int)(tile % a.tiles_x), ty = (int)(tile / a.tiles_x);
    const int x0 = tx * T, y0 = ty * T;
    const int x1 = x0 + T < a.width ? x0 + T : a.width, y1 = y0 + T < a.height ? y0 + T : a.height;

    uint32_t key[kSlots][4];
#pragma unroll
    for (int s = 0; s < kSlots; s++) {
#pragma unroll
        for (int q = 0; q < 4; q++) key[s][q] = kNoKey;
        const int item = lane + s * TEAM;
        const int y = y0 + item / kQuads;
        if (!live || item >= kItems || y >= y1) continue;
        const long long r0 = (long long)y * a.width + x0, r1 = (long long)y * a.width + x1;   // the row's pixels, r0 < r1 <= n_px
        const long long p0 = (r0 & ~3ll) + 4 * (item % kQuads);                                 // an aligned quad, p0 >= 0
        if (p0 >= r1) continue;
        uint32_t b[4];
        if (a.vec && p0 + 4 <= a.n_px) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bits + p0);
            b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) b[q] = p0 + q >= r0 && p0 + q < r1 ? bits[p0 + q] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) key[s][q] = p0 + q >= r0 && p0 + q < r1 ? select_key(b[q]) : kNoKey;
    }

    // the ranks of this tile: n from the grid's geometry
    const uint32_t n = live ? (uint32_t)((x1 - x0) * (y1 - y0)) : 1u;
    const bool wide = a.n_ranks > 2;   // the same for every lane
    uint32_t rank[4], prefix[4], below[4];
#pragma unroll
    for (int r = 0; r < 4; r++) rank[r] = tile_select_rank(n, a.q_num[r], a.q_den), prefix[r] = 0, below[r] = 0;

    // count(cand): per rank the number of the team's keys under cand[r] (equal to it with EQ), in 16-bit fields of lo and hi
    int step = 0;
    auto count = [&](const uint32_t (&cand)[4], bool eq, uint32_t &lo, uint32_t &hi) {
        lo = 0, hi = 0;
#pragma unroll
        for (int s = 0; s < kSlots; s++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t k = key[s][q];
                lo += (eq ? k == cand[0] : k < cand[0]) ? 1u : 0u;
                lo += (eq ? k == cand[1] : k < cand[1]) ? 0x10000u : 0u;
                if (wide) {
                    hi += (eq ? k == cand[2] : k < cand[2]) ? 1u : 0u;
                    hi += (eq ? k == cand[3] : k < cand[3]) ? 0x10000u : 0u;
                }
            }
        lo = team_add<SUB>(lo);
        if (wide) hi = team_add<SUB>(hi);
        if (kWaves) {   // a field holds at most 4096 here too: the tile's pixels
            const int buf = step & 1, wave = (int)(threadIdx.x >> 6);
            if ((threadIdx.x & 63) == 0) meet[buf][0][wave] = lo, meet[buf][1][wave] = hi;
            __syncthreads();   // the other buffer is written next: its readers are behind this barrier
            lo = 0, hi = 0;
#pragma unroll
            for (int w = 0; w < (kWaves ? kWaves : 1); w++) lo += meet[buf][0][w], hi += meet[buf][1][w];
            step++;
        }
    };

    for (int bit = 30; bit >= 0; bit--) {
        uint32_t cand[4], lo, hi;
#pragma unroll
        for (int r = 0; r < 4; r++) cand[r] = prefix[r] | (1u << bit);
        count(cand, false, lo, hi);
        const uint32_t c[4] = {lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu, hi >> 16};
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (c[r] <= rank[r]) prefix[r] = cand[r], below[r] = c[r];
    }
    uint32_t lo, hi;
    count(prefix, true, lo, hi);
    const uint32_t equal[4] = {lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu, hi >> 16};

    if (live) {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (lane == r && r < a.n_ranks) {   // a lane per rank; every index is a constant
                if (a.out.value[r]) reinterpret_cast<uint32_t *>(a.out.value[r])[tile] = prefix[r];
                if (a.out.n_below[r]) a.out.n_below[r][tile] = (int32_t)below[r];
                if (a.out.n_equal[r]) a.out.n_equal[r][tile] = (int32_t)equal[r];
            }
    }
}

template <int T, int TEAM>
void launch_select(const TileSelectArgs &a, hipStream_t s) {
    const long long n_groups = (a.n_tiles + kTileSelectBlock / TEAM - 1) / (kTileSelectBlock / TEAM);   // at most 2^26
    hipLaunchKernelGGL((tile_select_kernel<T, TEAM>), dim3((unsigned)n_groups), dim3(kTileSelectBlock), 0, s, a);
}

// ---------------------------------------------------------------- the gate
constexpr int kGateBlock = 256;

__device__ __forceinline__ long long gate_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// a lane per tile: closed[t] is read and written by that lane alone
__global__ __launch_bounds__(kGateBlock) void gate_tile_kernel(GateArgs a) {
    __shared__ long long part[kGateBlock / 64][3];
    const long long t = (long long)blockIdx.x * kGateBlock + threadIdx.x;
    long long n_open = 0, n_closed_now = 0, n_px_open = 0;
    if (t < a.n_tiles) {
        const bool was_closed = a.closed && a.closed[t] != 0;
        const bool above = select_key(reinterpret_cast<const uint32_t *>(a.tile_value)[t]) > a.threshold_key;
        const bool is_open = !was_closed && above;
        a.open[t] = is_open ? 1 : 0;
        if (a.closed && !was_closed) a.closed[t] = above ? 0 : 1;
        const int tx = (int)(t % a.tiles_x), ty = (int)(t / a.tiles_x);
        const int w = (tx + 1) * a.tile < a.width ? a.tile : a.width - tx * a.tile;
        const int h = (ty + 1) * a.tile < a.height ? a.tile : a.height - ty * a.tile;
        n_open = is_open, n_closed_now = !was_closed && !above, n_px_open = is_open ? w * h : 0;
    }
    if (!a.result) return;   // the same for every lane
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    n_open = gate_wave_sum(n_open), n_closed_now = gate_wave_sum(n_closed_now), n_px_open = gate_wave_sum(n_px_open);
    if (lane == 0) part[wave][0] = n_open, part[wave][1] = n_closed_now, part[wave][2] = n_px_open;
    __syncthreads();
    if (threadIdx.x < 3) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kGateBlock / 64; w++) v += part[w][threadIdx.x];
        int64_t *at = threadIdx.x == 0 ? &a.result->n_open : threadIdx.x == 1 ? &a.result->n_closed_now : &a.result->n_px_open;
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(at), (unsigned long long)v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 3) a.result->n_tiles = a.n_tiles;   // behind the zeroing on the stream
}

// a lane per aligned quad of the film's linear index, every image in the one pass; open[] comes through the cache
__global__ __launch_bounds__(kGateBlock) void gate_pixel_kernel(GateArgs a) {
    const long long p0 = ((long long)blockIdx.x * kGateBlock + threadIdx.x) * 4;
    if (p0 >= a.n_px) return;
    const uint32_t W = (uint32_t)a.width;
    uint32_t y = (uint32_t)((unsigned long long)p0 / W), x = (uint32_t)((unsigned long long)p0 - (unsigned long long)y * W);   // p0 < 2^32
    uint32_t keep[4];   // all ones: the pixel's tile is open
#pragma unroll
    for (int q = 0; q < 4; q++) {
        keep[q] = 0;
        if (p0 + q < a.n_px) {
            const long long t = (long long)(y >> a.tile_shift) * a.tiles_x + (x >> a.tile_shift);
            keep[q] = a.open[t] ? 0xFFFFFFFFu : 0u;
            if (++x == W) x = 0, y++;
        }
    }
    const bool full = p0 + 4 <= a.n_px;
#pragma unroll
    for (int i = 0; i < STATMC_GATE_MAX_IMAGES; i++) {
        if (i >= a.n_images) break;
        const uint32_t *src = a.src[i];
        uint32_t *dst = a.dst[i];
        if (a.vec && full) {
            uint4 v = *reinterpret_cast<const uint4 *>(src + p0);
            v.x &= keep[0], v.y &= keep[1], v.z &= keep[2], v.w &= keep[3];
            *reinterpret_cast<uint4 *>(dst + p0) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (p0 + q < a.n_px) dst[p0 + q] = src[p0 + q] & keep[q];
        }
    }
}

}  // namespace

// One launch: the kernel of the tile size.
hipError_t launch_tile_select(const TileSelectArgs &a, hipStream_t s) {
    switch (a.tile) {
    case 8: launch_select<8, 16>(a, s); break;
    case 16: launch_select<16, 64>(a, s); break;
    case 32: launch_select<32, 256>(a, s); break;
    case 64: launch_select<64, 256>(a, s); break;
    default: return hipErrorInvalidValue;   // check_tile_select_call lets no other through
    }
    return hipGetLastError();
}

// The result is zeroed on the stream; the tile pass, then the pixel pass, follow each other on it.
hipError_t launch_gate_tiles(const GateArgs &a, hipStream_t s) {
    if (a.result) {
        hipError_t e = hipMemsetAsync(a.result, 0, sizeof(statmc_gate_result), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gate_tile_kernel, dim3((unsigned)((a.n_tiles + kGateBlock - 1) / kGateBlock)), dim3(kGateBlock), 0, s, a);
    if (a.n_images > 0) {
        const long long quads = (a.n_px + 3) / 4;
        hipLaunchKernelGGL(gate_pixel_kernel, dim3((unsigned)((quads + kGateBlock - 1) / kGateBlock)), dim3(kGateBlock), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace statmc
