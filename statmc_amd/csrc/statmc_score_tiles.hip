// statmc_score_tiles.hip -- statmc_score_tiles (include/statmc.h): per T x T tile of a score image the exact sum, sum of squares and
// mean under a cap, the class counts and the maximum key, in one launch.  DESIGN.md 4.2j.
//
// A tile belongs to a TEAM of lanes of one workgroup: 16 lanes for T = 8 (four tiles per wave), a wave for T = 16, the workgroup for
// T = 32 and 64.  Nothing is shared between workgroups: no workspace, no global atomic.
//   - The loads.  Row y of a tile is the pixels [y W + x0, y W + x1) of the film's linear index; a lane takes one ALIGNED quad of that
//     index -- T / 4 + 1 of them can touch a row -- as one dwordx4 where the image is 16-byte aligned, and masks the elements that
//     belong to the neighbouring tiles.  Element by element otherwise, to the same bits.
//   - The accumulation is score_sum_pass_kernel's (statmc_score_sum.hip) with one cap: a lane's run of like (s >> 4) bands stays in
//     five 64-bit registers; a finished run goes to the team's limb table in LDS through 64-bit LDS atomics; a team whose lanes all
//     end in one band (a converged tile) adds them up by shuffles first.  A pixel above the cap only counts.
//   - The finalisation (statmc_score_tiles_args.h), after the table is complete: the sum, the sum of squares and the mean go to three
//     lanes that run ONE body on their own limbs in LDS -- the carries and the capped pixels' product (tile_capped_limbs) -- and part
//     only for the rounding to a double or the division to a float.  With T = 32 / 64 the three are lane 0 of three waves.  A NULL
//     plane's lane does nothing.
#include "statmc_device.h"
#include "statmc_score_tiles_args.h"

namespace statmc {

namespace {

constexpr int kTilesBlock = 256;
constexpr int kTilesMaxGrid = 2048;   // workgroups: they stride over the groups of tiles
enum { kTileCountZero = 0, kTileCountInfinite, kTileCountClipped, kTileMaxKey, kTileCounters };

template <int WIDTH>
__device__ __forceinline__ unsigned long long team_sum(unsigned long long v) {
#pragma unroll
    for (int off = WIDTH / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, WIDTH);
    return v;
}
template <int WIDTH>
__device__ __forceinline__ uint32_t team_sum(uint32_t v) {
#pragma unroll
    for (int off = WIDTH / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, WIDTH);
    return v;
}
template <int WIDTH>
__device__ __forceinline__ uint32_t team_max(uint32_t v) {
#pragma unroll
    for (int off = WIDTH / 2; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, WIDTH);
        v = o > v ? o : v;
    }
    return v;
}

// A lane's run: band = s >> 4, -1 none.  It fixes the limbs: the sum's are (s >> 5), + 1; the square's (s >> 4), + 1, + 2.
struct TileRun {
    int band;
    unsigned long long lo, hi, q0, q1, q2;   // a pixel adds less than 2^32 to each, a tile has at most 2^12 pixels
};

__device__ __forceinline__ void tile_flush(unsigned long long *table, const TileRun &r) {
    if (r.band < 0) return;
    unsigned long long *sum = table + (r.band >> 1), *sq = table + kSumLimbs + r.band;
    if (r.lo) atomicAdd(sum, r.lo);
    if (r.hi) atomicAdd(sum + 1, r.hi);
    if (r.q0) atomicAdd(sq, r.q0);
    if (r.q1) atomicAdd(sq + 1, r.q1);
    if (r.q2) atomicAdd(sq + 2, r.q2);
}

template <int T, int TEAM>
__global__ __launch_bounds__(kTilesBlock) void score_tiles_kernel(TilesArgs a) {
    constexpr int kTeams = kTilesBlock / TEAM;        // tiles of a workgroup's step
    constexpr int kQuads = T / 4 + 1;                 // aligned quads that can touch a tile's row
    constexpr int kItems = T * kQuads;                // (row, quad) pairs of a tile
    constexpr int SUB = TEAM < 64 ? TEAM : 64;        // the lanes of a team that shuffles reach
    static_assert(kTilesBlock % TEAM == 0 && (SUB & (SUB - 1)) == 0 && TEAM >= 4, "teams tile the workgroup; a team has a lane per role");
    __shared__ unsigned long long table[kTeams][kTileAccWords];
    __shared__ uint32_t counter[kTeams][kTileCounters];
    __shared__ uint32_t limbs[kTeams][3][kTileLimbs + 1];

    const int team = (int)threadIdx.x / TEAM, lane = (int)threadIdx.x % TEAM;
    const int wave_lane = (int)(threadIdx.x & 63);
    const long long n_groups = (a.n_tiles + kTeams - 1) / kTeams;
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(a.score);
    const uint32_t ck = a.cap_key;

    for (long long group = blockIdx.x; group < n_groups; group += gridDim.x) {   // the same trips for every lane of the workgroup
        const long long tile = group * kTeams + team;
        const bool live = tile < a.n_tiles;
        for (int i = lane; i < kTileAccWords; i += TEAM) table[team][i] = 0;
        if (lane < kTileCounters) counter[team][lane] = 0;
        __syncthreads();

        const int tx = (int)(tile % a.tiles_x), ty = (int)(tile / a.tiles_x);
        const int x0 = tx * T, y0 = ty * T;
        const int x1 = x0 + T < a.width ? x0 + T : a.width, y1 = y0 + T < a.height ? y0 + T : a.height;

        uint32_t n_zero = 0, n_infinite = 0, n_clipped = 0, max_key = 0;
        TileRun run = {-1, 0, 0, 0, 0, 0};
        for (int item = lane; item < kItems; item += TEAM) {
            const int y = y0 + item / kQuads;
            if (!live || y >= y1) continue;
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
            for (int q = 0; q < 4; q++) {
                const bool inside = p0 + q >= r0 && p0 + q < r1;
                const uint32_t k = inside ? select_key(b[q]) : 0u;
                n_zero += inside && k == 0;
                n_infinite += k == kSumInfinite;
                n_clipped += k > ck;
                max_key = k > max_key ? k : max_key;
                if (k != 0 && k <= ck && k < kSumInfinite) {
                    const uint32_t M = sum_significand(k);
                    const int s = sum_shift(k);
                    if ((s >> 4) != run.band) {
                        tile_flush(table[team], run);
                        run = TileRun{s >> 4, 0, 0, 0, 0, 0};
                    }
                    const unsigned long long v = (unsigned long long)M << (s & 31);
                    const unsigned long long sq = (unsigned long long)M * M;
                    const int sh = (2 * s) & 31;
                    const unsigned long long upper = sq >> (32 - sh);   // a shift of 1 .. 32
                    run.lo += (uint32_t)v, run.hi += v >> 32;
                    run.q0 += (uint32_t)(sq << sh), run.q1 += (uint32_t)upper, run.q2 += upper >> 32;
                }
            }
        }
        // the last runs: lanes that all ended in one band (or had no pixel) add theirs up first.  Every lane shuffles; who flushes
        // is decided afterwards.
        {
            const int band = (int)team_max<SUB>((uint32_t)(run.band + 1)) - 1;
            const unsigned long long agree = __ballot(run.band == band || run.band < 0);
            const unsigned long long mine = SUB == 64 ? ~0ull : ((1ull << (SUB & 63)) - 1ull) << (wave_lane & ~(SUB - 1));
            TileRun all = {band, team_sum<SUB>(run.lo), team_sum<SUB>(run.hi), team_sum<SUB>(run.q0), team_sum<SUB>(run.q1), team_sum<SUB>(run.q2)};
            if ((agree & mine) == mine) {
                if ((wave_lane & (SUB - 1)) == 0) tile_flush(table[team], all);
            } else {
                tile_flush(table[team], run);
            }
            n_zero = team_sum<SUB>(n_zero), n_infinite = team_sum<SUB>(n_infinite), n_clipped = team_sum<SUB>(n_clipped);
            max_key = team_max<SUB>(max_key);
            if ((wave_lane & (SUB - 1)) == 0) {
                if (n_zero) atomicAdd(&counter[team][kTileCountZero], n_zero);
                if (n_infinite) atomicAdd(&counter[team][kTileCountInfinite], n_infinite);
                if (n_clipped) atomicAdd(&counter[team][kTileCountClipped], n_clipped);
                if (max_key) atomicMax(&counter[team][kTileMaxKey], max_key);
            }
        }
        __syncthreads();

        // the finalisation: roles 0, 1, 2 form sum, sum_sq and mean in one body; role 3 writes the counts and the maximum
        const int role = TEAM <= 64 ? lane : ((lane & 63) == 0 ? lane >> 6 : 4);
        if (live && role < 4) {
            const uint32_t px = (uint32_t)((x1 - x0) * (y1 - y0));
            const uint32_t zero = counter[team][kTileCountZero], infinite = counter[team][kTileCountInfinite];
            const uint32_t clipped = counter[team][kTileCountClipped];
            if (role == 3) {
                if (a.out.max) reinterpret_cast<uint32_t *>(a.out.max)[tile] = counter[team][kTileMaxKey];
                if (a.out.n_px) a.out.n_px[tile] = (int32_t)px;
                if (a.out.n_zero) a.out.n_zero[tile] = (int32_t)zero;
                if (a.out.n_infinite) a.out.n_infinite[tile] = (int32_t)infinite;
                if (a.out.n_clipped) a.out.n_clipped[tile] = (int32_t)clipped;
            } else if (role == 0 ? a.out.sum != nullptr : role == 1 ? a.out.sum_sq != nullptr : a.out.mean != nullptr) {
                const bool squares = role == 1;
                const uint64_t *acc = reinterpret_cast<const uint64_t *>(table[team]) + (squares ? kSumLimbs : 0);
                const int n = squares ? kSumSqLimbs : kSumLimbs;
                uint32_t *limb = limbs[team][role];
                tile_capped_limbs(acc, n, squares, ck, clipped, limb);
                if (role == 2) {
                    const uint32_t counted = px - (ck == kSumInfinite ? infinite : 0u);
                    reinterpret_cast<uint32_t *>(a.out.mean)[tile] = counted ? tile_mean_bits(limb, n + 2, counted) : 0u;
                } else {
                    const uint64_t r = sum_round_bits(limb, n + 2, squares ? kSumSqUnitExp : kSumUnitExp);
                    reinterpret_cast<uint64_t *>(squares ? a.out.sum_sq : a.out.sum)[tile] = r;
                }
            }
        }
        __syncthreads();   // the table and the limbs are read: the next step may zero them
    }
}

template <int T, int TEAM>
void launch_tiles(const TilesArgs &a, hipStream_t s) {
    const long long n_groups = (a.n_tiles + kTilesBlock / TEAM - 1) / (kTilesBlock / TEAM);
    const unsigned grid = (unsigned)(n_groups < kTilesMaxGrid ? n_groups : kTilesMaxGrid);
    hipLaunchKernelGGL((score_tiles_kernel<T, TEAM>), dim3(grid), dim3(kTilesBlock), 0, s, a);
}

}  // namespace

// One launch: the kernel of the tile size.
hipError_t launch_score_tiles(const TilesArgs &a, hipStream_t s) {
    switch (a.tile) {
    case 8: launch_tiles<8, 16>(a, s); break;
    case 16: launch_tiles<16, 64>(a, s); break;
    case 32: launch_tiles<32, 256>(a, s); break;
    case 64: launch_tiles<64, 256>(a, s); break;
    default: return hipErrorInvalidValue;   // check_score_tiles_call lets no other through
    }
    return hipGetLastError();
}

}  // namespace statmc
