// statmc_device.h -- kernel-side argument blocks and launch prototypes shared by the
// .hip translation units of libstatmc_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/statmc.h"

namespace statmc {

// a plane that whole 4-pixel groups can move to and from as dwordx4 (NULL, an absent plane, passes)
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------- pointwise kernels
struct PrepassArgs {
    const int32_t *n;
    const float *mean, *m2, *m3;
    float *mean_corr, *disc;
    long long n_elems;  // width*height*channels
    int channels;
    int table;            // alpha_index + 3 * sides
    int welch;            // discriminator = s^2 / n (no quantile)
    int small_n_exclude;  // n < 2 -> NaN mean / discriminator
};

struct MeanVarsArgs {
    const int32_t *n;
    const float *film_m2;
    float *film_var;
    int width, height, channels, row_n_quirk;
};

constexpr int kMaxStatTypes = 16;   // stat types of a call x row ranges of a call (statmc_accumulate_row_ranges)
struct AccumulateType {
    const float *samples;
    int32_t *n;
    float *mean, *m2, *m3, *film_mean, *film_m2;
    long long n_elems;  // elements this launch updates: width * rows * channels
    long long stride;   // floats between consecutive samples of an element: width * height * channels (> n_elems when the launch covers a range of rows)
    int channels, n_samples, transform, max_moment;
    // optional epilogue (max_moment 3): the pre-pass of the updated moments -- Johnson-corrected mean and discriminator, what
    // prepass_kernel computes from n / mean / m2 / m3 -- written while the state is still in registers (NULL: off)
    float *mean_corr, *disc;
    int pre_table;      // Student-t table of the device's significance level and sides (t_quantile)
    int pre_flags;      // 1: Welch degrees of freedom (t = 1: the pair looks its quantile up), 2: n < 2 excludes the pixel
};
constexpr int kMaxSlots = 64;
struct AccumulateArgs {
    AccumulateType t[kMaxStatTypes];
    int n_types;
    int resident_blocks;  // 0: by shape (plan_accumulate); > 0: that many workgroups walk all types; -1: never (A/B)
    int cus;              // compute units of the device (the resident grid's size where the shape calls for one)
    int umul;             // 2: the mean-only feature types prefetch twice as deep (statmc_debug_accumulate_umul; A/B)
    int dma;              // RGB sample planes arrive by LDS-DMA (default 1; 0: loads into registers, A/B)
    int grid_mode;        // -1: by batch length (default); 0: capped grid, slots per type in proportion to cost, grid-stride; 1: one pass per workgroup, types round-robin
    int dma_first;        // the first rows of the LDS-DMA ring are requested before the state loads
    int occ;              // unused: kept so that the fields behind it keep their kernel-argument offsets
    int apart;            // 1: samples and moments are known to lie in different interference classes (statmc_malloc_placed blocks)
    // large grid: workgroup b serves slot b % n_slots; slots are dealt to types in proportion to cost
    int n_slots;
    int type_slots[kMaxStatTypes];
    unsigned char slot_type[kMaxSlots], slot_rank[kMaxSlots];
    // the type-fused walk (plan_accumulate): 0 by shape, 1 whenever the launch is eligible, -1 never (statmc_debug_accumulate_fused);
    // read by the host only, and last so that the fields before it keep their kernel-argument offsets
    int fused;
    // statmc_accumulate_formats: bit i = t[i].samples is an IEEE-half arena (n_elems and stride still count elements).  Read by
    // accumulate_half_kernel alone; it takes the padding behind `fused`, so the argument keeps its size.
    int half_mask;
};
// the kernels take the block by value: nothing in it moves (occ, fused and half_mask are where they are for that reason)
static_assert(sizeof(AccumulateArgs) == 2032 && offsetof(AccumulateArgs, n_slots) == 1828, "AccumulateArgs: kernel-argument offsets");

// samples of every type arrive tile by tile: AccumulateType::samples is the type's arena, tile k's
// block starts at float offset tile_offsets[k] * channels and holds tile_samples[k] planes of
// tile_h x tile_w pixels; AccumulateType::n_samples and n_elems are not used
struct AccumulateTilesArgs {
    AccumulateType t[kMaxStatTypes];
    int n_types;
    const int32_t *tile_bounds;      // device, {x0, y0, x1, y1} per tile
    const long long *tile_offsets;   // device, in pixel-samples
    const int32_t *tile_samples;     // device
    int n_tiles, width, height, vec;
    int dma;                         // RGB sample planes arrive by LDS-DMA (default 1)
    int umul, order, wg_per_cu;      // experiment knobs (statmc_debug_accumulate_tiles_variant): prefetch depth x2, item order, grid size
    int dma_first;                   // A/B (statmc_debug_accumulate_launch): the first rows of the LDS-DMA ring requested before the state loads
    // statmc_accumulate_tiles_formats: bit i = t[i].samples is an IEEE-half arena (tile_offsets still count pixel-samples).  Non-zero:
    // the launch is accumulate_tiles_half_kernel's, and `vec` holds one bit per type (the vector path is a type's own there).  It
    // takes the padding behind dma_first, so the fields before it keep their kernel-argument offsets and the argument its size.
    int half_mask;
};
static_assert(sizeof(AccumulateTilesArgs) == sizeof(AccumulateType) * kMaxStatTypes + 72 && offsetof(AccumulateTilesArgs, half_mask) + 4 == sizeof(AccumulateTilesArgs),
              "AccumulateTilesArgs: kernel-argument offsets");

// statmc_accumulate_counted / statmc_accumulate_tiles_counted (statmc_counted.hip): the arena of the uncounted entry plus an int32
// film image that says how many of its planes are live for each pixel.  Argument blocks of their own: AccumulateArgs and
// AccumulateTilesArgs above, and the kernels that take them, stay what they are.
struct AccumulateCountedArgs {
    AccumulateType t[kMaxStatTypes];         // as AccumulateArgs::t (stat types x row ranges); n_samples is the arena's capacity S
    const int32_t *counts[kMaxStatTypes];    // the count of entry i's first pixel (the film image, advanced to the entry's first row)
    statmc_prepass_context ctx;              // the pre-pass epilogue's table and flags (entries with mean_corr / disc)
    int n_types;
    int half_mask;                           // bit i = t[i].samples is an IEEE-half arena
};
struct AccumulateTilesCountedArgs {
    AccumulateType t[kMaxStatTypes];         // as AccumulateTilesArgs::t
    statmc_prepass_context ctx;
    const int32_t *counts;                   // [height][width], indexed by film pixel
    const int32_t *tile_bounds;              // device, {x0, y0, x1, y1} per tile
    const long long *tile_offsets;           // device, in pixel-samples
    const int32_t *tile_samples;             // device: the capacity S of tile k's block
    int n_types, n_tiles, width, height;
    int vec;                                 // bit i = type i's images, arena and the counts image are aligned for the vector path
    int half_mask;
};
static_assert(sizeof(AccumulateCountedArgs) <= 4096 && sizeof(AccumulateTilesCountedArgs) <= 4096, "passed by value: the kernel-argument limit");
// path (out): what statmc_debug_last_accumulate_counted reports -- 1 the vector path, 2 element by element
hipError_t launch_accumulate_counted(const AccumulateCountedArgs &a, hipStream_t s, int *path);
hipError_t launch_accumulate_tiles_counted(const AccumulateTilesCountedArgs &a, hipStream_t s, int *path);
// whether a lane can own 4 consecutive pixels of the type as 16-byte pieces (statmc_pointwise.hip; film_major: also the plane sizes)
bool acc_type_vectorizable(const AccumulateType &t, bool half_arena, bool film_major);

// statmc_combine_statistics: one entry per pair of states.  The counts are read from cnt_dst / cnt_src: the entry's own
// count images, or those of the entry it borrows them from.  The ABI puts borrowing entries first, so that they read the
// counts before their owner (later in the same lane) writes n = nA + nB.
enum { kCombMean = 0, kCombM2, kCombM3, kCombFilmMean, kCombFilmM2, kCombFields };
struct CombineEntry {
    int32_t *cnt_dst;
    const int32_t *cnt_src;
    float *d[kCombFields];           // dst planes (NULL: not combined)
    const float *s[kCombFields];     // the matching src planes
    float *mean_corr, *disc;         // optional pre-pass epilogue (own counts, max_moment 3)
    int channels, write_n, pre_table, pre_flags;
};
struct CombineArgs {
    CombineEntry e[kMaxStatTypes];
    int n_entries;
    int vec;                         // every plane 16-byte aligned: whole 4-pixel groups move as dwordx4
    long long n_px;
};
hipError_t launch_combine(const CombineArgs &a, hipStream_t s);

// statmc_combine_many: one chain of up to three planes per kernel entry -- an ABI entry's moments, or its raw-sample chain
// (film_mean / film_m2 of their own), which is a chain of at most two planes weighed with the same counts -- folded over
// n_sources parts.  src holds kCombManySrcPtrs pointers per (entry, source): the part's counts, then its planes; entry i's
// source k starts at (i * n_sources + k) * kCombManySrcPtrs.  The whole argument stays below the 4-KB kernel-argument
// limit, so a launch takes min(kMaxStatTypes, kCombManySlots / n_sources) entries; the ABI splits a call into launches,
// entries that do not write counts first (launches of one stream run in order).
enum { kCombManyPlanes = 3, kCombManySrcPtrs = 1 + kCombManyPlanes, kCombManySlots = 90 };
struct CombineManyEntry {
    int32_t *cnt_dst;
    float *d[kCombManyPlanes];       // dst planes, the first `moments` of them
    float *mean_corr, *disc;         // optional pre-pass epilogue (own counts, moments 3)
    int channels, moments, write_n, pre;   // pre: pre_table | pre_flags << 8
};
struct CombineManyArgs {
    long long n_px;
    int n_entries, n_sources;
    int vec;                         // every plane 16-byte aligned: whole 4-pixel groups move as dwordx4
    int reserved;
    CombineManyEntry e[kMaxStatTypes];
    const void *src[kCombManySlots * kCombManySrcPtrs];
};
static_assert(sizeof(CombineManyArgs) <= 4096, "CombineManyArgs is passed by value: the kernel-argument limit");
hipError_t launch_combine_many(const CombineManyArgs &a, hipStream_t s);

// statmc_accumulate_records (statmc_records.hip): every type's `samples` is record-major [n_records][channels]; the types
// travel as the ABI's own descriptors, which is what statmc::device::PixelStats loads and stores through.
struct RecordsArgs {
    statmc_stat_type t[kMaxStatTypes];
    statmc_prepass_context ctx;      // the pre-pass epilogue's table and flags (types with mean_corr / discriminator)
    const int32_t *order;            // record indices sorted by pixel, stable          (workspace)
    const int32_t *seg;              // {start, end} of every pixel's run in order[]    (workspace)
    long long n_records, n_px;
    int n_types;
};
// the per-(device, stream) scratch of one call: byte offsets into one block
struct RecordsWorkspace {
    size_t keys_off, order_off, seg_off, seg_bytes, temp_off, temp_bytes, bytes;
};
hipError_t records_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w);   // host only: no launch
// phases: 1 = grouping, 2 = fold, 3 = both (the ABI's call; 1 and 2 alone: statmc_debug_accumulate_records_phases)
// split_above: 0 = statmc_accumulate_records (records_fold_kernel); >= 1 = statmc_accumulate_records_split (records_split_fold_kernel)
hipError_t launch_accumulate_records(const RecordsArgs &a, const int32_t *pixels, const RecordsWorkspace &w, char *ws, int phases,
                                     int split_above, hipStream_t s);

// statmc_accumulate_records_interleaved (statmc_records.hip; the host's decisions: statmc_records_plan.h): record i starts at
// records + i * stride and holds its pixel index at pixel_off and type t's values at off[t], half where bit t of half_mask is set.
// The grouping, order[], seg[] and the workspace are statmc_accumulate_records'.
struct RecordsInterleavedArgs {
    statmc_stat_type t[kMaxStatTypes];
    statmc_prepass_context ctx;
    const int32_t *order;
    const int32_t *seg;
    const char *records;
    long long n_records, n_px;
    int n_types;
    int stride, pixel_off;
    int off[kMaxStatTypes];
    unsigned half_mask;
};
struct RecordsInterleavedPlan;      // statmc_records_plan.h
hipError_t records_interleaved_workspace_layout(long long n_records, long long n_px, RecordsWorkspace &w);   // host only: no launch
// split_above: 0 = statmc_accumulate_records_interleaved; >= 1 = statmc_accumulate_records_interleaved_split
hipError_t launch_accumulate_records_interleaved(const RecordsInterleavedArgs &a, const RecordsInterleavedPlan &plan, const RecordsWorkspace &w, char *ws,
                                                 int phases, int split_above, hipStream_t s);

// statmc_gather_states / statmc_combine_records (statmc_state_records.hip): argument block and checks are statmc_state_records_args.h's.
// The combine groups its records as statmc_accumulate_records does -- group_records_by_pixel is that entry's grouping step on its
// own (statmc_records.hip): seg[] zeroed, the stable sort of the record indices by pixel into order[], seg[], in the workspace
// block ws that records_workspace_layout laid out.
struct StateRecordsArgs;
hipError_t group_records_by_pixel(const int32_t *pixels, long long n_records, long long n_px, const RecordsWorkspace &w, char *ws, hipStream_t s);
hipError_t launch_gather_states(const StateRecordsArgs &a, hipStream_t s);
hipError_t launch_combine_records(const StateRecordsArgs &a, const RecordsWorkspace &w, char *ws, hipStream_t s);

// statmc_pool_statistics (statmc_pool.hip): the argument block and its checks are statmc_pool_args.h's, a host-only header
struct PoolArgs;
hipError_t launch_pool(const PoolArgs &a, hipStream_t s);

// statmc_sample_scores / statmc_plan_samples (statmc_plan.hip): argument blocks and checks are statmc_plan_args.h's, host-only
struct ScoreArgs;
struct PlanArgs;
hipError_t launch_sample_scores(const ScoreArgs &a, hipStream_t s);
hipError_t launch_plan_samples(const PlanArgs &a, size_t workspace_bytes, hipStream_t s);

// statmc_error_scores / statmc_plan_to_target (statmc_error.hip): argument blocks and checks are statmc_error_args.h's, host-only
struct ErrorArgs;
struct TargetArgs;
hipError_t launch_error_scores(const ErrorArgs &a, hipStream_t s);
hipError_t launch_plan_to_target(const TargetArgs &a, hipStream_t s);

// statmc_upsample_filtered (statmc_upsample.hip): the argument block and its checks are statmc_upsample_args.h's, a host-only header
struct UpsampleArgs;
hipError_t launch_upsample(const UpsampleArgs &a, hipStream_t s);

// statmc_score_select / statmc_score_count_above (statmc_select.hip): argument blocks and checks are statmc_select_args.h's, host-only
struct SelectArgs;
struct CountAboveArgs;
hipError_t launch_score_select(const SelectArgs &a, hipStream_t s);
hipError_t launch_score_count_above(const CountAboveArgs &a, hipStream_t s);

// statmc_score_sum (statmc_score_sum.hip): argument block, checks and finalisation are statmc_score_sum_args.h's, host-only
struct SumArgs;
hipError_t launch_score_sum(const SumArgs &a, hipStream_t s);

// statmc_score_tiles (statmc_score_tiles.hip): argument block, checks and finalisation are statmc_score_tiles_args.h's, host-only
struct TilesArgs;
hipError_t launch_score_tiles(const TilesArgs &a, hipStream_t s);

// statmc_score_tile_select / statmc_gate_tiles (statmc_tile_select.hip): argument blocks and checks are statmc_tile_select_args.h's, host-only
struct TileSelectArgs;
struct GateArgs;
hipError_t launch_tile_select(const TileSelectArgs &a, hipStream_t s);
hipError_t launch_gate_tiles(const GateArgs &a, hipStream_t s);

// statmc_score_window (statmc_score_window.hip): argument block and checks are statmc_score_window_args.h's, host-only
struct ScoreWindowArgs;
hipError_t launch_score_window(const ScoreWindowArgs &a, hipStream_t s);

// statmc_compact_offsets / statmc_compact_accumulate (statmc_compact.hip): argument blocks and checks are statmc_compact_args.h's
struct CompactOffsetsArgs;
struct CompactArgs;
hipError_t launch_compact_offsets(const CompactOffsetsArgs &a, hipStream_t s);
// force: statmc_debug_compact_path's value; path (out): what statmc_debug_last_compact_path reports
hipError_t launch_compact_accumulate(const CompactArgs &a, int force, hipStream_t s, int *path);
// statmc_compact_accumulate_interleaved (statmc_compact.hip): argument block, checks and the plan are statmc_compact_interleaved_args.h's
struct CompactInterleavedArgs;
struct RecordsInterleavedPlan;
// kernel: plan_compact_interleaved's; window: the staged variant's LDS bytes per wave; path (out): what
// statmc_debug_last_compact_interleaved_path reports
hipError_t launch_compact_accumulate_interleaved(const CompactInterleavedArgs &a, const RecordsInterleavedPlan &plan, int kernel, int window,
                                                 hipStream_t s, int *path);

struct MergeTilesArgs {
    const void *tile_pixels;
    const int32_t *tile_bounds;
    const long long *tile_offsets;
    int32_t *n;
    float *mean, *m2, *m3, *film_mean, *film_m2;
    int width, height, channels, transform;
};

struct TileMomentsArgs {
    const float *values;
    float *out;
    int width, height, channels, tile_size, tiles_x, tiles_y;
};

// ---------------------------------------------------------------- window filter
struct GBufferDesc {
    const float *data;
    int channels;
    float dr;  // -0.5/sd^2
};

// one buffer (one colour image, one stat set) per launch
struct FilterArgs {
    const float *mean_corr, *disc, *colour;
    float *out;
    // filter spec (statmc_filter_spec): every field but dof = Welch has an LDS kernel (statmc_filter.hip, statmc_filter_sym.hip)
    int gate, channel_rule, dof, border;
    int force_variant, force_parts;   // unused: kept so that the fields behind them keep their kernel-argument offsets
    const int32_t *n;            // Welch mode: sample counts
    const float *tq;             // Welch mode: this device's quantile table (4096 entries)
    const float *tq2;            // ... and its squares: tq2[dof] = fl(t_dof * t_dof), dof = 0 .. 4096, entry 0 = entry 1 (pair-symmetric kernel)
    int width, height;           // local image
    int rx0, ry0, rx1, ry1;      // output ROI
    int rx_split, n_main_items;  // LDS kernel: regular tiles cover [rx0, rx_split), DUAL tiles [rx_split, rx1)
    int radius;
    float ds;                    // -0.5/sd_s^2
    int n_g;
    GBufferDesc g[STATMC_MAX_GBUFFERS];
    // fast path only (T = float3, two 3-channel G-buffers):
    const float *spatial_tab;    // [(2r+1)][2*RP+7] log2-domain spatial exponents, -inf outside r
    float gscale0, gscale1;      // sqrt(-dr_g * log2(e))
    // G-buffer sets other than "up to two RGB images" whose channels still fit the kernel's six feature
    // slots (e.g. normal + depth + material id): slot f reads data[pixel * stride + offset] * scale;
    // gscale0 = gscale1 = 1 then.  scale 0 = empty slot.
    int feat_generic;
    struct FeatSlot {
        const float *data;
        int stride, offset;
        float scale;
    } feat[6];
    int n_parts;                 // window rows are swept by n_parts workgroups per tile ...
    float *partial;              // ... which leave their sums here: [n_parts][height][width][4 (RGB) | 8 (float x3)]
    // fast path, filter<float>: up to three 1-channel buffers per launch (f_active of them real;
    // the rest repeat the last one and are not stored)
    const float *f_mean_corr[3], *f_disc[3], *f_colour[3];
    const int32_t *f_n[3];       // Welch degrees of freedom: the buffers' sample counts (pair-symmetric kernel: two buffers per launch)
    float *f_out[3];
    int f_active;
    const float *packed;         // optional [height][width][packed_ch] inputs: mc, disc, colour, g0, g1 (RGB each)[, s0, s1]
    int packed_ch;               // 15, 16 (+ the sample count's bits: the Welch builds of the pair-symmetric kernel) or 17 (+ two
                                 // 1-channel G-buffers: its eight-plane build)
    // pair-symmetric kernel (statmc_filter_sym.hip): tiles of 128 x 8 pixels on a grid fixed in film coordinates
    struct SymGeom {
        int tx0, ty0, ntx, nty;   // tile range of the launch (film tile indices)
        int fx0, fy0;             // film coordinates of local pixel (0, 0)
        long long item_stride4;   // float4 per work item (tile, part) in the patch workspace
        float4 *patch;            // [items][p-side 8 x 128 | q-side rows x 168] (sum w*colour rgb, sum w)
        int pair;                 // filter<float>: f_active (1 or 2) 1-channel buffers (f_mean_corr / f_disc / f_colour / f_out) per launch
        float *pair_images;       // ... staged from three [height][width][3] images this launch packs them into
        float4 *border_extra;     // border rule "clamp": per pixel, the sums over the taps beyond the image (border_virtual_kernel)
        int *redo;                // Welch: one flag per work item, set by the band build for the items the far build computes again
        // eight feature planes (NG = 8 build): up to two RGB and up to two 1-channel G-buffers of the argument list, sorted
        // into slots by the planner; scale = sqrt(-dr * log2 e), 0 = empty slot (never read)
        // Tail split (round 4): the tiles of the film's tile rows >= split_ty sweep with parts_hi workgroups each instead of
        // n_parts, so that the launch's last round of workgroups is full (1280 x 720: 900 tiles = 3.5 rounds of 256).  The
        // work items of the n_parts-tiles come first (n_lo_items of them: the launch's tile rows below split_ty), then
        // those of the parts_hi-tiles.  parts_hi = 0: every tile has n_parts.  Chosen for the WHOLE local image, like n_parts.
        int parts_hi, split_ty, n_lo_tiles, n_lo_items;
        int steps;                // window rows a tile sweeps: radius + 1
        const float *tab_rt;      // runtime-radius build (radius < 20): [radius + 1][47] spatial exponents, row = dy, -inf beyond the radius
        int g8;
        const float *rgb[2], *sc[2];
        float rgb_scale[2], sc_scale[2];
    } sym;
};

struct PackArgs {
    const float *mean_corr, *disc, *colour, *g0, *g1;  // [src_h][src_w][3]  (an absent G-buffer: nullptr, packed as zeros)
    float *packed;                                      // [dst_h][dst_w][ch]
    int src_w, src_h, dst_w, dst_x0, dst_y0;
    const float *s0, *s1;                               // ch = 17: the two 1-channel G-buffers [src_h][src_w] (nullptr: zeros)
    int ch;                                             // 15 | 16 | 17
    const int32_t *n;                                   // ch = 16: the sample counts (channel 15 holds their bits: Welch dof)
};
hipError_t launch_pack_inputs(const PackArgs &a, hipStream_t s);

// pre-pass and pack in one pass (RGB): statistics + colour + two G-buffers in, packed image out
// (mean_corr / disc also written to their own images when the pointers are set)
struct PrepassPackArgs {
    const int32_t *n;
    const float *mean, *m2, *m3, *colour, *g0, *g1;
    float *mean_corr, *disc;   // optional
    float *packed;             // [dst_h][dst_w][ch]
    int src_w, src_h, dst_w, dst_x0, dst_y0, table, welch, small_n_exclude;
    int split_row, skip_rows;   // rows >= split_row of the launch's src_h rows sit skip_rows further down in every image (two row ranges in one launch)
    const float *s0, *s1;       // ch = 17: the two 1-channel G-buffers (nullptr: zeros); g0 / g1 may be nullptr as well then
    int ch;                     // 15 | 16 (channel 15 = the bits of n: Welch degrees of freedom) | 17
};
hipError_t launch_prepass_pack(const PrepassPackArgs &a, hipStream_t s);

hipError_t upload_t_tables();
hipError_t upload_t_table(int table, const float *host_4096);
const float *t_table_device_ptr(int table);  // current device's copy of quantile table `table`
const float *t_table_sq_device_ptr(int table);  // ... of its squares (fl(t * t), what the Welch pair test multiplies with)
hipError_t launch_prepass(const PrepassArgs &a, hipStream_t s);
hipError_t launch_mean_vars(const MeanVarsArgs &a, hipStream_t s);
// What one film-major accumulation runs.  plan_accumulate decides it from the argument alone -- no HIP call, no global or
// thread-local state, so tests/cpp/test_accumulate_plan.cpp pins every rule without a GPU -- and launch_accumulate launches it.
enum { kAccPerType = 0, kAccPerTypeHalf, kAccFused, kAccFusedHalf };
struct AccumulateFusedArgs;     // the type-fused walk's argument (statmc_pointwise.hip)
struct AccumulatePlan {
    int kernel;             // kAccPerType: accumulate_kernel, kAccPerTypeHalf: accumulate_half_kernel, kAccFused / kAccFusedHalf: accumulate_fused[_half]_kernel
    int vec;                // whole 4-pixel groups move as 16-byte (half arenas: 8-byte) pieces; 0: element by element
    int dma, umul;          // accumulate_kernel's template arguments: the LDS-DMA ring's depth (0: register loads), the prefetch depth
    int K, M, fmt;          // the fused kernels': mean-only RGB types, mean-only 1-channel types, formats (0 / 1 / 2 as acc_fused_is_half has it)
    unsigned grid;          // workgroups
    size_t lds;             // dynamic LDS per workgroup, bytes
    int resident_blocks, grid_mode;     // what the per-type kernels read from their argument
    int loader;             // what last_accumulate_loader() reports
};
AccumulatePlan plan_accumulate(const AccumulateArgs &a, AccumulateFusedArgs *fused_out);   // fused_out (may be NULL): filled when a fused kernel is planned
hipError_t launch_accumulate(const AccumulateArgs &a, hipStream_t s);
unsigned last_accumulate_grid();
int last_accumulate_fused();         // 1: the calling thread's last film-major launch ran the type-fused walk
int last_accumulate_loader();        // that launch's 16-bit arenas: 0 it had none, 1 the vector path, 2 element by element
hipError_t launch_accumulate_tiles(const AccumulateTilesArgs &a, hipStream_t s);
hipError_t launch_merge_tiles(const MergeTilesArgs &a, int n_tiles, int max_tile_pixels, hipStream_t s);
hipError_t launch_tile_moments(const TileMomentsArgs &a, hipStream_t s);
hipError_t launch_film_update(const void *pixels, long long n, float splat_scale, float scale, float *rgb, hipStream_t s);

// What one window-filter call runs (plan_window_filter, statmc_filter.hip): the kernel and build of its launches, how its
// buffers are grouped into launches, and the tables and workspace the C-ABI layer provides for them.
enum { kFilterGeneric, kFilterLds, kFilterSym };
struct FilterPlan {
    int kernel;                 // of the main launches: kFilterGeneric (global memory), kFilterLds (one-sided), kFilterSym (pair-symmetric)
    bool lds_r20;               // the one-sided kernel's launches run its compile-time r = 20 build
    int per_launch;             // float buffers per main launch: 1, 2 (pair-symmetric) or 3 (one-sided)
    bool lds_tail;              // an odd number of float buffers ends with three of them on the one-sided kernel, in one part
    bool spatial_tab, sym_rt_tab;   // the launches read FilterArgs::spatial_tab / sym.tab_rt
    // workspace in floats: the one-sided kernel's partial sums (n_parts > 1), or the pair-symmetric kernel's patches, pair
    // images, clamped-border sums and Welch redo flags, in this order, each a multiple of 4
    size_t partial_floats, patch_floats, image_floats, extra_floats, redo_floats;
    int redo_items;             // pair-symmetric: work items of the launch (one redo flag each)
    int tail_rows;              // ... tile rows the tail split sweeps with sym.parts_hi parts (0: uniform)
    char variant[48], tail_variant[96];   // names of the main launches and of the tail launch
};
// STATMC_OK, or STATMC_ERR_UNSUPPORTED (with the message recorded) for a block + halo image no kernel can read.  Fills the
// layout fields of k: feature scales and slots, parts, the pair-symmetric kernel's tile range and split.
int plan_window_filter(FilterArgs &k, int channels, int n_buffers, int n_cus, int force_variant, int split, FilterPlan &p);
// What the planner and the pack entries say to a 17-channel block + halo image that holds exactly two RGB G-buffers and no
// 1-channel one under STATMC_DOF_PIXEL.  It would run the eight-plane build, which shares the window after read group 6, where the
// whole film with the same G-buffers -- and its 15-channel image -- runs the G7 build at r = 20 (statmc_filter_sym.hip, gsplit_of):
// not the same bits.  The set has one packed layout, 15 channels.
constexpr const char *kTwoRgbIn17Channels =
    "packed image (17 channels): exactly two RGB G-buffers and no 1-channel one belong in the 15-channel layout under STATMC_DOF_PIXEL "
    "(the 17-channel image would not reproduce the whole film's bits)";
hipError_t launch_window_filter(const FilterPlan &p, bool tail, const FilterArgs &a, int channels, hipStream_t s);
// window-sweep parts per tile for the whole local image (statmc_filter_split_auto: sym, split 0)
int whole_image_parts(const FilterArgs &a, bool sym, int n_cus, int split);
// Size in floats of the spatial table the fast path wants for radius r (0 if r unsupported).
size_t spatial_table_floats(int radius);
size_t sym_rt_table_floats(int radius);                   // pair-symmetric kernel, radius < 20
void fill_sym_rt_table(float *host_tab, int radius, float ds);
void fill_spatial_table(float *host_tab, int radius, float ds);

// statmc_placement.hip (device memory placed by HBM rank)
int abi_fail(int code, const char *fmt, ...);   // records the calling thread's statmc_last_error() text, returns `code` (statmc_abi.hip)
int placement_role_of(const void *ptr);         // STATMC_MEM_STATE / _STREAM when `ptr` lies in a block dealt with the wanted class, else -1
int placement_free(void *ptr);                  // 1: `ptr` was a statmc_malloc_placed block and is free now; 0: not the placed allocator's; -1: inside its ranges, not a live block's start
hipError_t workspace_alloc(void **p, size_t bytes);   // the library's own read-and-written workspaces: STATE role where the device's caller uses placed memory, hipMalloc otherwise
hipError_t workspace_free(void *p);
hipError_t placement_grant_peer(int owner_device, int peer_device);   // blocks of `owner`'s placed allocator become valid operands of copies device `peer` executes

}  // namespace statmc
