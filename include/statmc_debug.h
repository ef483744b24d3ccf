/* statmc_debug.h -- test, A/B and diagnostic switches of libstatmc_hip.so.  NOT part of the drop-in boundary
 * (include/statmc.h): nothing here has a counterpart in the reference, and a product host never calls it.  tests/,
 * bench.py's secondary legs and tools/experiments do.
 *
 * Like all library state the switches are PER DEVICE: they act on the calling thread's current device (statmc_set_device),
 * which must have been set up, and return STATMC_ERR_NO_DEVICE otherwise. */
#ifndef STATMC_DEBUG_H
#define STATMC_DEBUG_H

#include "statmc.h"

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Window-filter kernel of the device: 0 automatic; 1 window_filter_generic (global memory); 2 the one-sided LDS kernel's
 * runtime-radius build; 3 its compile-time r = 20 build (the kernel the pair-symmetric one replaced).  Any other value:
 * STATMC_ERR_INVALID. */
int statmc_debug_force_filter_variant(int variant);
/* Older name of statmc_set_filter_split (include/statmc.h). */
int statmc_debug_force_filter_parts(int parts);
/* Parts per tile of the calling thread's last window-filter call. */
int statmc_debug_last_filter_parts(void);
/* ... and its tail split: the last *tail_rows tile rows of the image swept with *parts_hi parts (0, 0: uniform). */
int statmc_debug_last_filter_tail(int *parts_hi, int *tail_rows);

/* Film-major accumulation: n > 0 runs it as n resident workgroups; 0 = by shape (default: the large interleaved grid, or one
 * workgroup per compute unit on 1080p-sized films of placed buffers from 256 samples per launch up); -1 = never a resident grid. */
int statmc_debug_accumulate_resident_blocks(int n);
/* Workgroups of the calling thread's last statmc_accumulate launch (which launch shape the sizes chose: DESIGN.md 4.1). */
int statmc_debug_last_accumulate_grid(void);
/* Film-major accumulation, the type-fused walk (one wave folds every stat type of its pixel groups in one pass over the samples;
 * launches of one RGB type with the transform and three moments plus up to two mean-only RGB and up to two mean-only 1-channel
 * types, all of the same pixels and batch length, 16-byte aligned): 0 = by shape (default: where the resident grid is taken, and from 128 samples per
 * launch up on films of 960 x 540 to 1920 x 1080 pixels);
 * 1 = every eligible launch, at any film size, with min(compute units, 256-group units) workgroups or the number set through
 * statmc_debug_accumulate_resident_blocks(n); -1 = never.  statmc_debug_accumulate_resident_blocks(-1) and
 * statmc_debug_accumulate_dma(0) switch it off as well.  Same bits either way.  Any other value: STATMC_ERR_INVALID. */
int statmc_debug_accumulate_fused(int mode);
/* 1 if the calling thread's last statmc_accumulate launch ran the type-fused walk, else 0. */
int statmc_debug_last_accumulate_fused(void);
/* How the calling thread's last film-major launch read its 16-bit arenas (statmc_accumulate_formats): 0 = it had none, 1 = the
 * vector path (8-byte pieces per lane, or the type-fused walk's LDS-DMA rows), 2 = the element-by-element fallback. */
int statmc_debug_last_accumulate_loader(void);
/* 1 (default): RGB sample planes stream through LDS-DMA; 0: loads into registers (same bits).  Any other value:
 * STATMC_ERR_INVALID. */
int statmc_debug_accumulate_dma(int on);
/* Film-major launch shape: grid_mode -1 = chosen by the batch length (default); 1 = one pass per workgroup, stat types
 * round-robin; 0 = capped grid with slots per type and a grid-stride walk.  dma_first 1 = the first rows of the LDS-DMA
 * ring are requested before the state loads (A/B; default 0). */
int statmc_debug_accumulate_launch(int grid_mode, int dma_first);
/* 2: the mean-only feature types of the film-major kernel prefetch twice as deep (default 1). */
int statmc_debug_accumulate_umul(int umul);
/* Tile-fed accumulation: prefetch depth of the mean-only types (1 | 2, default 2), item order, workgroups per CU. */
int statmc_debug_accumulate_tiles_variant(int umul, int order, int wg_per_cu);

/* Whether the calling thread's last accumulate call (statmc_accumulate and its _rows / _row_ranges / _formats forms,
 * statmc_accumulate_tiles[_formats], statmc_accumulate[_tiles]_counted) launched a counted kernel, and on which path: 0 = none (an
 * uncounted entry that got as far as its launch, sample_counts == NULL, a counted call that was a no-op or was refused), 1 = a
 * counted kernel on the vector path, 2 = a counted kernel element by element.  Tile launches: 1 when every type's images, its arena and the counts image are aligned for the vector path
 * and the film's width is a multiple of 4 (a tile whose own rows do not split into 4-pixel groups still goes element by element). */
int statmc_debug_last_accumulate_counted(void);

/* statmc_accumulate_records, for timing its two steps apart (tools/time_accumulate_records.py): 1 = the grouping only, 2 = the
 * fold only, over the index that the last full or grouping-only call with the same pixels and record count left in the
 * stream's workspace, 3 = both (default).  Any other value: STATMC_ERR_INVALID.  Applies to statmc_accumulate_records_split and
 * statmc_accumulate_records_interleaved_split as well (tools/time_accumulate_records_split.py). */
int statmc_debug_accumulate_records_phases(int phases);
/* statmc_accumulate_records_interleaved (to which the phases above apply too), the kernel of its fold: 0 = chosen by the type set
 * (default); 1 = the general kernel, one lane per pixel and stat type; 2 = the fused kernel, one lane per pixel holding every
 * type's state, where the call is eligible for it (one RGB type with the transform and three moments plus up to two mean-only
 * RGB and up to two mean-only 1-channel types, every field fp32, or the feature fields half with the radiance field in either
 * format), the general kernel elsewhere.  Same bits either way.  Any other value: STATMC_ERR_INVALID. */
int statmc_debug_accumulate_records_interleaved_path(int path);
/* The kernel the calling thread's last statmc_accumulate_records_interleaved call planned for its fold: 1 general, 2 fused; 0 if
 * it has not planned one (no call yet, a no-op, a refused call). */
int statmc_debug_last_accumulate_records_interleaved_path(void);

/* statmc_compact_accumulate, the kernel of its fold: 0 = the default (DESIGN.md 4.1j says which and why); 1 = staged, a wave
 * streaming the contiguous span of its 64 pixels through LDS, where the library has it -- elsewhere, and for whatever the staged
 * kernel does not take, the direct one; 2 = direct, one lane per pixel and stat type straight from global memory: the A/B
 * yardstick and the fallback.  Same bits either way.  Any other value: STATMC_ERR_INVALID. */
#define STATMC_COMPACT_PATH_STAGED 1
#define STATMC_COMPACT_PATH_DIRECT 2
#define STATMC_COMPACT_PATH_SPLIT 4
int statmc_debug_compact_path(int path);
/* What the calling thread's last statmc_compact_accumulate call launched: STATMC_COMPACT_PATH_STAGED or _DIRECT, plus
 * STATMC_COMPACT_PATH_SPLIT when the call had a split_above below INT32_MAX (runs above it folded by the 64 lanes of a wave); 0 if
 * it launched nothing (no call yet, a no-op, a refused call).  The report names the KERNEL of the launch, not what each wave did:
 * inside the staged kernel a wave stages only where the span of its 64 pixels fits 12 KiB, holds no run above split_above and
 * its clamped runs tile that span; every other wave of the launch takes the direct fold there.  Which waves those are follows
 * from the offsets alone (tools/time_accumulate_compact.py restates the rule as `staged_wave_share`); the library keeps no
 * per-wave count. */
int statmc_debug_last_compact_path(void);

/* statmc_compact_accumulate_interleaved, the kernel of its fold: 0 = the default (DESIGN.md 4.1k says which and why); 1 = the
 * fused kernel, staged: one lane per pixel holds every type's state, and a wave whose 64 clamped runs tile one span of records
 * that fits the wave's LDS window (and holds no run above split_above) lands that span in LDS and folds out of it -- every other
 * wave of the launch folds directly; 2 = the fused kernel, direct: every lane walks its run straight from global memory; 3 = the
 * general kernel, one lane per pixel and stat type.  1 and 2 apply where the type set is one of the fused fold's; elsewhere the
 * general kernel runs.  Same bits every way.  Any other value: STATMC_ERR_INVALID. */
#define STATMC_COMPACT_ILV_PATH_FUSED_STAGED 1
#define STATMC_COMPACT_ILV_PATH_FUSED_DIRECT 2
#define STATMC_COMPACT_ILV_PATH_GENERAL 3
#define STATMC_COMPACT_ILV_PATH_SPLIT 4
int statmc_debug_compact_interleaved_path(int path);
/* What the calling thread's last statmc_compact_accumulate_interleaved call launched: one of the three kernels above, plus
 * STATMC_COMPACT_ILV_PATH_SPLIT when the call had a split_above below INT32_MAX (runs above it folded by the 64 lanes of a wave:
 * behind a fused kernel in a second launch of the general one); 0 if it launched nothing (no call yet, a no-op, a refused call).
 * As statmc_debug_last_compact_path, the report names the KERNEL, not what each wave did. */
int statmc_debug_last_compact_interleaved_path(void);
/* The staged kernel's LDS window per wave, bytes: a multiple of 1024 in [1024, 65536], or 0 for the default.  One wave per
 * workgroup: the window decides how many waves share a CU (tools/time_accumulate_compact_interleaved.py times the choices). */
int statmc_debug_compact_interleaved_window(int bytes);

/* The placed allocator's probe (statmc_amd/csrc/statmc_placement.hip) on memory of the caller's: streams [stream_ptr, + stream_bytes)
 * while every fourth step read-modify-writes 16 bytes inside [rmw_ptr, + rmw_bytes) -- the words there change.  Best of five, ms.
 * Two buffers in the same interference class: ~ 9 % slower than two in different ones (1-GiB stream, 64-MiB window). */
int statmc_debug_interference_probe(const void *stream_ptr, size_t stream_bytes, void *rmw_ptr, size_t rmw_bytes, float *ms);
/* The role of the statmc_malloc_placed block that holds `ptr` (any address inside it; window blocks included), -1 when `ptr` is
 * in none, the block was dealt without the wanted class, or the device tells no classes apart: what statmc_accumulate asks. */
int statmc_debug_placement_role(const void *ptr);
/* The placed allocator's fast level for a list of probe times against slot 0 (ms; <= 0 = not probed) and slot 0's probe against
 * itself (0 = unknown): what its class thresholds are multiples of.  Pure arithmetic, no device call (tests/test_abi_cpu.py). */
float statmc_debug_placement_fast_level(const float *probes_ms, int n, float self_ms);

/* Welch degrees of freedom on the pair-symmetric kernel: the number of work items of the calling thread's last launch
 * that left their band of the quantile table and were computed again from the table in global memory (0 for a film of
 * uniform sample count; -1: the last pair-symmetric launch was not a Welch one).  Waits for the device. */
int statmc_debug_welch_far_items(void);
/* Largest filter workspace of the current device (bench.py reports where it lives). */
int statmc_debug_last_workspace(void **ptr, size_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* STATMC_DEBUG_H */
