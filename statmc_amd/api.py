"""ctypes binding of libstatmc_hip.so (include/statmc.h) + thin helpers that marshal torch
tensors (device memory, streams) into the C structs.  Plumbing only: every number is produced
by the HIP kernels behind the C ABI.
"""
import ctypes as C
import os

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))

STATMC_OK = 0
ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE = -1, -2, -3, -4
DOF_PIXEL, DOF_WELCH = 0, 1      # statmc_filter_spec.dof (include/statmc.h)
MAX_BUFFERS, MAX_GBUFFERS = 16, 8


class StatmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("statmc error %d: %s" % (code, msg))
        self.code = code


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("step", C.c_size_t), ("cols", C.c_int32), ("rows", C.c_int32)]


class FilterArgs(C.Structure):
    _fields_ = [
        ("n_buffers", C.c_uint8), ("width", C.c_uint16), ("height", C.c_uint16),
        ("filter_ds_factor", C.c_float), ("filter_radius", C.c_uint8), ("denoise_film", C.c_uint8),
        ("n", C.POINTER(Image)), ("mean", C.POINTER(Image)), ("m2", C.POINTER(Image)),
        ("m3", C.POINTER(Image)), ("film", C.POINTER(Image)), ("film_buffer", Image),
        ("g_buffers", C.POINTER(Image)), ("g_channel_counts", C.POINTER(C.c_uint8)),
        ("g_dr_factors", C.POINTER(C.c_float)), ("n_g_buffers", C.c_size_t),
        ("mean_corr", C.POINTER(Image)), ("discriminator", C.POINTER(Image)),
        ("film_filtered", C.POINTER(Image)), ("film_filtered_buffer", Image),
        ("stream", C.c_void_p),
        ("roi_x0", C.c_int32), ("roi_y0", C.c_int32), ("roi_x1", C.c_int32), ("roi_y1", C.c_int32),
        ("packed_inputs", Image),
        ("film_x0", C.c_int32), ("film_y0", C.c_int32),
    ]


class FilterSpec(C.Structure):
    """statmc_filter_spec: what the reference tree leaves open about filter<T>.  All-zero = default."""
    _fields_ = [("gate", C.c_int32), ("channel_rule", C.c_int32), ("sides", C.c_int32), ("dof", C.c_int32),
                ("border", C.c_int32), ("small_n", C.c_int32)]

    def __init__(self, gate=0, channel_rule=0, sides=0, dof=0, border=0, small_n=0):
        super().__init__(gate, channel_rule, sides, dof, border, small_n)

    def as_tuple(self):
        return (self.gate, self.channel_rule, self.sides, self.dof, self.border, self.small_n)


class PlacementInfo(C.Structure):
    _fields_ = [("active", C.c_int32), ("virtual_memory", C.c_int32), ("slots", C.c_int32), ("probes", C.c_int32),
                ("slots_a", C.c_int32), ("slots_b", C.c_int32), ("slots_c", C.c_int32), ("slots_unclear", C.c_int32), ("slots_idle", C.c_int32),
                ("slots_as_they_came", C.c_int32 * 2), ("fast_probe_ms", C.c_float), ("slow_probe_ms", C.c_float),
                ("slab_bytes", C.c_uint64 * 2), ("live_bytes", C.c_uint64 * 2), ("slots_released", C.c_int32), ("peer_devices", C.c_int32),
                ("peak_slots", C.c_int32), ("rebased", C.c_int32)]


MEM_STATE, MEM_STREAM = 0, 1
SAMPLES_F32, SAMPLES_F16 = 0, 1     # statmc_accumulate_formats: what a stat type's sample arena holds


class StatType(C.Structure):
    _fields_ = [
        ("channels", C.c_int32), ("transform", C.c_int32), ("max_moment", C.c_int32),
        ("n_samples", C.c_int32), ("samples", C.c_void_p), ("n", C.c_void_p),
        ("mean", C.c_void_p), ("m2", C.c_void_p), ("m3", C.c_void_p),
        ("film_mean", C.c_void_p), ("film_m2", C.c_void_p),
        ("mean_corr", C.c_void_p), ("discriminator", C.c_void_p),
    ]


class RecordLayout(C.Structure):
    """statmc_record_layout: where in an interleaved record the pixel index and every stat type's values lie, and in which
    format (statmc_accumulate_records_interleaved)."""
    _fields_ = [("stride", C.c_int32), ("pixel_offset", C.c_int32), ("sample_offset", C.c_int32 * 16), ("sample_format", C.c_int32 * 16)]


class PrepassContext(C.Structure):
    """statmc_prepass_context: what a renderer's own kernel needs for the pre-pass store of statmc::device::PixelStats
    (include/statmc_device_api.hpp): the current device's t table (device pointer) and the epilogue's flags (1 Welch, 2 small n
    excluded)."""
    _fields_ = [("t_table", C.c_void_p), ("flags", C.c_int32), ("reserved", C.c_int32)]


class CombineEntry(C.Structure):
    """statmc_combine_entry: part A (dst, updated in place) and part B (src) of one set of statistics."""
    _fields_ = [("dst", StatType), ("src", StatType), ("count_of", C.c_int32)]


class CombineManyEntry(C.Structure):
    """statmc_combine_many_entry: part 0 (dst, updated in place) and a host array of further parts, in fold order."""
    _fields_ = [("dst", StatType), ("srcs", C.POINTER(StatType)), ("count_of", C.c_int32)]


class PoolEntry(C.Structure):
    """statmc_pool_entry: the coarse film (dst, written) and the fine film (src) of one set of statistics."""
    _fields_ = [("dst", StatType), ("src", StatType), ("count_of", C.c_int32)]


class PlanResult(C.Structure):
    """statmc_plan_result: what statmc_plan_samples writes to device memory next to the count image."""
    _fields_ = [("total", C.c_int64), ("budget", C.c_int64), ("level_bits", C.c_uint32), ("status", C.c_int32),
                ("n_live", C.c_int32), ("n_saturated", C.c_int32)]


class TargetResult(C.Structure):
    """statmc_target_result: what statmc_plan_to_target writes to device memory next to the count image (48 bytes)."""
    _fields_ = [("total", C.c_int64), ("need", C.c_int64), ("n_open", C.c_int64), ("n_capped", C.c_int64), ("n_unjudged", C.c_int64),
                ("n_live", C.c_int32), ("n_saturated", C.c_int32)]


SELECT_MAX_RANKS = 8


class SelectResult(C.Structure):
    """statmc_select_result: what statmc_score_select writes to device memory."""
    _fields_ = [("n_px", C.c_int64), ("n_live", C.c_int64), ("n_saturated", C.c_int64), ("n_ranks", C.c_int32), ("pad", C.c_int32),
                ("rank", C.c_int64 * SELECT_MAX_RANKS), ("value_bits", C.c_uint32 * SELECT_MAX_RANKS),
                ("n_below", C.c_int64 * SELECT_MAX_RANKS), ("n_equal", C.c_int64 * SELECT_MAX_RANKS)]


SUM_MAX_CAPS = 4


class SumResult(C.Structure):
    """statmc_sum_result: what statmc_score_sum writes to device memory (152 bytes)."""
    _fields_ = [("n_px", C.c_int64), ("n_zero", C.c_int64), ("n_finite", C.c_int64), ("n_infinite", C.c_int64), ("n_caps", C.c_int32), ("pad", C.c_int32),
                ("cap_bits", C.c_uint32 * SUM_MAX_CAPS), ("n_clipped", C.c_int64 * SUM_MAX_CAPS),
                ("sum", C.c_double * SUM_MAX_CAPS), ("sum_sq", C.c_double * SUM_MAX_CAPS)]


SCORE_TILES_MAX_TILE = 64
TILE_PLANES = ("sum", "sum_sq", "mean", "max", "n_px", "n_zero", "n_infinite", "n_clipped")      # statmc_tile_scores' fields, in its order


class TileScores(C.Structure):
    """statmc_tile_scores: a HOST struct of DEVICE pointers to the planes statmc_score_tiles writes; NULL: not formed."""
    _fields_ = [("sum", C.c_void_p), ("sum_sq", C.c_void_p), ("mean", C.c_void_p), ("max", C.c_void_p),
                ("n_px", C.c_void_p), ("n_zero", C.c_void_p), ("n_infinite", C.c_void_p), ("n_clipped", C.c_void_p)]


TILE_SELECT_MAX_RANKS = 4
TILE_SELECT_MAX_DEN = 65536
TILE_QUANTILE_FIELDS = ("value", "n_below", "n_equal")      # statmc_tile_quantiles' fields, in its order
GATE_MAX_IMAGES = 4


class TileQuantiles(C.Structure):
    """statmc_tile_quantiles: a HOST struct of DEVICE pointers to the planes statmc_score_tile_select writes, one per field and rank
    slot; NULL: not formed."""
    _fields_ = [("value", C.c_void_p * TILE_SELECT_MAX_RANKS), ("n_below", C.c_void_p * TILE_SELECT_MAX_RANKS),
                ("n_equal", C.c_void_p * TILE_SELECT_MAX_RANKS)]


class GateResult(C.Structure):
    """statmc_gate_result: what statmc_gate_tiles writes to device memory (32 bytes)."""
    _fields_ = [("n_tiles", C.c_int64), ("n_open", C.c_int64), ("n_closed_now", C.c_int64), ("n_px_open", C.c_int64)]


SCORE_ABSOLUTE, SCORE_RELATIVE = 0, 1     # statmc_sample_scores' metric
ERROR_NO_TABLE = -1                       # statmc_error_scores' table: the standard error, no quantile
SCORE_WINDOW_MAX, SCORE_WINDOW_MIN = 0, 1  # statmc_score_window's op
SCORE_WINDOW_MAX_RADIUS = 32
PLAN_LEVEL_LO, PLAN_LEVEL_HI = 0x20000000, 0x5F000000   # statmc_plan_samples' level range [U_LO, U_HI]: 2^-63 .. 2^63
PLAN_MAX_COUNT = 1 << 20
MAX_COMBINE_SOURCES = 15

EXPORTS = [
    "statmc_last_error", "statmc_setup", "statmc_device_cus", "statmc_set_device", "statmc_set_significance", "statmc_get_significance", "statmc_set_t_quantiles",
    "statmc_set_filter_spec", "statmc_get_filter_spec", "statmc_reset_filter_spec", "statmc_pinned_from", "statmc_copy_device_settings",
    "statmc_set_filter_split", "statmc_get_filter_split", "statmc_filter_split_auto",
    "statmc_malloc", "statmc_free", "statmc_malloc_placed", "statmc_placement_expect", "statmc_placement_info", "statmc_placement_map", "statmc_placement_trim", "statmc_malloc_host", "statmc_free_host", "statmc_memset", "statmc_upload", "statmc_download",
    "statmc_stream_create", "statmc_stream_create_with_priority", "statmc_stream_destroy", "statmc_synchronize",
    "statmc_event_create", "statmc_event_destroy", "statmc_event_record", "statmc_stream_wait_event",
    "statmc_filter_f32", "statmc_filter_f32x3", "statmc_prepass", "statmc_window_filter", "statmc_pack_filter_inputs", "statmc_prepass_pack", "statmc_prepass_pack_rows",
    "statmc_halo_exchange", "statmc_halo_exchange_rccl", "statmc_rccl_available", "statmc_rccl_unique_id", "statmc_rccl_comm_create", "statmc_rccl_comm_destroy", "statmc_copy_rect", "statmc_calculate_mean_vars", "statmc_accumulate", "statmc_accumulate_rows", "statmc_accumulate_row_ranges", "statmc_accumulate_formats", "statmc_accumulate_tiles", "statmc_accumulate_tiles_formats", "statmc_accumulate_counted", "statmc_accumulate_tiles_counted", "statmc_accumulate_records", "statmc_accumulate_records_interleaved", "statmc_accumulate_records_split", "statmc_accumulate_records_interleaved_split", "statmc_combine_statistics", "statmc_combine_many", "statmc_pool_statistics", "statmc_upsample_filtered", "statmc_sample_scores", "statmc_plan_samples_workspace", "statmc_plan_samples", "statmc_error_scores", "statmc_plan_to_target", "statmc_score_select_workspace", "statmc_score_select", "statmc_score_count_above", "statmc_score_sum_workspace", "statmc_score_sum", "statmc_score_tiles", "statmc_score_tile_select", "statmc_gate_tiles", "statmc_score_window", "statmc_compact_offsets_workspace", "statmc_compact_offsets", "statmc_compact_accumulate", "statmc_compact_accumulate_interleaved", "statmc_state_dwords", "statmc_gather_states", "statmc_combine_records", "statmc_get_prepass_context", "statmc_merge_tiles", "statmc_tile_moments", "statmc_film_update",
    "statmc_last_filter_variant", "statmc_version", "statmc_clock_probe",
]

_lib = None


def library_path():
    return _build.SO


def load():
    """Load libstatmc_hip.so.  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_build.SO):
        raise RuntimeError(
            "libstatmc_hip.so is missing (%s). Build it with `python -m statmc_amd.build` or "
            "__graft_entry__.build(); statmc_amd has no CPU/PyTorch fallback." % _build.SO)
    if _build.SO == _build.DEFAULT_SO and _build.stale():
        raise RuntimeError("libstatmc_hip.so was built from other sources than the ones in statmc_amd/csrc "
                           "(content hash mismatch): rebuild with `python -m statmc_amd.build` before using it")
    lib = C.CDLL(_build.SO)
    lib.statmc_last_error.restype = C.c_char_p
    lib.statmc_last_filter_variant.restype = C.c_char_p
    lib.statmc_pinned_from.restype = C.c_char_p
    lib.statmc_setup.argtypes = [C.c_int]
    lib.statmc_set_significance.argtypes = [C.c_int]
    lib.statmc_set_t_quantiles.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.statmc_set_filter_spec.argtypes = [C.POINTER(FilterSpec)]
    lib.statmc_get_filter_spec.argtypes = [C.POINTER(FilterSpec)]
    lib.statmc_copy_device_settings.argtypes = [C.c_int, C.c_int]
    lib.statmc_set_filter_split.argtypes = [C.c_int]
    lib.statmc_filter_split_auto.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.statmc_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.statmc_free.argtypes = [C.c_void_p]
    lib.statmc_malloc_placed.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]
    lib.statmc_placement_expect.argtypes = [C.c_int, C.c_size_t]
    lib.statmc_placement_info.argtypes = [C.POINTER(PlacementInfo)]
    lib.statmc_malloc_host.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.statmc_free_host.argtypes = [C.c_void_p]
    lib.statmc_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    lib.statmc_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.statmc_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.statmc_stream_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.statmc_stream_create_with_priority.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.statmc_stream_destroy.argtypes = [C.c_void_p]
    lib.statmc_event_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.statmc_event_destroy.argtypes = [C.c_void_p]
    lib.statmc_event_record.argtypes = [C.c_void_p, C.c_void_p]
    lib.statmc_stream_wait_event.argtypes = [C.c_void_p, C.c_void_p]
    lib.statmc_synchronize.argtypes = [C.c_void_p]
    lib.statmc_filter_f32.argtypes = [C.POINTER(FilterArgs)]
    lib.statmc_filter_f32x3.argtypes = [C.POINTER(FilterArgs)]
    lib.statmc_prepass.argtypes = [C.POINTER(FilterArgs), C.c_int]
    lib.statmc_window_filter.argtypes = [C.POINTER(FilterArgs), C.c_int]
    lib.statmc_pack_filter_inputs.argtypes = [C.POINTER(FilterArgs), C.POINTER(Image), C.c_int, C.c_int]
    lib.statmc_prepass_pack.argtypes = [C.POINTER(FilterArgs), C.POINTER(Image), C.c_int, C.c_int]
    lib.statmc_prepass_pack_rows.argtypes = [C.POINTER(FilterArgs), C.POINTER(Image), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.statmc_halo_exchange.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.statmc_halo_exchange_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.statmc_rccl_unique_id.argtypes = [C.c_void_p]
    lib.statmc_rccl_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    lib.statmc_rccl_comm_destroy.argtypes = [C.c_void_p]
    lib.statmc_copy_rect.argtypes = [C.POINTER(Image), C.c_int, C.c_int, C.c_int, C.POINTER(Image), C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.statmc_set_device.argtypes = [C.c_int]
    lib.statmc_calculate_mean_vars.argtypes = [C.c_uint8, C.c_uint16, C.c_uint16, C.c_int,
                                               C.POINTER(Image), C.POINTER(Image), C.POINTER(Image),
                                               C.c_int, C.c_void_p]
    lib.statmc_accumulate.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p]
    lib.statmc_accumulate_rows.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.statmc_accumulate_row_ranges.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p]
    lib.statmc_accumulate_formats.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                              C.c_void_p]
    lib.statmc_debug_last_accumulate_loader.restype = C.c_int
    lib.statmc_accumulate_tiles.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p]
    lib.statmc_accumulate_tiles_formats.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p]
    lib.statmc_accumulate_counted.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                              C.POINTER(C.c_int32), C.c_int, C.c_void_p]
    lib.statmc_accumulate_tiles_counted.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.statmc_debug_last_accumulate_counted.restype = C.c_int
    lib.statmc_accumulate_records.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.statmc_debug_accumulate_records_phases.argtypes = [C.c_int]
    lib.statmc_accumulate_records_interleaved.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.POINTER(RecordLayout),
                                                          C.c_int64, C.c_void_p]
    lib.statmc_accumulate_records_split.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.statmc_accumulate_records_interleaved_split.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.POINTER(RecordLayout),
                                                                C.c_int64, C.c_int32, C.c_void_p]
    lib.statmc_debug_accumulate_records_interleaved_path.argtypes = [C.c_int]
    lib.statmc_debug_last_accumulate_records_interleaved_path.restype = C.c_int
    lib.statmc_get_prepass_context.argtypes = [C.POINTER(PrepassContext)]
    lib.statmc_combine_statistics.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(CombineEntry), C.c_int, C.c_void_p]
    lib.statmc_combine_many.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(CombineManyEntry), C.c_int, C.c_int, C.c_void_p]
    lib.statmc_pool_statistics.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.POINTER(PoolEntry), C.c_int, C.c_void_p]
    lib.statmc_upsample_filtered.argtypes = [C.POINTER(FilterArgs), C.POINTER(FilterArgs), C.c_int, C.c_int]
    lib.statmc_sample_scores.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.statmc_plan_samples_workspace.argtypes = [C.c_uint16, C.c_uint16]
    lib.statmc_plan_samples_workspace.restype = C.c_size_t
    lib.statmc_plan_samples.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                        C.POINTER(PlanResult), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.statmc_score_select_workspace.argtypes = []
    lib.statmc_score_select_workspace.restype = C.c_size_t
    lib.statmc_score_select.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.POINTER(SelectResult), C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    lib.statmc_error_scores.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    lib.statmc_plan_to_target.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p,
                                          C.POINTER(TargetResult), C.c_void_p]
    lib.statmc_score_count_above.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]
    lib.statmc_score_sum_workspace.argtypes = []
    lib.statmc_score_sum_workspace.restype = C.c_size_t
    lib.statmc_score_sum.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(SumResult), C.c_void_p,
                                     C.c_size_t, C.c_void_p]
    lib.statmc_score_tiles.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_int, C.c_float, C.POINTER(TileScores), C.c_void_p]
    lib.statmc_score_tile_select.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int32, C.c_int,
                                             C.POINTER(TileQuantiles), C.c_void_p]
    lib.statmc_gate_tiles.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
    lib.statmc_score_window.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.statmc_compact_offsets_workspace.argtypes = [C.c_uint16, C.c_uint16]
    lib.statmc_compact_offsets_workspace.restype = C.c_size_t
    lib.statmc_compact_offsets.argtypes = [C.c_uint16, C.c_uint16, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                           C.c_void_p]
    lib.statmc_compact_accumulate.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int64,
                                              C.c_int32, C.c_void_p]
    lib.statmc_debug_compact_path.argtypes = [C.c_int]
    lib.statmc_debug_last_compact_path.restype = C.c_int
    lib.statmc_compact_accumulate_interleaved.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.POINTER(RecordLayout),
                                                          C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.statmc_debug_compact_interleaved_path.argtypes = [C.c_int]
    lib.statmc_debug_compact_interleaved_window.argtypes = [C.c_int]
    lib.statmc_debug_last_compact_interleaved_path.restype = C.c_int
    lib.statmc_state_dwords.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.statmc_state_dwords.restype = C.c_size_t
    lib.statmc_gather_states.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.c_void_p]
    lib.statmc_combine_records.argtypes = [C.c_uint16, C.c_uint16, C.POINTER(StatType), C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.c_int32,
                                           C.c_void_p]
    lib.statmc_merge_tiles.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p]
    lib.statmc_tile_moments.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]
    lib.statmc_film_update.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.statmc_clock_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.statmc_debug_force_filter_variant.argtypes = [C.c_int]
    lib.statmc_debug_force_filter_parts.argtypes = [C.c_int]
    lib.statmc_debug_last_filter_parts.restype = C.c_int
    lib.statmc_debug_accumulate_resident_blocks.argtypes = [C.c_int]
    lib.statmc_debug_accumulate_dma.argtypes = [C.c_int]
    lib.statmc_debug_accumulate_fused.argtypes = [C.c_int]
    lib.statmc_debug_last_accumulate_fused.restype = C.c_int
    _lib = lib
    return lib


def check(rc):
    if rc != STATMC_OK:
        raise StatmcError(rc, load().statmc_last_error().decode())
    return rc


_setup_done = set()


def setup(device=0):
    if device not in _setup_done:
        check(load().statmc_setup(int(device)))
        _setup_done.add(device)


def set_filter_spec(spec=None, **fields):
    """Filter spec of the current device: a FilterSpec, or its fields by keyword; no argument = the pinned default
    (and the pinned significance level)."""
    if spec is None and not fields:     # what a freshly set-up device has (include/statmc_pinned_spec.h)
        check(load().statmc_reset_filter_spec())
        return
    spec = spec if spec is not None else FilterSpec(**fields)
    check(load().statmc_set_filter_spec(C.byref(spec)))


def get_significance():
    """The current device's significance-level index (statmc_get_significance: 0 = 0.005, 1 = 0.002, 2 = 0.05)."""
    return int(load().statmc_get_significance())


def get_filter_spec():
    spec = FilterSpec()
    check(load().statmc_get_filter_spec(C.byref(spec)))
    return spec


def last_filter_variant():
    return load().statmc_last_filter_variant().decode()


def force_filter_variant(v):
    """0 auto, 1 generic (global-memory) kernel, 2 runtime-radius one-sided LDS kernel, 3 one-sided r = 20 LDS kernel.
    (include/statmc_debug.h; per device, like the two switches below)"""
    check(load().statmc_debug_force_filter_variant(int(v)))


def accumulate_resident_blocks(n):
    """0: by shape (default); n > 0: the accumulate kernel runs as n resident workgroups; -1: never a resident grid."""
    check(load().statmc_debug_accumulate_resident_blocks(int(n)))


def accumulate_dma(on):
    """1 (default): the RGB sample planes of the accumulation stream through LDS-DMA; 0: loads into registers (A/B, tests)."""
    check(load().statmc_debug_accumulate_dma(int(on)))


def last_accumulate_loader():
    """How the calling thread's last film-major accumulation read its 16-bit arenas: 0 it had none, 1 the vector path, 2 element by
    element."""
    return int(load().statmc_debug_last_accumulate_loader())


def accumulate_fused(mode):
    """The accumulation's type-fused walk: 0 by shape (default), 1 whenever the launch is eligible, -1 never (A/B, tests)."""
    check(load().statmc_debug_accumulate_fused(int(mode)))


def last_accumulate_fused():
    """1 if the calling thread's last film-major accumulation ran the type-fused walk, else 0."""
    return int(load().statmc_debug_last_accumulate_fused())


def force_filter_parts(k):
    """0 automatic; k >= 1: the LDS kernels sweep the window with k workgroups per tile (= set_filter_split)."""
    check(load().statmc_set_filter_split(int(k)))


def set_filter_split(parts):
    """Window-sweep split of the current device: 0 = automatic (fitted to the local image and the device), k >= 1 = pinned.
    Calls with the same split reproduce each other bit for bit whatever the image shape (include/statmc.h)."""
    check(load().statmc_set_filter_split(int(parts)))


def get_filter_split():
    return int(load().statmc_get_filter_split())


def filter_split_auto(width, height, radius):
    """What the automatic choice picks on the current device for a whole image of this size."""
    k = int(load().statmc_filter_split_auto(int(width), int(height), int(radius)))
    if k < 0:
        check(k)
    return k


# ------------------------------------------------------------------ torch marshalling
def _torch():
    import torch
    return torch


def current_stream_handle():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def image_of(t):
    """Describe a [H, W] or [H, W, C] device tensor as a statmc_image: packed, or with a row pitch (a view such as
    padded[:, :W] of a wider tensor -- what a cv::cuda::GpuMat allocated with a pitch looks like)."""
    assert t.is_cuda and t.element_size() == 4
    h, w = t.shape[0], t.shape[1]
    c = t.shape[2] if t.dim() == 3 else 1
    inner = (t.stride(1) == c and t.stride(2) == 1) if t.dim() == 3 else t.stride(1) == 1
    assert inner and t.stride(0) >= w * c, "device images must have packed pixels and a row pitch of at least one row"
    return Image(C.c_void_p(t.data_ptr()), t.stride(0) * 4, w, h)


def _img_array(tensors):
    arr = (Image * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = image_of(t)
    return arr


def make_filter_args(n, mean, m2, m3, film, mean_corr, disc, film_filtered, g_buffers, g_sds=None,
                     g_dr=None, filter_sd=10.0, radius=20, denoise_film=False, film_buffer=None,
                     film_filtered_buffer=None, roi=None, stream=None, keep=None, packed=None, film_origin=None,
                     packed_g_channels=None):
    """Build a statmc_filter_args from lists of per-buffer device tensors (reference argument
    order, estimator.cpp:437-459).  Returns (args, keepalive).  packed: optional [H, W, 15 | 16 | 17]
    block + halo tensor the window filter reads instead of the separate images (16: + the sample count, for Welch degrees
    of freedom; 17: packed_g_channels
    names the channel count of every G-buffer in it, e.g. [3, 3, 1, 1], one g_sds / g_dr entry each)."""
    tables = [mean_corr, mean, film, film_filtered, n]
    nb = max(len(t) for t in tables) if packed is None else 1
    ref = next(t[0] for t in tables if t) if packed is None else packed
    h, w = ref.shape[0], ref.shape[1]
    a = FilterArgs()
    ka = []
    a.n_buffers, a.width, a.height = nb, w, h
    a.filter_ds_factor = -0.5 / (filter_sd * filter_sd)   # estimator.h:259
    a.filter_radius = radius
    a.denoise_film = 1 if denoise_film else 0
    for name, lst in (("n", n), ("mean", mean), ("m2", m2), ("m3", m3), ("film", film),
                      ("mean_corr", mean_corr), ("discriminator", disc), ("film_filtered", film_filtered)):
        if lst:
            arr = _img_array(lst)
            ka.append(arr)
            setattr(a, name, arr)
    if film_buffer is not None:
        a.film_buffer = image_of(film_buffer)
    if film_filtered_buffer is not None:
        a.film_filtered_buffer = image_of(film_filtered_buffer)
    ng = len(g_buffers)
    if ng:
        garr = _img_array(g_buffers)
        gch = (C.c_uint8 * ng)(*[(g.shape[2] if g.dim() == 3 else 1) for g in g_buffers])
        if g_dr is None:
            g_dr = [-0.5 / (sd * sd) for sd in g_sds]      # estimator.cpp:16
        gdr = (C.c_float * ng)(*g_dr)
        ka += [garr, gch, gdr]
        a.g_buffers, a.g_channel_counts, a.g_dr_factors = garr, gch, gdr
    a.n_g_buffers = ng
    if packed is not None:
        pch = packed.shape[2]
        a.packed_inputs = Image(C.c_void_p(packed.data_ptr()), w * pch * 4, w, h)
        if g_dr is None:
            g_dr = [-0.5 / (sd * sd) for sd in g_sds]
        gch_list = list(packed_g_channels) if packed_g_channels is not None else [3] * len(g_dr)
        assert len(gch_list) == len(g_dr)
        gdr = (C.c_float * len(g_dr))(*g_dr)
        gch = (C.c_uint8 * len(g_dr))(*gch_list)
        ka += [gdr, gch]
        a.g_dr_factors, a.g_channel_counts, a.n_g_buffers = gdr, gch, len(g_dr)
    a.stream = stream if stream is not None else current_stream_handle()
    if roi is not None:
        a.roi_x0, a.roi_y0, a.roi_x1, a.roi_y1 = roi
    if film_origin is not None:   # film coordinates of local pixel (0, 0): block + halo images of the multi-GPU path
        a.film_x0, a.film_y0 = film_origin
    ka.append((n, mean, m2, m3, film, mean_corr, disc, film_filtered, g_buffers, film_buffer,
               film_filtered_buffer, packed))
    return a, ka


def prepass(args, channels):
    check(load().statmc_prepass(C.byref(args), channels))


def window_filter(args, channels):
    check(load().statmc_window_filter(C.byref(args), channels))


def pack_filter_inputs(args, packed, dst_x0, dst_y0):
    """Owned block of the five filter inputs -> [Hp, Wp, 15 | 16 | 17] block + halo tensor at (dst_x0, dst_y0)."""
    img = image_of(packed)
    check(load().statmc_pack_filter_inputs(C.byref(args), C.byref(img), dst_x0, dst_y0))


def prepass_pack(args, packed, dst_x0, dst_y0, rows=None):
    """Pre-pass of buffer 0 + pack of the five filter inputs in one pass (mean_corr / discriminator are
    also written to their own images when the args carry them).  rows: one or two (y0, y1) ranges of the block -- only
    those rows, in one launch."""
    img = image_of(packed)
    if rows is None:
        check(load().statmc_prepass_pack(C.byref(args), C.byref(img), dst_x0, dst_y0))
    else:
        flat = (C.c_int32 * (2 * len(rows)))(*[int(v) for r in rows for v in r])
        check(load().statmc_prepass_pack_rows(C.byref(args), C.byref(img), dst_x0, dst_y0, flat, len(rows)))


def filter_f32x3(args):
    check(load().statmc_filter_f32x3(C.byref(args)))


def filter_f32(args):
    check(load().statmc_filter_f32(C.byref(args)))


class _PlacedBlock:
    """A statmc_malloc_placed block seen by torch through __cuda_array_interface__; freed (statmc_free) when the last
    tensor that aliases it goes away."""

    def __init__(self, nbytes, role, shape, typestr):
        p = C.c_void_p()
        check(load().statmc_malloc_placed(C.byref(p), max(int(nbytes), 1), int(role)))
        self.ptr = p.value
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (self.ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self.ptr:
                load().statmc_free(C.c_void_p(self.ptr))
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass
        self.ptr = None


def empty_placed(shape, dtype, device, role):
    """torch tensor on `device` in memory placed by HBM rank (include/statmc.h: statmc_malloc_placed): role MEM_STATE for
    the images a launch reads and writes (the running moments), MEM_STREAM for read-once sample arenas.  Uninitialised."""
    import torch
    typestr = {torch.float32: "<f4", torch.float16: "<f2", torch.int32: "<i4", torch.uint8: "|u1", torch.int64: "<i8"}[dtype]
    n = 1
    for d in shape:
        n *= int(d)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(idx):
        blk = _PlacedBlock(n * torch.empty((), dtype=dtype).element_size(), role, shape if n else (0,), typestr)
        if n == 0:
            return torch.empty(shape, dtype=dtype, device=device)
        return torch.as_tensor(blk, device=device)


def placement_expect(role, nbytes, device=None):
    """Announces the bytes about to be asked for in `role` (include/statmc.h: the class search is budgeted, and the arenas' class chosen, for all
    of them at once)."""
    import torch
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    with torch.cuda.device(idx):
        check(load().statmc_placement_expect(int(role), int(nbytes)))


def zeros_placed(shape, dtype, device, role):
    return empty_placed(shape, dtype, device, role).zero_()


def placement_info():
    info = PlacementInfo()
    check(load().statmc_placement_info(C.byref(info)))
    out = {k: (list(getattr(info, k)) if k in ("slots_as_they_came", "slab_bytes", "live_bytes") else getattr(info, k)) for k, _ in PlacementInfo._fields_}
    buf = C.create_string_buffer(1024)
    check(load().statmc_placement_map(buf, 1024))
    out["map"] = buf.value.decode()
    return out


class RcclComm:
    """An RCCL communicator made through the C ABI (statmc_rccl_unique_id / statmc_rccl_comm_create): what a multi-process C++
    host uses for statmc_halo_exchange_rccl.  rank 0 makes the id (RcclComm.unique_id()), the host hands its 128 bytes to the
    other ranks by its own means, every rank constructs RcclComm(n_ranks, rank, id) on its device (collective)."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(load().statmc_rccl_unique_id(buf))
        return buf.raw

    def __init__(self, n_ranks, rank, id128):
        assert len(id128) == 128
        self.n_ranks, self.rank = n_ranks, rank
        self.handle = C.c_void_p()
        check(load().statmc_rccl_comm_create(C.byref(self.handle), n_ranks, rank, C.c_char_p(id128)))

    def destroy(self):
        if self.handle:
            check(load().statmc_rccl_comm_destroy(self.handle))
            self.handle = C.c_void_p()


def halo_exchange_rccl(packed, device_index, gx, gy, block_w, block_h, radius, comm, stream=None):
    """statmc_halo_exchange_rccl on this rank's block + halo image `packed` ([rows, cols, channels] device tensor)."""
    from .peer import Block
    blk = Block()
    blk.device = device_index
    blk.packed = image_of(packed)
    blk.stream = stream if stream is not None else current_stream_handle()
    check(load().statmc_halo_exchange_rccl(C.byref(blk), gx, gy, block_w, block_h, radius, comm.handle, comm.rank))


def placement_trim():
    """Releases the idle slots of the current device's placed allocator (statmc_placement_trim); returns how many."""
    n = load().statmc_placement_trim()
    if n < 0:
        check(n)
    return n


def make_stat_type(samples, state, transform, max_moment, prepass_into=None):
    """samples: [S, H, W, C] device tensor; state: dict of device tensors n/mean/m2/m3/film_mean/film_m2.
    prepass_into = (mean_corr, discriminator): the accumulation's epilogue also writes the pre-pass of the updated moments there
    (statmc_stat_type::mean_corr / discriminator; max_moment 3)."""
    t = StatType()
    c = samples.shape[3] if samples.dim() == 4 else 1
    t.channels, t.transform, t.max_moment = c, int(bool(transform)), int(max_moment)
    t.n_samples = samples.shape[0]
    t.samples = samples.data_ptr()
    t.n = state["n"].data_ptr()
    t.mean = state["mean"].data_ptr()
    t.m2 = state["m2"].data_ptr() if state.get("m2") is not None else None
    t.m3 = state["m3"].data_ptr() if state.get("m3") is not None else None
    t.film_mean = state["film_mean"].data_ptr() if state.get("film_mean") is not None else None
    t.film_m2 = state["film_m2"].data_ptr() if state.get("film_m2") is not None else None
    if prepass_into is not None:
        t.mean_corr, t.discriminator = prepass_into[0].data_ptr(), prepass_into[1].data_ptr()
    return t


def _state_side(state, channels, max_moment, own_counts):
    t = StatType()
    t.channels, t.max_moment = int(channels), int(max_moment)
    ptr = lambda k: state[k].data_ptr() if state.get(k) is not None else None
    t.n = ptr("n") if own_counts else None
    t.mean, t.m2, t.m3 = ptr("mean"), ptr("m2"), ptr("m3")
    t.film_mean, t.film_m2 = ptr("film_mean"), ptr("film_m2")
    return t


def make_combine_entry(dst, src, channels, max_moment, count_of=-1, prepass_into=None):
    """One statmc_combine_entry: dst / src are state dicts of device tensors (n, mean, m2, m3, film_mean, film_m2; a missing
    or None entry is not passed).  count_of = k >= 0: weigh with entry k's counts as they were before the call (dst / src
    "n" are not passed then).  prepass_into = (mean_corr, discriminator): the call's epilogue writes the pre-pass of the
    combined moments there (max_moment 3, own counts)."""
    e = CombineEntry()
    own = count_of < 0
    e.dst = _state_side(dst, channels, max_moment, own)
    e.src = _state_side(src, channels, max_moment, own)
    e.count_of = -1 if own else int(count_of)
    if prepass_into is not None:
        e.dst.mean_corr, e.dst.discriminator = prepass_into[0].data_ptr(), prepass_into[1].data_ptr()
    return e


def prepass_context():
    """statmc_get_prepass_context of the current device: query again after set_significance / set_filter_spec."""
    ctx = PrepassContext()
    check(load().statmc_get_prepass_context(C.byref(ctx)))
    return ctx


def combine_statistics(width, height, entries, stream=None):
    """statmc_combine_statistics: every entry's src statistics into its dst, in one launch (include/statmc.h)."""
    arr = (CombineEntry * max(len(entries), 1))(*entries)
    check(load().statmc_combine_statistics(int(width), int(height), arr, len(entries),
                                           stream if stream is not None else current_stream_handle()))


def make_combine_many_entry(dst, srcs, channels, max_moment, count_of=-1, prepass_into=None):
    """One statmc_combine_many_entry: dst and every element of `srcs` are state dicts as for make_combine_entry; srcs is
    the fold order.  The entry keeps its array of source descriptors alive (`_srcs`, `_n_sources` of them)."""
    e = CombineManyEntry()
    own = count_of < 0
    e.dst = _state_side(dst, channels, max_moment, own)
    arr = (StatType * max(len(srcs), 1))(*[_state_side(s, channels, max_moment, own) for s in srcs])
    e._srcs, e._n_sources = arr, len(srcs)
    e.srcs = C.cast(arr, C.POINTER(StatType))
    e.count_of = -1 if own else int(count_of)
    if prepass_into is not None:
        e.dst.mean_corr, e.dst.discriminator = prepass_into[0].data_ptr(), prepass_into[1].data_ptr()
    return e


def combine_many(width, height, entries, n_sources=None, stream=None):
    """statmc_combine_many: every entry's sources into its dst, a left fold in source order, in one pass over memory
    (include/statmc.h).  n_sources defaults to the length of the entries' source lists, which must agree."""
    if n_sources is None:
        counts = set(getattr(e, "_n_sources", 0) for e in entries)
        if len(counts) > 1:
            raise ValueError("combine_many: the entries have different numbers of sources (%s)" % sorted(counts))
        n_sources = counts.pop() if counts else 0
    arr = (CombineManyEntry * max(len(entries), 1))(*entries)
    check(load().statmc_combine_many(int(width), int(height), arr, len(entries), int(n_sources),
                                     stream if stream is not None else current_stream_handle()))


def pooled_size(width, height, k):
    """The coarse film of statmc_pool_statistics: (ceil(width / k), ceil(height / k))."""
    return -(-int(width) // int(k)), -(-int(height) // int(k))


def make_pool_entry(dst, src, channels, max_moment, count_of=-1, prepass_into=None):
    """One statmc_pool_entry: dst (the coarse film, written) and src (the fine film) are state dicts of device tensors as for
    make_combine_entry.  count_of = q >= 0: every merge is weighed with entry q's fine counts ("n" is not passed then).
    prepass_into = (mean_corr, discriminator) of the coarse size: the epilogue writes the pre-pass of the pooled moments there
    (max_moment 3, own counts)."""
    e = PoolEntry()
    own = count_of < 0
    e.dst = _state_side(dst, channels, max_moment, own)
    e.src = _state_side(src, channels, max_moment, own)
    e.count_of = -1 if own else int(count_of)
    if prepass_into is not None:
        e.dst.mean_corr, e.dst.discriminator = prepass_into[0].data_ptr(), prepass_into[1].data_ptr()
    return e


def pool_statistics(width, height, k, entries, stream=None):
    """statmc_pool_statistics: the statistics of every k x k block of the width x height film in every entry's src pooled into
    one pixel of its dst, in one launch (include/statmc.h: the Morton-ordered tree of two-part combines; k = 2, 4 or 8)."""
    arr = (PoolEntry * max(len(entries), 1))(*entries)
    check(load().statmc_pool_statistics(int(width), int(height), int(k), arr, len(entries),
                                        stream if stream is not None else current_stream_handle()))


def upsample_filtered(fine_args, coarse_args, k, channels):
    """The filtered image of the film pooled k x k (coarse_args: after its pre-pass and window filter) onto the fine film's filtered
    image (fine_args: after its pre-pass), by statmc_upsample_filtered: one launch per buffer on fine_args.stream, the fine film is
    only read.  Both blocks are make_filter_args'."""
    check(load().statmc_upsample_filtered(C.byref(fine_args), C.byref(coarse_args), int(k), int(channels)))


_METRICS = {"absolute": SCORE_ABSOLUTE, "relative": SCORE_RELATIVE}


def sample_scores(n, film_mean, film_m2, metric="relative", eps=1e-3, out=None, stream=None):
    """statmc_sample_scores: the per-pixel noise score of the running statistics n [H, W] int32 and film_mean / film_m2 [H, W, C]
    float32 (C = 1 or 3; a [H, W] image is one channel) -- "absolute": the sample standard deviation summed over the channels'
    variances; "relative": that over eps + sum |film_mean|; +inf where n < 2.  Returns the float32 score image [H, W] (`out`, or a new
    tensor)."""
    tc = _torch()
    h, w = int(n.shape[0]), int(n.shape[1])
    ch = int(film_mean.shape[2]) if film_mean.dim() == 3 else 1
    for name, t, dt in (("n", n, tc.int32), ("film_mean", film_mean, tc.float32), ("film_m2", film_m2, tc.float32)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("sample_scores: %s must be a contiguous %s CUDA tensor" % (name, dt))
    if film_mean.numel() != h * w * ch or film_m2.numel() != h * w * ch:
        raise ValueError("sample_scores: film_mean and film_m2 must hold [H, W, C] = [%d, %d, %d] values" % (h, w, ch))
    if out is None:
        out = tc.empty(h, w, dtype=tc.float32, device=n.device)
    elif out.dtype != tc.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != h * w:
        raise ValueError("sample_scores: out must be a contiguous float32 CUDA tensor of H * W values")
    m = _METRICS[metric] if isinstance(metric, str) else int(metric)
    check(load().statmc_sample_scores(w, h, ch, m, float(eps), n.data_ptr(), film_mean.data_ptr(), film_m2.data_ptr(), out.data_ptr(),
                                      stream if stream is not None else current_stream_handle()))
    return out


def plan_samples_workspace(width, height):
    """statmc_plan_samples_workspace: the bytes of workspace statmc_plan_samples wants for a width x height film (no device needed)."""
    return int(load().statmc_plan_samples_workspace(int(width), int(height)))


_plan_scratch = {}    # (device index, stream handle) -> (workspace, result): alive while kernels of that stream may still use them


def plan_result_dict(result):
    """The statmc_plan_result a plan_samples call wrote into the int64 [4] device tensor `result`, as a dict (a device-to-host copy:
    synchronises with the work that wrote it on the current stream; after a call on another stream synchronise that one first)."""
    r = PlanResult.from_buffer_copy(result.cpu().numpy().tobytes())
    return {k: int(getattr(r, k)) for k, _ in PlanResult._fields_}


def plan_samples(score, budget, c_min, c_max, n=None, out=None, workspace=None, result=None, stream=None, return_result=False):
    """statmc_plan_samples: spends `budget` samples over the film by the float32 score image [H, W] -- n + counts proportional to the
    score, every count in [c_min, c_max], the sum equal to the budget to the sample wherever the bounds allow it (include/statmc.h).
    n: int32 [H, W] counts so far, None = 0 everywhere.  Returns the int32 count image [H, W] (`out`, or a new tensor): what
    accumulate(..., sample_counts=) takes as it is.  Asynchronous; workspace (uint8, at least plan_samples_workspace bytes) and result
    (int64 [4], the statmc_plan_result's 32 bytes) are the caller's or, if None, tensors kept per (device, stream) until the next call on
    that stream.  return_result=True: waits for the call and returns (counts, result as a dict)."""
    tc = _torch()
    if score.dtype != tc.float32 or not score.is_cuda or not score.is_contiguous() or score.dim() != 2:
        raise ValueError("plan_samples: score must be a contiguous float32 CUDA tensor [H, W]")
    h, w = int(score.shape[0]), int(score.shape[1])
    if n is not None and (n.dtype != tc.int32 or not n.is_cuda or not n.is_contiguous() or n.numel() != h * w):
        raise ValueError("plan_samples: n must be a contiguous int32 CUDA tensor of H * W counts")
    if out is None:
        out = tc.empty(h, w, dtype=tc.int32, device=score.device)
    else:
        _counts_pointer(out, w, h, "plan_samples")
    st = stream if stream is not None else current_stream_handle()
    need = plan_samples_workspace(w, h)
    if workspace is None or result is None:
        key = (score.device.index, st.value if hasattr(st, "value") else int(st or 0))
        held = _plan_scratch.get(key)
        if held is None or held[0].numel() < need:
            held = (tc.empty(need, dtype=tc.uint8, device=score.device), tc.empty(4, dtype=tc.int64, device=score.device))
            _plan_scratch[key] = held
        workspace = workspace if workspace is not None else held[0]
        result = result if result is not None else held[1]
    check(load().statmc_plan_samples(w, h, score.data_ptr(), n.data_ptr() if n is not None else None, int(budget), int(c_min), int(c_max),
                                     out.data_ptr(), C.cast(result.data_ptr(), C.POINTER(PlanResult)), workspace.data_ptr(),
                                     workspace.numel() * workspace.element_size(), st))
    if not return_result:
        return out
    check(load().statmc_synchronize(st))
    return out, plan_result_dict(result)


_ERRORS = {"stderr": ERROR_NO_TABLE}    # "ci": the two-sided table at the device's significance level (error_table)


def error_table(error):
    """statmc_error_scores' `table` of an error kind: "stderr" -> ERROR_NO_TABLE; "ci" -> the two-sided table at the current device's
    significance level (get_significance(): the two-sided tables are 0..2); an int -1..5 is taken as it is."""
    if error == "ci":
        return get_significance()
    if isinstance(error, str):
        if error not in _ERRORS:
            raise ValueError("error must be None, \"stderr\", \"ci\" or a table index, not %r" % (error,))
        return _ERRORS[error]
    return int(error)


def error_scores(n, film_mean, film_m2, metric="relative", eps=1e-3, table=ERROR_NO_TABLE, out=None, stream=None):
    """statmc_error_scores: the per-pixel error of the mean of the running statistics n [H, W] int32 and film_mean / film_m2 [H, W, C]
    float32 (C = 1 or 3) -- table ERROR_NO_TABLE (or "stderr"): the standard error sqrt(v / n); table 0..5 (alpha_index + 3 * sides; or
    "ci": two-sided at the device's significance level): that times the device's Student-t quantile at n - 1 degrees of freedom, the
    half-width of the confidence interval; "relative": over eps + sum |film_mean|; +inf where n < 2.  Returns the float32 image [H, W]
    (`out`, or a new tensor): what plan_to_target, score_window, score_select and score_count_above take."""
    tc = _torch()
    h, w = int(n.shape[0]), int(n.shape[1])
    ch = int(film_mean.shape[2]) if film_mean.dim() == 3 else 1
    for name, t, dt in (("n", n, tc.int32), ("film_mean", film_mean, tc.float32), ("film_m2", film_m2, tc.float32)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("error_scores: %s must be a contiguous %s CUDA tensor" % (name, dt))
    if film_mean.numel() != h * w * ch or film_m2.numel() != h * w * ch:
        raise ValueError("error_scores: film_mean and film_m2 must hold [H, W, C] = [%d, %d, %d] values" % (h, w, ch))
    if out is None:
        out = tc.empty(h, w, dtype=tc.float32, device=n.device)
    elif out.dtype != tc.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != h * w:
        raise ValueError("error_scores: out must be a contiguous float32 CUDA tensor of H * W values")
    m = _METRICS[metric] if isinstance(metric, str) else int(metric)
    check(load().statmc_error_scores(w, h, ch, m, float(eps), error_table(table), n.data_ptr(), film_mean.data_ptr(), film_m2.data_ptr(),
                                     out.data_ptr(), stream if stream is not None else current_stream_handle()))
    return out


_TARGET_WORDS = C.sizeof(TargetResult) // 8
_target_scratch = {}    # (device index, stream handle) -> result, as _plan_scratch


def target_result_dict(result):
    """The statmc_target_result a plan_to_target call wrote into the int64 [6] device tensor `result`, as a dict (a device-to-host
    copy: synchronises with the work that wrote it on the current stream; after a call on another stream synchronise that one first)."""
    r = TargetResult.from_buffer_copy(result.cpu().numpy().tobytes())
    return {k: int(getattr(r, k)) for k, _ in TargetResult._fields_}


def plan_to_target(error, n, target, c_min, c_max, out=None, result=None, stream=None, return_result=False):
    """statmc_plan_to_target: per pixel the samples that bring the float32 error image [H, W] (error_scores', a window of it, or a
    metric of the renderer's that falls like 1 / sqrt(n)) to `target`, n (error / target)^2 - n clamped to [c_min, c_max]; c_min where
    the error is at the target already, c_max where nobody can judge the pixel yet (include/statmc.h).  n: int32 [H, W] counts so far.
    Returns the int32 count image [H, W] (`out`, or a new tensor): what accumulate(..., sample_counts=) takes as it is.  Asynchronous;
    result (int64 [6], the statmc_target_result's 48 bytes) is the caller's or, if None, a tensor kept per (device, stream) until the
    next call on that stream.  return_result=True: waits for the call and returns (counts, result as a dict)."""
    tc = _torch()
    h, w = _score_image(error, "plan_to_target")
    if n is None or n.dtype != tc.int32 or not n.is_cuda or not n.is_contiguous() or n.numel() != h * w:
        raise ValueError("plan_to_target: n must be a contiguous int32 CUDA tensor of H * W counts")
    if out is None:
        out = tc.empty(h, w, dtype=tc.int32, device=error.device)
    else:
        _counts_pointer(out, w, h, "plan_to_target")
    st = stream if stream is not None else current_stream_handle()
    if result is None:
        key = (error.device.index, st.value if hasattr(st, "value") else int(st or 0))
        result = _target_scratch.get(key)
        if result is None:
            result = _target_scratch[key] = tc.empty(_TARGET_WORDS, dtype=tc.int64, device=error.device)
    if result.dtype != tc.int64 or not result.is_cuda or not result.is_contiguous() or result.numel() < _TARGET_WORDS:
        raise ValueError("plan_to_target: result must be a contiguous int64 CUDA tensor of %d words" % _TARGET_WORDS)
    check(load().statmc_plan_to_target(w, h, error.data_ptr(), n.data_ptr(), float(target), int(c_min), int(c_max), out.data_ptr(),
                                       C.cast(result.data_ptr(), C.POINTER(TargetResult)), st))
    if not return_result:
        return out
    check(load().statmc_synchronize(st))
    return out, target_result_dict(result)


def score_select_workspace():
    """statmc_score_select_workspace: the bytes of workspace statmc_score_select wants, for every film size (no device needed)."""
    return int(load().statmc_score_select_workspace())


_SELECT_WORDS = C.sizeof(SelectResult) // 8
_select_scratch = {}    # (device index, stream handle) -> (workspace, result), as _plan_scratch


def _score_image(score, what):
    tc = _torch()
    if score.dtype != tc.float32 or not score.is_cuda or not score.is_contiguous() or score.dim() != 2:
        raise ValueError("%s: score must be a contiguous float32 CUDA tensor [H, W]" % what)
    return int(score.shape[0]), int(score.shape[1])


def read_select_result(t):
    """The statmc_select_result a score_select call wrote into the int64 [32] device tensor `t`, as a dict whose per-rank fields are
    lists of n_ranks entries; "values" are value_bits as numpy float32.  One small device-to-host copy: it synchronises with the work
    that wrote `t` on the current stream; after a call on another stream synchronise that one first."""
    import numpy as np
    r = SelectResult.from_buffer_copy(t.cpu().numpy().tobytes())
    k = int(r.n_ranks)
    out = {f: int(getattr(r, f)) for f in ("n_px", "n_live", "n_saturated", "n_ranks")}
    for f in ("rank", "value_bits", "n_below", "n_equal"):
        out[f] = [int(v) for v in getattr(r, f)[:k]]
    out["values"] = np.array(out["value_bits"], np.uint32).view(np.float32)
    return out


def score_select(score, ranks, workspace=None, result=None, stream=None):
    """statmc_score_select: the ranks[i]-th smallest keys (0-based; 1 to 8 ranks, any order) of the float32 score image [H, W], with
    the number of pixels below and equal to each, and the class counts (include/statmc.h).  Returns the device result, an int64 [32]
    tensor holding the statmc_select_result's 256 bytes: read_select_result(t) downloads it.  Asynchronous; workspace (uint8, at
    least score_select_workspace() bytes) and result are the caller's or, if None, tensors kept per (device, stream) until the next
    call on that stream."""
    tc = _torch()
    h, w = _score_image(score, "score_select")
    ranks = [int(r) for r in ranks]
    st = stream if stream is not None else current_stream_handle()
    if workspace is None or result is None:
        key = (score.device.index, st.value if hasattr(st, "value") else int(st or 0))
        held = _select_scratch.get(key)
        if held is None:
            held = (tc.empty(score_select_workspace(), dtype=tc.uint8, device=score.device),
                    tc.empty(_SELECT_WORDS, dtype=tc.int64, device=score.device))
            _select_scratch[key] = held
        workspace = workspace if workspace is not None else held[0]
        result = result if result is not None else held[1]
    if result.dtype != tc.int64 or not result.is_cuda or not result.is_contiguous() or result.numel() < _SELECT_WORDS:
        raise ValueError("score_select: result must be a contiguous int64 CUDA tensor of %d words" % _SELECT_WORDS)
    arr = (C.c_int64 * max(len(ranks), 1))(*ranks)
    check(load().statmc_score_select(w, h, score.data_ptr(), arr, len(ranks), C.cast(result.data_ptr(), C.POINTER(SelectResult)),
                                     workspace.data_ptr(), workspace.numel() * workspace.element_size(), st))
    return result


def score_count_above(score, thresholds, out=None, stream=None):
    """statmc_score_count_above: per threshold (1 to 8, none NaN) the number of pixels of the float32 score image [H, W] whose key is
    above the threshold's (include/statmc.h).  Returns the int64 device tensor [len(thresholds)] (`out`, or a new one).
    Asynchronous."""
    tc = _torch()
    h, w = _score_image(score, "score_count_above")
    thresholds = [float(t) for t in thresholds]
    if out is None:
        out = tc.empty(max(len(thresholds), 1), dtype=tc.int64, device=score.device)[:len(thresholds)]
    elif out.dtype != tc.int64 or not out.is_cuda or not out.is_contiguous() or out.numel() != len(thresholds):
        raise ValueError("score_count_above: out must be a contiguous int64 CUDA tensor of one count per threshold")
    arr = (C.c_float * max(len(thresholds), 1))(*thresholds)
    check(load().statmc_score_count_above(w, h, score.data_ptr(), arr, len(thresholds), out.data_ptr() if out.numel() else None,
                                          stream if stream is not None else current_stream_handle()))
    return out


def score_sum_workspace():
    """statmc_score_sum_workspace: the bytes of workspace statmc_score_sum wants, for every film size (no device needed)."""
    return int(load().statmc_score_sum_workspace())


_SUM_WORDS = C.sizeof(SumResult) // 8
_sum_scratch = {}    # (device index, stream handle) -> (workspace, result), as _plan_scratch


def read_sum_result(t):
    """The statmc_sum_result a score_sum call wrote into the int64 [19] device tensor `t`, as a dict whose per-cap fields are lists
    of n_caps entries: "sum" and "sum_sq" as Python floats (the doubles, bit for bit), "caps" the caps' keys as numpy float32.  One
    small device-to-host copy: it synchronises with the work that wrote `t` on the current stream; after a call on another stream
    synchronise that one first."""
    import numpy as np
    r = SumResult.from_buffer_copy(t.cpu().numpy().tobytes())
    k = int(r.n_caps)
    out = {f: int(getattr(r, f)) for f in ("n_px", "n_zero", "n_finite", "n_infinite", "n_caps")}
    for f in ("cap_bits", "n_clipped"):
        out[f] = [int(v) for v in getattr(r, f)[:k]]
    for f in ("sum", "sum_sq"):
        out[f] = [float(v) for v in getattr(r, f)[:k]]
    out["caps"] = np.array(out["cap_bits"], np.uint32).view(np.float32)
    return out


def score_sum(score, caps, workspace=None, result=None, stream=None):
    """statmc_score_sum: per cap (1 to 4, none NaN, any order; +inf: no cap, the +inf pixels are left out) the exact sum and sum of
    squares of min(score, cap) over the float32 score image [H, W], each rounded once to a double, with the number of pixels above
    the cap and the class counts (include/statmc.h).  Returns the device result, an int64 [19] tensor holding the statmc_sum_result's
    152 bytes: read_sum_result(t) downloads it.  Asynchronous; workspace (uint8, at least score_sum_workspace() bytes) and result are
    the caller's or, if None, tensors kept per (device, stream) until the next call on that stream."""
    tc = _torch()
    h, w = _score_image(score, "score_sum")
    caps = [float(c) for c in caps]
    st = stream if stream is not None else current_stream_handle()
    if workspace is None or result is None:
        key = (score.device.index, st.value if hasattr(st, "value") else int(st or 0))
        held = _sum_scratch.get(key)
        if held is None:
            held = (tc.empty(score_sum_workspace(), dtype=tc.uint8, device=score.device),
                    tc.empty(_SUM_WORDS, dtype=tc.int64, device=score.device))
            _sum_scratch[key] = held
        workspace = workspace if workspace is not None else held[0]
        result = result if result is not None else held[1]
    if result.dtype != tc.int64 or not result.is_cuda or not result.is_contiguous() or result.numel() < _SUM_WORDS:
        raise ValueError("score_sum: result must be a contiguous int64 CUDA tensor of %d words" % _SUM_WORDS)
    arr = (C.c_float * max(len(caps), 1))(*caps)
    check(load().statmc_score_sum(w, h, score.data_ptr(), arr, len(caps), C.cast(result.data_ptr(), C.POINTER(SumResult)),
                                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), st))
    return result


def tile_grid(height, width, tile):
    """(tiles_y, tiles_x) of statmc_score_tiles' planes for a film of height x width pixels"""
    tile = int(tile)
    return -(-int(height) // tile), -(-int(width) // tile)


def _tile_plane_dtypes():
    tc = _torch()
    return {"sum": tc.float64, "sum_sq": tc.float64, "mean": tc.float32, "max": tc.float32,
            "n_px": tc.int32, "n_zero": tc.int32, "n_infinite": tc.int32, "n_clipped": tc.int32}


def score_tiles(score, tile, cap=float("inf"), planes=TILE_PLANES, out=None, stream=None):
    """statmc_score_tiles: per tile x tile block (8, 16, 32 or 64; partial blocks at the right and bottom edges included) of the
    float32 score image [H, W] the exact sum and sum of squares of min(score, cap) as doubles, their mean as a correctly rounded
    float32, the maximum key, and the counts of pixels, of key 0, of +inf and above the cap (include/statmc.h).  cap = +inf: no cap,
    the +inf pixels are left out of sum, sum_sq and mean.  Returns {name: device tensor [tiles_y, tiles_x]} for the names in
    `planes` (TILE_PLANES' names; a plane not named is not formed); `out` may hand in the tensors to write, contiguous and of
    tile_grid's shape.  "mean" and "max" are score images that score_select, score_count_above, score_window and plan_samples take;
    "n_clipped" is a count image that compact_offsets(..., cap=1) turns into the list of open tiles.  Asynchronous: one launch,
    no workspace."""
    tc = _torch()
    h, w = _score_image(score, "score_tiles")
    planes = tuple(planes)
    dtypes = _tile_plane_dtypes()
    for p in planes:
        if p not in dtypes:
            raise ValueError("score_tiles: no plane %r: one of %s" % (p, ", ".join(TILE_PLANES)))
    shape = tile_grid(h, w, tile) if int(tile) > 0 else (0, 0)
    res, ptrs = {}, TileScores()
    for p in planes:
        t = None if out is None else out.get(p)
        if t is None:
            t = tc.empty(shape, dtype=dtypes[p], device=score.device)
        elif t.dtype != dtypes[p] or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError("score_tiles: out[%r] must be a contiguous %s CUDA tensor of shape %s" % (p, dtypes[p], shape))
        res[p] = t
        setattr(ptrs, p, t.data_ptr() if t.numel() else None)
    check(load().statmc_score_tiles(w, h, score.data_ptr(), int(tile), float(cap), C.byref(ptrs),
                                    stream if stream is not None else current_stream_handle()))
    return res


def read_tile_scores(res):
    """The planes a score_tiles call returned, as numpy arrays of the same shapes and types.  Small device-to-host copies: they
    synchronise with the work that wrote them on the current stream; after a call on another stream synchronise that one first."""
    return {p: t.cpu().numpy() for p, t in res.items()}


def tile_quantile_fraction(q):
    """(num, den) of a quantile given as a (num, den) pair or as a float in [0, 1]: a float goes through
    Fraction(q).limit_denominator(65536), so 0.95 is 19/20 and 0.5 is 1/2."""
    from fractions import Fraction
    if isinstance(q, (tuple, list)):
        num, den = int(q[0]), int(q[1])
    else:
        f = Fraction(float(q)).limit_denominator(TILE_SELECT_MAX_DEN)
        num, den = f.numerator, f.denominator
    return num, den


def score_tile_select(score, tile, nums, den, fields=TILE_QUANTILE_FIELDS, out=None, stream=None):
    """statmc_score_tile_select: per tile x tile block (8, 16, 32 or 64; partial blocks at the edges included) of the float32 score
    image [H, W] and per quantile nums[i] / den (1 to 4 of them; 1 <= den <= 65536, 0 <= nums[i] <= den) the key at the nearest rank
    max(0, ceil(n nums[i] / den) - 1) of the block's n pixels, with the number of the block's pixels below and equal to it
    (include/statmc.h).  Returns {field: [device tensor [tiles_y, tiles_x] per quantile]} for the fields named ("value" float32,
    "n_below" and "n_equal" int32; a field not named is not formed); `out` may hand in the tensors to write in the same shape of
    dict, a None entry being left out.  The "value" planes are score images that score_count_above, score_select, score_window,
    plan_samples and gate_tiles take.  Asynchronous: one launch, no workspace."""
    tc = _torch()
    h, w = _score_image(score, "score_tile_select")
    nums = [int(v) for v in nums]
    fields = tuple(fields)
    for f in fields:
        if f not in TILE_QUANTILE_FIELDS:
            raise ValueError("score_tile_select: no field %r: one of %s" % (f, ", ".join(TILE_QUANTILE_FIELDS)))
    if len(nums) > TILE_SELECT_MAX_RANKS:
        raise ValueError("score_tile_select: %d quantiles: 1 to %d" % (len(nums), TILE_SELECT_MAX_RANKS))
    shape = tile_grid(h, w, tile) if int(tile) > 0 else (0, 0)
    res, ptrs = {}, TileQuantiles()
    for f in fields:
        res[f] = []
        for i in range(len(nums)):
            t = None if out is None or f not in out else out[f][i]
            if t is None and out is not None and f in out:
                res[f].append(None)
                continue
            dtype = tc.float32 if f == "value" else tc.int32
            if t is None:
                t = tc.empty(shape, dtype=dtype, device=score.device)
            elif t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError("score_tile_select: out[%r][%d] must be a contiguous %s CUDA tensor of shape %s" % (f, i, dtype, shape))
            res[f].append(t)
            getattr(ptrs, f)[i] = t.data_ptr() if t.numel() else None
    arr = (C.c_int32 * max(len(nums), 1))(*nums)
    check(load().statmc_score_tile_select(w, h, score.data_ptr(), int(tile), arr, int(den), len(nums), C.byref(ptrs),
                                          stream if stream is not None else current_stream_handle()))
    return res


def read_tile_quantiles(res):
    """The planes a score_tile_select call returned, as numpy arrays in the same dict of lists (None stays None).  Small device-to-host
    copies: they synchronise with the work that wrote them on the current stream; after a call on another stream synchronise that one
    first."""
    return {f: [None if t is None else t.cpu().numpy() for t in ts] for f, ts in res.items()}


_GATE_WORDS = C.sizeof(GateResult) // 8


def gate_tiles(height, width, tile, tile_value, threshold, closed=None, open=None, images=(), out=None, result=None, stream=None):
    """statmc_gate_tiles: the tiles of the height x width film whose tile_value (a float32 plane of tile_grid's shape, e.g. a
    score_tile_select "value" plane) is above `threshold` by score_count_above's rule, and that `closed` (an int32 plane, updated in
    place; None: no memory) has not closed before, are open; `images` (0 to 4 contiguous [H, W] tensors of 4-byte elements, float32
    scores and int32 counts alike) are copied with the pixels of every other tile set to the all-zero word (include/statmc.h).  `out`:
    the tensors to write, one per image, the image itself for in place; None: new tensors.  Returns (open int32 [tiles_y, tiles_x],
    the gated images as a list, the device result: an int64 [4] tensor read by read_gate_result).  A closed tile never reopens: start
    `closed` from zeros.  Asynchronous: two launches."""
    tc = _torch()
    shape = tile_grid(height, width, tile) if int(tile) > 0 else (0, 0)
    dev = tile_value.device
    if tile_value.dtype != tc.float32 or not tile_value.is_cuda or not tile_value.is_contiguous() or tuple(tile_value.shape) != shape:
        raise ValueError("gate_tiles: tile_value must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    if open is None:
        open = tc.empty(shape, dtype=tc.int32, device=dev)
    for name, t in (("closed", closed), ("open", open)):
        if t is not None and (t.dtype != tc.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape):
            raise ValueError("gate_tiles: %s must be a contiguous int32 CUDA tensor of shape %s" % (name, shape))
    images = list(images)
    outs = list(out) if out is not None else [tc.empty_like(im) for im in images]
    if len(outs) != len(images):
        raise ValueError("gate_tiles: out must hold one tensor per image")
    for name, ts in (("images", images), ("out", outs)):
        for i, t in enumerate(ts):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4 or t.numel() != int(height) * int(width):
                raise ValueError("gate_tiles: %s[%d] must be a contiguous CUDA tensor of H * W 4-byte elements" % (name, i))
    if result is None:
        result = tc.empty(_GATE_WORDS, dtype=tc.int64, device=dev)
    elif result.dtype != tc.int64 or not result.is_cuda or not result.is_contiguous() or result.numel() < _GATE_WORDS:
        raise ValueError("gate_tiles: result must be a contiguous int64 CUDA tensor of %d words" % _GATE_WORDS)
    k = len(images)
    src = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in images])
    dst = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in outs])
    check(load().statmc_gate_tiles(int(width), int(height), int(tile), tile_value.data_ptr(), float(threshold),
                                   closed.data_ptr() if closed is not None else None, open.data_ptr() if open.numel() else None,
                                   src if k else None, dst if k else None, k, result.data_ptr(),
                                   stream if stream is not None else current_stream_handle()))
    return open, outs, result


def read_gate_result(t):
    """The statmc_gate_result a gate_tiles call wrote into the int64 [4] device tensor `t`, as a dict of Python integers.  One small
    device-to-host copy: it synchronises with the work that wrote `t` on the current stream; after a call on another stream
    synchronise that one first."""
    r = GateResult.from_buffer_copy(t.cpu().numpy().tobytes())
    return {f: int(getattr(r, f)) for f, _ in GateResult._fields_}


_WINDOW_OPS = {"max": SCORE_WINDOW_MAX, "min": SCORE_WINDOW_MIN}


def score_window(score, radius, op="max", out=None, stream=None):
    """statmc_score_window: per pixel the maximum ("max": a dilation) or minimum ("min": an erosion) of the keys of the float32 score
    image [H, W] over the pixels within `radius` (0 to SCORE_WINDOW_MAX_RADIUS) to every side, the border clipped (include/statmc.h).
    Returns the float32 image [H, W] (`out`, or a new tensor; never `score` itself): what plan_samples, score_select and
    score_count_above take as score.  score_window(score_window(s, r, "min"), r) is the opening, which drops isolated spikes first.
    Asynchronous."""
    tc = _torch()
    h, w = _score_image(score, "score_window")
    if out is None:
        out = tc.empty(h, w, dtype=tc.float32, device=score.device)
    elif out.dtype != tc.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != h * w:
        raise ValueError("score_window: out must be a contiguous float32 CUDA tensor of H * W values")
    o = _WINDOW_OPS[op] if isinstance(op, str) else int(op)
    check(load().statmc_score_window(w, h, score.data_ptr(), o, int(radius), out.data_ptr(),
                                     stream if stream is not None else current_stream_handle()))
    return out


def make_stat_type_arena(arena, channels, state, transform, max_moment, prepass_into=None):
    """Stat type whose samples arrive tile by tile (accumulate_tiles): `arena` is a flat device tensor, torch.float32 or -- with
    SAMPLES_F16 as the type's entry of accumulate_tiles' sample_formats -- torch.float16."""
    torch = _torch()
    if arena.dtype not in (torch.float32, torch.float16):
        raise ValueError("make_stat_type_arena: the arena is torch.float32 or torch.float16, not %s" % arena.dtype)
    t = make_stat_type(arena.view(1, 1, -1, 1), state, transform, max_moment, prepass_into=prepass_into)
    t.channels, t.n_samples = int(channels), 0
    return t


def _counts_pointer(sample_counts, width, height, who):
    """The address of a per-pixel count image: an int32 CUDA tensor of height * width elements, packed (a view that starts
    anywhere in a larger tensor is fine -- the entry wants 4-byte alignment, the vector path 16)."""
    tc = _torch()
    if sample_counts.dtype != tc.int32 or not sample_counts.is_cuda or not sample_counts.is_contiguous():
        raise ValueError("%s: sample_counts must be a contiguous int32 CUDA tensor" % who)
    if sample_counts.numel() != int(width) * int(height):
        raise ValueError("%s: sample_counts holds %d counts, the film %d pixels" % (who, sample_counts.numel(), int(width) * int(height)))
    return sample_counts.data_ptr()


def last_accumulate_counted():
    """statmc_debug_last_accumulate_counted: 0 = the calling thread's last accumulate call launched no counted kernel, 1 = a counted
    kernel on the vector path, 2 = a counted kernel element by element."""
    return int(load().statmc_debug_last_accumulate_counted())


def accumulate(width, height, stat_types, stream=None, rows=None, sample_formats=None, sample_counts=None):
    """rows = (y0, y1): only those rows of the film (statmc_accumulate_rows); rows = [(y0, y1), ...]: several disjoint
    ranges in one launch (statmc_accumulate_row_ranges).  sample_formats = [SAMPLES_F32 | SAMPLES_F16, ...], one per stat
    type: what each type's sample arena holds (statmc_accumulate_formats).  sample_counts = int32 CUDA tensor [height, width]:
    pixel p folds its first min(max(count, 0), n_samples) samples only (statmc_accumulate_counted)."""
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    st = stream if stream is not None else current_stream_handle()
    if sample_formats is not None or sample_counts is not None:
        fmts = None
        if sample_formats is not None:
            if len(sample_formats) != len(stat_types):
                raise ValueError("accumulate: one sample format per stat type")
            fmts = (C.c_int32 * max(len(stat_types), 1))(*[int(f) for f in sample_formats])
        if rows is None:
            flat, n_ranges = None, 0
        else:
            if len(rows) == 2 and not hasattr(rows[0], "__len__"):
                rows = [rows]
            flat, n_ranges = (C.c_int32 * (2 * len(rows)))(*[int(v) for r in rows for v in r]), len(rows)
        if sample_counts is not None:
            check(load().statmc_accumulate_counted(width, height, arr, fmts, len(stat_types), _counts_pointer(sample_counts, width, height, "accumulate"),
                                                   flat, n_ranges, st))
        else:
            check(load().statmc_accumulate_formats(width, height, arr, fmts, len(stat_types), flat, n_ranges, st))
    elif rows is None:
        check(load().statmc_accumulate(width, height, arr, len(stat_types), st))
    elif len(rows) == 2 and not hasattr(rows[0], "__len__"):
        check(load().statmc_accumulate_rows(width, height, arr, len(stat_types), int(rows[0]), int(rows[1]), st))
    else:
        flat = (C.c_int32 * (2 * len(rows)))(*[int(v) for r in rows for v in r])
        check(load().statmc_accumulate_row_ranges(width, height, arr, len(stat_types), flat, len(rows), st))


def accumulate_tiles(width, height, stat_types, tile_bounds, tile_offsets, tile_samples, stream=None, sample_formats=None, sample_counts=None):
    """stat_types: make_stat_type_arena(arena, ...) per type, `arena` a flat device tensor holding the
    tiles' sample blocks; tile_bounds int32 [n,4], tile_offsets int64 [n] (pixel-samples),
    tile_samples int32 [n]: device tensors.  sample_formats = [SAMPLES_F32 | SAMPLES_F16, ...], one per stat type: what each
    type's arena holds (statmc_accumulate_tiles_formats); None: fp32 arenas, the existing entry.  sample_counts = int32 CUDA
    tensor [height, width] indexed by film pixel: a pixel folds its first min(max(count, 0), tile_samples) samples only
    (statmc_accumulate_tiles_counted)."""
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    st = stream if stream is not None else current_stream_handle()
    if sample_counts is not None:
        fmts = None
        if sample_formats is not None:
            if len(sample_formats) != len(stat_types):
                raise ValueError("accumulate_tiles: one sample format per stat type")
            fmts = (C.c_int32 * max(len(stat_types), 1))(*[int(f) for f in sample_formats])
        check(load().statmc_accumulate_tiles_counted(width, height, arr, fmts, len(stat_types), tile_bounds.data_ptr(), tile_offsets.data_ptr(),
                                                     tile_samples.data_ptr(), tile_bounds.shape[0],
                                                     _counts_pointer(sample_counts, width, height, "accumulate_tiles"), st))
        return
    if sample_formats is None:
        check(load().statmc_accumulate_tiles(width, height, arr, len(stat_types), tile_bounds.data_ptr(),
                                             tile_offsets.data_ptr(), tile_samples.data_ptr(), tile_bounds.shape[0], st))
        return
    if len(sample_formats) != len(stat_types):
        raise ValueError("accumulate_tiles: one sample format per stat type")
    fmts = (C.c_int32 * max(len(stat_types), 1))(*[int(f) for f in sample_formats])
    check(load().statmc_accumulate_tiles_formats(width, height, arr, fmts, len(stat_types), tile_bounds.data_ptr(),
                                                 tile_offsets.data_ptr(), tile_samples.data_ptr(), tile_bounds.shape[0], st))


def make_stat_type_records(samples, channels, state, transform, max_moment, prepass_into=None):
    """Stat type whose samples arrive as records (accumulate_records): `samples` is a record-major fp32 device tensor,
    [n_records, channels] or flat; record i's values are samples[i * channels : (i + 1) * channels]."""
    if not samples.is_contiguous():   # the descriptor holds the address: a reshaped copy would be gone before the call
        raise ValueError("make_stat_type_records: samples must be contiguous")
    return make_stat_type_arena(samples.view(-1), channels, state, transform, max_moment, prepass_into=prepass_into)


RECORDS_SPLIT_LANES = 64          # STATMC_RECORDS_SPLIT_LANES
RECORDS_SPLIT_DEFAULT = 256       # STATMC_RECORDS_SPLIT_DEFAULT (include/statmc.h; measured: DESIGN.md 4.1f)


def accumulate_records(width, height, stat_types, pixels, stream=None, split_above=None):
    """statmc_accumulate_records (include/statmc.h): `pixels` is an int32 device tensor, one entry per record (y * width + x;
    anything outside the film marks a skipped record); every stat type (make_stat_type_records) holds one sample per record.
    Per pixel the records are folded in ascending record index: the bits of statmc_accumulate after the same samples.
    split_above = k: statmc_accumulate_records_split -- a pixel with more than k records is folded by the 64 lanes of a wave
    (64 chunks, merged in a fixed tree: the same statistics, other last bits); None: the sequential entry."""
    tc = _torch()
    if pixels.dtype != tc.int32 or not pixels.is_contiguous():
        raise ValueError("accumulate_records: pixels must be a contiguous int32 tensor")
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    stream = stream if stream is not None else current_stream_handle()
    if split_above is None:
        check(load().statmc_accumulate_records(int(width), int(height), arr, len(stat_types), pixels.data_ptr(), pixels.numel(), stream))
    else:
        check(load().statmc_accumulate_records_split(int(width), int(height), arr, len(stat_types), pixels.data_ptr(), pixels.numel(),
                                                     int(split_above), stream))


RECORDS_PATH_AUTO, RECORDS_PATH_GENERAL, RECORDS_PATH_FUSED = 0, 1, 2


def make_stat_type_record_field(channels, state, transform, max_moment, prepass_into=None):
    """Stat type of accumulate_records_interleaved: the state images only -- where its values lie in a record is the layout's to say."""
    t = StatType()
    t.channels, t.transform, t.max_moment = int(channels), int(bool(transform)), int(max_moment)
    t.n = state["n"].data_ptr()
    t.mean = state["mean"].data_ptr()
    t.m2 = state["m2"].data_ptr() if state.get("m2") is not None else None
    t.m3 = state["m3"].data_ptr() if state.get("m3") is not None else None
    t.film_mean = state["film_mean"].data_ptr() if state.get("film_mean") is not None else None
    t.film_m2 = state["film_m2"].data_ptr() if state.get("film_m2") is not None else None
    if prepass_into is not None:
        t.mean_corr, t.discriminator = prepass_into[0].data_ptr(), prepass_into[1].data_ptr()
    return t


def make_record_layout(stride, pixel_offset, sample_offsets, sample_formats=None):
    """statmc_record_layout from plain numbers: one offset (and format, default fp32) per stat type, in the order of the types."""
    lay = RecordLayout()
    lay.stride, lay.pixel_offset = int(stride), int(pixel_offset)
    if len(sample_offsets) > 16:
        raise ValueError("make_record_layout: at most 16 stat types")
    formats = [SAMPLES_F32] * len(sample_offsets) if sample_formats is None else list(sample_formats)
    if len(formats) != len(sample_offsets):
        raise ValueError("make_record_layout: one format per offset")
    for i, (o, f) in enumerate(zip(sample_offsets, formats)):
        lay.sample_offset[i], lay.sample_format[i] = int(o), int(f)
    return lay


def pack_records(pixels, fields, formats=None, stride=None, pixel_offset=0, offsets=None, fill=0):
    """Interleaves numpy arrays into one record buffer (host side; the tests and tools/time_accumulate_records.py use it).
    pixels: int32 [n]; fields: per stat type a float array [n, C] (or [n]); formats: SAMPLES_F32 | SAMPLES_F16 per field (a half
    field is rounded to IEEE half here).  offsets: the byte offset of every field; default: the fields behind the pixel index
    in the order given, each at the next multiple of its element size.  stride: default the end of the last field rounded up to 4.
    Bytes no field covers hold `fill`.  Returns (records uint8 [n * stride], RecordLayout)."""
    import numpy as np
    pixels = np.ascontiguousarray(pixels, dtype=np.int32)
    n = pixels.size
    formats = [SAMPLES_F32] * len(fields) if formats is None else list(formats)
    cols = []
    for f, fmt in zip(fields, formats):
        a = np.ascontiguousarray(f, dtype=np.float16 if fmt == SAMPLES_F16 else np.float32)
        a = a.reshape(n, a.shape[1] if a.ndim == 2 else 1)      # (n = 0 cannot infer the channels)
        cols.append(a.view(np.uint8).reshape(n, a.shape[1] * a.itemsize))
    if offsets is None:
        offsets, at = [], pixel_offset + 4
        for c, fmt in zip(cols, formats):
            elem = 2 if fmt == SAMPLES_F16 else 4
            at = (at + elem - 1) // elem * elem
            offsets.append(at)
            at += c.shape[1]
    end = max([pixel_offset + 4] + [o + c.shape[1] for o, c in zip(offsets, cols)])
    if stride is None:
        stride = (end + 3) // 4 * 4
    if end > stride:
        raise ValueError("pack_records: a field ends at byte %d, behind the stride %d" % (end, stride))
    rec = np.full((n, stride), fill, dtype=np.uint8)
    for o, c in zip(offsets, cols):       # later fields win where fields overlap: hand an overlapping pair the same values
        rec[:, o:o + c.shape[1]] = c
    rec[:, pixel_offset:pixel_offset + 4] = pixels.view(np.uint8).reshape(n, 4)
    return rec.reshape(-1), make_record_layout(stride, pixel_offset, offsets, formats)


def accumulate_records_interleaved(width, height, stat_types, records, layout, n_records=None, stream=None, split_above=None):
    """statmc_accumulate_records_interleaved (include/statmc.h): `records` is a contiguous uint8 or int32 device tensor of
    n_records records of layout.stride bytes each (default: as many as the tensor holds); stat_types from
    make_stat_type_record_field, in the order of the layout's fields.  The bits of accumulate_records on the de-interleaved arrays.
    split_above = k: statmc_accumulate_records_interleaved_split (the bits of accumulate_records(..., split_above=k) on those arrays)."""
    tc = _torch()
    if records.dtype not in (tc.uint8, tc.int32) or not records.is_contiguous():
        raise ValueError("accumulate_records_interleaved: records must be a contiguous uint8 or int32 tensor")
    nbytes = records.numel() * records.element_size()
    if n_records is None:
        n_records = nbytes // layout.stride if layout.stride > 0 else 0
    elif int(n_records) * layout.stride > nbytes:
        raise ValueError("accumulate_records_interleaved: %d records of %d bytes do not fit the tensor (%d bytes)" % (n_records, layout.stride, nbytes))
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    stream = stream if stream is not None else current_stream_handle()
    if split_above is None:
        check(load().statmc_accumulate_records_interleaved(int(width), int(height), arr, len(stat_types), records.data_ptr(), C.byref(layout),
                                                           int(n_records), stream))
    else:
        check(load().statmc_accumulate_records_interleaved_split(int(width), int(height), arr, len(stat_types), records.data_ptr(), C.byref(layout),
                                                                 int(n_records), int(split_above), stream))


def accumulate_records_interleaved_path(path):
    """statmc_debug_accumulate_records_interleaved_path: RECORDS_PATH_AUTO | _GENERAL | _FUSED (where eligible)."""
    check(load().statmc_debug_accumulate_records_interleaved_path(int(path)))


def last_accumulate_records_interleaved_path():
    """The fold the calling thread's last accumulate_records_interleaved planned: RECORDS_PATH_GENERAL | _FUSED (0: none)."""
    return int(load().statmc_debug_last_accumulate_records_interleaved_path())


INT32_MAX = 2 ** 31 - 1
COMPACT_PATH_AUTO, COMPACT_PATH_STAGED, COMPACT_PATH_DIRECT, COMPACT_PATH_SPLIT = 0, 1, 2, 4   # include/statmc_debug.h


def compact_offsets_workspace(width, height):
    """statmc_compact_offsets_workspace: the bytes of workspace statmc_compact_offsets wants for a width x height film (no device needed)."""
    return int(load().statmc_compact_offsets_workspace(int(width), int(height)))


_compact_scratch = {}    # (device index, stream handle) -> workspace: alive while kernels of that stream may still use it


def compact_offsets(counts, cap=None, owners_capacity=0, out=None, workspace=None, stream=None):
    """statmc_compact_offsets: the int32 count image [H, W] (statmc_plan_samples' or the renderer's own) -> (offsets, owners).
    offsets: int64 [H * W + 1], the exclusive prefix sum of min(max(counts, 0), cap) in raster order (cap None: no cap), the last
    entry the total, which stays on the device.  owners: int32 [owners_capacity], slot i's pixel, -1 at and behind the total (None
    with owners_capacity 0): a pixels[] for accumulate_records.  out = (offsets, owners) to write into the caller's tensors.
    Asynchronous; the workspace (uint8, compact_offsets_workspace bytes) is the caller's or one kept per (device, stream)."""
    tc = _torch()
    if counts.dim() != 2:
        raise ValueError("compact_offsets: counts must be an int32 CUDA tensor [H, W]")
    h, w = int(counts.shape[0]), int(counts.shape[1])
    _counts_pointer(counts, w, h, "compact_offsets")
    offsets, owners = out if out is not None else (None, None)
    owners_capacity = int(owners_capacity)
    if offsets is None:
        offsets = tc.empty(h * w + 1, dtype=tc.int64, device=counts.device)
    elif offsets.dtype != tc.int64 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() != h * w + 1:
        raise ValueError("compact_offsets: offsets must be a contiguous int64 CUDA tensor of H * W + 1 entries")
    if owners is None and owners_capacity > 0:
        owners = tc.empty(owners_capacity, dtype=tc.int32, device=counts.device)
    elif owners is not None and (owners.dtype != tc.int32 or not owners.is_cuda or not owners.is_contiguous() or owners.numel() < owners_capacity):
        raise ValueError("compact_offsets: owners must be a contiguous int32 CUDA tensor of at least owners_capacity entries")
    st = stream if stream is not None else current_stream_handle()
    need = compact_offsets_workspace(w, h)
    if workspace is None:
        key = (counts.device.index, st.value if hasattr(st, "value") else int(st or 0))
        workspace = _compact_scratch.get(key)
        if workspace is None or workspace.numel() < need:
            workspace = _compact_scratch[key] = tc.empty(need, dtype=tc.uint8, device=counts.device)
    check(load().statmc_compact_offsets(w, h, counts.data_ptr(), INT32_MAX if cap is None else int(cap), offsets.data_ptr(),
                                        owners.data_ptr() if owners is not None else None, owners_capacity, workspace.data_ptr(),
                                        workspace.numel() * workspace.element_size(), st))
    return offsets, owners


def make_stat_type_compact(samples, channels, state, transform, max_moment, prepass_into=None):
    """Stat type whose samples lie in a compact arena (compact_accumulate): `samples` is a contiguous sample-major device tensor,
    [n_samples, channels] or flat, torch.float32 or -- with SAMPLES_F16 as the type's sample format -- torch.float16."""
    if not samples.is_contiguous():   # the descriptor holds the address: a reshaped copy would be gone before the call
        raise ValueError("make_stat_type_compact: samples must be contiguous")
    t = make_stat_type_arena(samples.view(-1), channels, state, transform, max_moment, prepass_into=prepass_into)
    t.n_samples = min(samples.numel() // int(channels), INT32_MAX)   # ignored by the entry: compact_accumulate's default n_samples
    return t


def compact_accumulate(width, height, stat_types, offsets, n_samples=None, sample_formats=None, split_above=None, stream=None):
    """statmc_compact_accumulate (include/statmc.h): pixel p folds positions [offsets[p], offsets[p + 1]) -- clamped into
    [0, n_samples) -- of every stat type's arena (make_stat_type_compact) in ascending order: the bits of accumulate_records on the
    same samples.  offsets: int64 CUDA tensor of width * height + 1 entries (compact_offsets).  n_samples: the arenas' length in
    samples; None: the shortest of the tensors make_stat_type_compact was given (arenas beyond 2^31 - 1 samples: pass it).
    sample_formats = [SAMPLES_F32 | SAMPLES_F16, ...] per stat type (None: fp32).  split_above: a run of more samples is
    folded by the 64 lanes of a wave (the bits of accumulate_records(..., split_above=)); None: RECORDS_SPLIT_DEFAULT."""
    tc = _torch()
    if offsets.dtype != tc.int64 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() != int(width) * int(height) + 1:
        raise ValueError("compact_accumulate: offsets must be a contiguous int64 CUDA tensor of width * height + 1 entries")
    if n_samples is None:
        n_samples = min([int(t.n_samples) for t in stat_types], default=0)
        if n_samples == INT32_MAX:
            raise ValueError("compact_accumulate: arenas this long need n_samples given")
    fmts = None
    if sample_formats is not None:
        if len(sample_formats) != len(stat_types):
            raise ValueError("compact_accumulate: one sample format per stat type")
        fmts = (C.c_int32 * max(len(stat_types), 1))(*[int(f) for f in sample_formats])
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    check(load().statmc_compact_accumulate(int(width), int(height), arr, fmts, len(stat_types), offsets.data_ptr(), int(n_samples),
                                           RECORDS_SPLIT_DEFAULT if split_above is None else int(split_above),
                                           stream if stream is not None else current_stream_handle()))


def compact_path(path):
    """statmc_debug_compact_path: COMPACT_PATH_AUTO | _STAGED | _DIRECT."""
    check(load().statmc_debug_compact_path(int(path)))


def last_compact_path():
    """What the calling thread's last compact_accumulate launched: COMPACT_PATH_STAGED or _DIRECT, plus COMPACT_PATH_SPLIT when the
    call's split_above was below INT32_MAX (0: nothing)."""
    return int(load().statmc_debug_last_compact_path())


COMPACT_ILV_PATH_AUTO, COMPACT_ILV_PATH_FUSED_STAGED, COMPACT_ILV_PATH_FUSED_DIRECT, COMPACT_ILV_PATH_GENERAL, COMPACT_ILV_PATH_SPLIT = 0, 1, 2, 3, 4   # include/statmc_debug.h


def compact_accumulate_interleaved(width, height, stat_types, records, layout, offsets, n_records=None, split_above=None, stream=None):
    """statmc_compact_accumulate_interleaved (include/statmc.h): `records` is a contiguous uint8 or int32 device tensor of n_records
    records of layout.stride bytes each (default: as many as the tensor holds), pixel p's at slots [offsets[p], offsets[p + 1]) --
    clamped into [0, n_records) --; stat_types from make_stat_type_record_field, in the order of the layout's fields
    (make_record_layout; its pixel_offset is ignored).  offsets: int64 CUDA tensor of width * height + 1 entries (compact_offsets).
    The bits of compact_accumulate on the de-interleaved arenas.  split_above: None = RECORDS_SPLIT_DEFAULT."""
    tc = _torch()
    if records.dtype not in (tc.uint8, tc.int32) or not records.is_contiguous() or (records.numel() and not records.is_cuda):
        raise ValueError("compact_accumulate_interleaved: records must be a contiguous uint8 or int32 CUDA tensor")
    if offsets.dtype != tc.int64 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() != int(width) * int(height) + 1:
        raise ValueError("compact_accumulate_interleaved: offsets must be a contiguous int64 CUDA tensor of width * height + 1 entries")
    nbytes = records.numel() * records.element_size()
    if n_records is None:
        n_records = nbytes // layout.stride if layout.stride > 0 else 0
    elif int(n_records) * layout.stride > nbytes:
        raise ValueError("compact_accumulate_interleaved: %d records of %d bytes do not fit the tensor (%d bytes)" % (n_records, layout.stride, nbytes))
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    check(load().statmc_compact_accumulate_interleaved(int(width), int(height), arr, len(stat_types), records.data_ptr(), C.byref(layout),
                                                       offsets.data_ptr(), int(n_records),
                                                       RECORDS_SPLIT_DEFAULT if split_above is None else int(split_above),
                                                       stream if stream is not None else current_stream_handle()))


def compact_interleaved_path(path):
    """statmc_debug_compact_interleaved_path: COMPACT_ILV_PATH_AUTO | _FUSED_STAGED | _FUSED_DIRECT | _GENERAL."""
    check(load().statmc_debug_compact_interleaved_path(int(path)))


def compact_interleaved_window(nbytes):
    """statmc_debug_compact_interleaved_window: the staged kernel's LDS bytes per wave (a multiple of 1024 up to 65536; 0: the default)."""
    check(load().statmc_debug_compact_interleaved_window(int(nbytes)))


def last_compact_interleaved_path():
    """What the calling thread's last compact_accumulate_interleaved launched: COMPACT_ILV_PATH_FUSED_STAGED, _FUSED_DIRECT or
    _GENERAL, plus COMPACT_ILV_PATH_SPLIT when the call's split_above was below INT32_MAX (0: nothing)."""
    return int(load().statmc_debug_last_compact_interleaved_path())


def state_dwords(channels, max_moment, transform):
    """statmc_state_dwords: the dwords of one state record of such a stat type -- the int32 count, then per channel mean, m2, m3,
    film_mean, film_m2 as far as the type has them; 0 for values a stat type cannot have (no device needed)."""
    return int(load().statmc_state_dwords(int(channels), int(max_moment), int(bool(transform))))


def _state_arrays(stat_types, n, states, who, device=None):
    """One contiguous int32 CUDA tensor [n, D_t] per stat type: the caller's, checked, or (states None) new ones on `device`."""
    tc = _torch()
    dw = [state_dwords(t.channels, t.max_moment, t.transform) for t in stat_types]
    if states is None:
        return [tc.empty((n, d), dtype=tc.int32, device=device) for d in dw]
    if len(states) != len(stat_types):
        raise ValueError("%s: one state array per stat type" % who)
    for i, (s, d) in enumerate(zip(states, dw)):
        if s.dtype != tc.int32 or not s.is_contiguous() or (s.numel() and not s.is_cuda) or s.numel() != n * d:
            raise ValueError("%s: states[%d] must be a contiguous int32 CUDA tensor of %d x %d dwords" % (who, i, n, d))
    return list(states)


def gather_states(width, height, stat_types, pixels, out=None, stream=None):
    """statmc_gather_states (include/statmc.h): `pixels` is an int32 device tensor, one entry per record; record i of every stat
    type receives the stored state of pixel pixels[i] as state_dwords(...) dwords -- a value outside the film the state of no
    samples.  stat_types: make_stat_type_record_field (the images only).  Returns one int32 tensor [n, D_t] per stat type (out:
    the caller's, written in place).  Asynchronous; the images are only read."""
    tc = _torch()
    if pixels.dtype != tc.int32 or not pixels.is_contiguous():
        raise ValueError("gather_states: pixels must be a contiguous int32 tensor")
    n = pixels.numel()
    states = _state_arrays(stat_types, n, out, "gather_states", device=pixels.device)
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    ptrs = (C.c_void_p * max(len(states), 1))(*[s.data_ptr() for s in states])
    check(load().statmc_gather_states(int(width), int(height), arr, len(stat_types), pixels.data_ptr(), n, ptrs,
                                      stream if stream is not None else current_stream_handle()))
    return states


def combine_records(width, height, stat_types, pixels, states, split_above=None, stream=None):
    """statmc_combine_records (include/statmc.h): merges the records (pixels[i], states[t][i]) into the images of stat_types
    (make_stat_type_record_field) -- per pixel in ascending record index, the stored state as part A and every record with a
    positive count as part B of a two-part combine: the bits of combine_statistics / combine_many on the same parts.  A pixel
    without such a record keeps every bit.  split_above = k: a pixel with more than k records is folded by the 64 lanes of a wave
    (64 chunks, merged in a fixed tree); None: INT32_MAX, never split.  Asynchronous; the tensors must stay alive until it ran."""
    tc = _torch()
    if pixels.dtype != tc.int32 or not pixels.is_contiguous():
        raise ValueError("combine_records: pixels must be a contiguous int32 tensor")
    n = pixels.numel()
    states = _state_arrays(stat_types, n, states, "combine_records")
    arr = (StatType * max(len(stat_types), 1))(*stat_types)
    ptrs = (C.c_void_p * max(len(states), 1))(*[s.data_ptr() for s in states])
    check(load().statmc_combine_records(int(width), int(height), arr, len(stat_types), pixels.data_ptr(), n, ptrs,
                                        INT32_MAX if split_above is None else int(split_above),
                                        stream if stream is not None else current_stream_handle()))


def calculate_mean_vars(n, film_m2, film_var, row_n_quirk=True, stream=None):
    h, w = n[0].shape
    c = film_m2[0].shape[2] if film_m2[0].dim() == 3 else 1
    check(load().statmc_calculate_mean_vars(len(n), w, h, c, _img_array(n), _img_array(film_m2),
                                            _img_array(film_var), int(row_n_quirk),
                                            stream if stream is not None else current_stream_handle()))


def merge_tiles(width, height, channels, transform, tile_pixels, tile_bounds, tile_offsets, max_tile_pixels,
                state, stream=None):
    fm = state["film_mean"].data_ptr() if transform else None
    f2 = state["film_m2"].data_ptr() if transform else None
    check(load().statmc_merge_tiles(width, height, channels, int(bool(transform)), tile_pixels.data_ptr(),
                                    tile_bounds.data_ptr(), tile_offsets.data_ptr(), tile_bounds.shape[0],
                                    max_tile_pixels, state["n"].data_ptr(), state["mean"].data_ptr(),
                                    state["m2"].data_ptr(), state["m3"].data_ptr(), fm, f2,
                                    stream if stream is not None else current_stream_handle()))


def film_update(film_pixels, n_pixels, film_rgb, splat_scale=1.0, scale=1.0, stream=None):
    """film_pixels: uint8 device tensor holding n_pixels Film::Pixel structs (32 B each)."""
    check(load().statmc_film_update(film_pixels.data_ptr(), n_pixels, float(splat_scale), float(scale), film_rgb.data_ptr(),
                                    stream if stream is not None else current_stream_handle()))


def tile_moments(values, tile_size, out, stream=None):
    h, w = values.shape[0], values.shape[1]
    c = values.shape[2] if values.dim() == 3 else 1
    check(load().statmc_tile_moments(w, h, c, values.data_ptr(), tile_size, out.data_ptr(),
                                     stream if stream is not None else current_stream_handle()))


def clock_probe(out, cycles=200000, stream=None):
    """out: int64 device tensor of 2 elements <- {shader clocks counted, 10 ns ticks they took}."""
    assert out.is_cuda and out.numel() >= 2 and out.element_size() == 8
    check(load().statmc_clock_probe(out.data_ptr(), int(cycles), stream if stream is not None else current_stream_handle()))
