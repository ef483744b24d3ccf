"""numpy restatement of statmc_compact_offsets (include/statmc.h) and of statmc_compact_accumulate's run clamp: what
tests/test_compact_offsets_gpu.py and tests/test_compact_accumulate_gpu.py hold the device to."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
CHUNK = 1024          # pixels per scan block: one 64-bit workspace word each


def workspace_bytes(width, height):
    return -(-width * height // CHUNK) * 8


def clamped_counts(counts, cap=INT32_MAX):
    """c(p) = min(max(sample_counts[p], 0), cap) as int64, flat in raster order"""
    return np.clip(np.asarray(counts, dtype=np.int64).reshape(-1), 0, int(cap))


def offsets_ref(counts, cap=INT32_MAX):
    """int64 [H * W + 1]: the exclusive prefix sum of c(p) in raster order; the last entry is the total"""
    c = clamped_counts(counts, cap)
    out = np.zeros(c.size + 1, dtype=np.int64)
    np.cumsum(c, dtype=np.int64, out=out[1:])
    return out


def owners_ref(counts, owners_capacity, cap=INT32_MAX):
    """int32 [owners_capacity]: slot i's pixel for i below the total, -1 at and behind it"""
    c = clamped_counts(counts, cap)
    own = np.repeat(np.arange(c.size, dtype=np.int32), c)[:owners_capacity]
    return np.concatenate([own, np.full(owners_capacity - own.size, -1, np.int32)])


def clamp_runs(offsets, n_samples):
    """(start, end) per pixel: start = clamp(offsets[p], 0, n_samples), end = clamp(offsets[p + 1], start, n_samples)"""
    o = np.asarray(offsets, dtype=np.int64)
    start = np.clip(o[:-1], 0, n_samples)
    end = np.minimum(np.maximum(o[1:], start), n_samples)
    return start, end


def records_of_runs(start, end):
    """The (pixels, positions) record list the records entries take for the clamped runs: pixel p's positions start[p] ..
    end[p] - 1 in ascending order, pixels in raster order."""
    cnt = (end - start).astype(np.int64)
    pixels = np.repeat(np.arange(cnt.size, dtype=np.int32), cnt)
    first = np.repeat(start, cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return pixels, first + within
