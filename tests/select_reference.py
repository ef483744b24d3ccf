"""numpy restatement of statmc_score_select and statmc_score_count_above (include/statmc.h), for tests/test_score_select_cpu.py (its
own properties) and tests/test_score_select_gpu.py (the device's bits).  Keys are uint32 views; the k-th smallest comes from a full
np.sort -- not from the device's digit passes."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
MAX_RANKS = 8
LIVE_LO, LIVE_HI = 0x21800000, 0x5D800000      # the bit patterns of 2^-60 and 2^60
FIELDS = ("n_px", "n_live", "n_saturated", "n_ranks", "rank", "value_bits", "n_below", "n_equal")


def bits_of(score):
    return np.ascontiguousarray(np.asarray(score, F32)).reshape(-1).view(np.uint32)


def keys_of(score):
    """uint32 keys of a float32 image, flat: 0 for NaN of either sign and for everything with the sign bit, else the bit pattern"""
    b = bits_of(score)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    signbit = (b >> np.uint32(31)) != 0
    return np.where(nan | signbit, np.uint32(0), b)


def key_of(x):
    return int(keys_of(np.array([x], F32))[0])


def class_counts(keys):
    """(n_live, n_saturated) on keys"""
    return int(((keys >= LIVE_LO) & (keys <= LIVE_HI)).sum()), int((keys > LIVE_HI).sum())


def select_ref(score, ranks):
    """the fields of statmc_select_result as a dict, the per-rank ones as lists of len(ranks) Python integers"""
    keys = keys_of(score)
    ranks = [int(r) for r in ranks]
    assert 1 <= len(ranks) <= MAX_RANKS and all(0 <= r < keys.size for r in ranks)
    order = np.sort(keys)
    live, sat = class_counts(keys)
    value = [int(order[r]) for r in ranks]
    return dict(n_px=int(keys.size), n_live=live, n_saturated=sat, n_ranks=len(ranks), rank=ranks, value_bits=value,
                n_below=[int(np.searchsorted(order, v, "left")) for v in value],
                n_equal=[int(np.searchsorted(order, v, "right") - np.searchsorted(order, v, "left")) for v in value])


def count_above_ref(score, thresholds):
    keys = keys_of(score)
    return [int((keys > np.uint32(key_of(t))).sum()) for t in thresholds]


def nearest_rank(q, n_px):
    """rank(q) = max(0, ceil(q * P) - 1) in Python integers, q taken as the number it is (a Fraction) or as the double it converts to
    (Python and numpy floats)"""
    return max(0, math.ceil((q if isinstance(q, Fraction) else Fraction(float(q))) * n_px) - 1)


def values_of(value_bits):
    return np.array(value_bits, np.uint32).view(F32)
