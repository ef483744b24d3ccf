"""statmc_score_tiles (include/statmc.h) restated: per tile the keys from numpy uint32 views, the sums of M << s and (M << s)^2 in
Python integers (score_sum_reference.exact_sums), one correctly rounded conversion to a double, and the mean as a
fractions.Fraction rounded to float32 by a search of its own between the two neighbouring float32 values -- never through a double,
which would round twice.  Nothing of the library is used."""
from fractions import Fraction

import numpy as np

from score_sum_reference import INF_KEY, exact_sums, key_of, keys_of, round_to_double, units_of

TILES = (8, 16, 32, 64)
PLANES = ("sum", "sum_sq", "mean", "max", "n_px", "n_zero", "n_infinite", "n_clipped")
DTYPES = {"sum": np.float64, "sum_sq": np.float64, "mean": np.float32, "max": np.float32,
          "n_px": np.int32, "n_zero": np.int32, "n_infinite": np.int32, "n_clipped": np.int32}
UNIT = Fraction(1, 2 ** 149)


def value_of_key(k):
    """the exact value of the float32 with the non-negative finite bit pattern k"""
    return units_of(k) * UNIT


def nearest_float32_key(x):
    """The bit pattern of the float32 nearest, ties to even, to the Fraction x, 0 <= x <= the largest finite float32.  Bit order is
    value order on non-negative floats: a bisection finds the largest pattern whose value is <= x (value(k) <= x is
    units_of(k) * denominator <= numerator * 2^149, in integers), then x is compared with its two neighbours as Fractions; of two
    equally near patterns the even one is the one with the even significand."""
    assert 0 <= x <= value_of_key(INF_KEY - 1)
    num, den = x.numerator << 149, x.denominator
    lo, hi = 0, INF_KEY - 1      # value(lo) <= x always
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if units_of(mid) * den <= num:
            lo = mid
        else:
            hi = mid - 1
    if lo == INF_KEY - 1 or value_of_key(lo) == x:
        return lo
    below, above = x - value_of_key(lo), value_of_key(lo + 1) - x
    if below != above:
        return lo if below < above else lo + 1
    return lo if lo % 2 == 0 else lo + 1


def tile_ref(keys, ck):
    """one tile's statistics from its uint32 keys (any shape) under the cap's key ck, as Python numbers: sum and sum_sq as floats
    (the doubles), mean and max as float32 bit patterns"""
    keys = np.asarray(keys, np.uint32).reshape(-1)
    c = np.minimum(keys, np.uint32(ck))
    counted = c[c != INF_KEY]
    total, total_sq = exact_sums(counted)
    n_inf = int((keys == INF_KEY).sum())
    n_counted = int(keys.size) - (n_inf if ck == INF_KEY else 0)
    assert n_counted == counted.size
    return {"n_px": int(keys.size), "n_zero": int((keys == 0).sum()), "n_infinite": n_inf, "n_clipped": int((keys > ck).sum()),
            "sum": round_to_double(total, 149), "sum_sq": round_to_double(total_sq, 298),
            "mean": nearest_float32_key(Fraction(total, n_counted) * UNIT) if n_counted else 0, "max": int(keys.max())}


def tiles_ref(score, tile, cap):
    """every plane of statmc_score_tiles for the float32 image score[H][W]: {name: array [tiles_y][tiles_x]} with PLANES' names and
    DTYPES' types (mean and max as float32 with exactly the restated bit patterns)"""
    assert tile in TILES
    score = np.asarray(score, np.float32)
    H, W = score.shape
    keys = keys_of(score).reshape(H, W)
    ck = key_of(cap)
    ty, tx = -(-H // tile), -(-W // tile)
    out = {p: np.zeros((ty, tx), np.uint32 if p in ("mean", "max") else DTYPES[p]) for p in PLANES}
    for j in range(ty):
        for i in range(tx):
            t = tile_ref(keys[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile], ck)
            for p in PLANES:
                out[p][j, i] = t[p]
    out["mean"], out["max"] = out["mean"].view(np.float32), out["max"].view(np.float32)
    return out


def plane_bits(a):
    """a plane as integers: the doubles and floats as their bit patterns"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


def same_bits(got, want, planes=PLANES):
    """the names of the planes that differ in any bit"""
    return [p for p in planes if got[p].shape != want[p].shape or got[p].dtype != want[p].dtype
            or not np.array_equal(plane_bits(got[p]), plane_bits(want[p]))]
