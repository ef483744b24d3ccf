"""statmc_score_sum (include/statmc.h) restated: keys from numpy uint32 views, the sums of M << s and (M << s)^2 in Python integers
(exact_sums: pixels of one shift s are counted together first, in integers that cannot overflow), one correctly rounded conversion at
the end, float(Fraction(N, 2^149)).  Nothing of the library is used."""
from fractions import Fraction

import numpy as np

MAX_CAPS = 4
INF_KEY = 0x7F800000


def keys_of(score):
    """NaN of either sign and everything with the sign bit are 0; everything else is its own bit pattern"""
    b = np.ascontiguousarray(score, np.float32).reshape(-1).view(np.uint32)
    dead = ((b & np.uint32(0x7FFFFFFF)) > np.uint32(INF_KEY)) | ((b >> np.uint32(31)) != 0)
    return np.where(dead, np.uint32(0), b)


def key_of(x):
    return int(keys_of(np.array([x], np.float32))[0])


def units_of(k):
    """val(k) * 2^149 as an integer, 0 < k < 0x7F800000; 0 for k == 0"""
    e, m = k >> 23, k & 0x7FFFFF
    M = (m | 0x800000) if e else m
    s = e - 1 if e else 0
    return M << s


def round_to_double(n, unit):
    """the double nearest, ties to even, to n * 2^-unit"""
    return float(Fraction(n, 2 ** unit))


def exact_sums(c):
    """(sum of units_of, sum of its squares) over the uint32 keys c, all below INF_KEY, as Python integers.  The keys are grouped by
    their shift s; within a group the significands M < 2^24 and the halves of M^2 < 2^48 are added in uint64, which is exact for
    fewer than 2^40 of them; M << s and M^2 << 2 s are then formed and added in Python integers."""
    if c.size == 0:
        return 0, 0
    e, m = c >> np.uint32(23), c & np.uint32(0x7FFFFF)
    M = np.where(e != 0, m | np.uint32(0x800000), m).astype(np.uint64)
    s = np.where(e != 0, e - np.uint32(1), np.uint32(0)).astype(np.int64)
    order = np.argsort(s, kind="stable")
    s, M = s[order], M[order]
    starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    q = M * M
    sum_m = np.add.reduceat(M, starts)
    sum_lo, sum_hi = np.add.reduceat(q & np.uint64(0xFFFFFF), starts), np.add.reduceat(q >> np.uint64(24), starts)
    total = total_sq = 0
    for sh, a, lo, hi in zip(s[starts], sum_m, sum_lo, sum_hi):
        total += int(a) << int(sh)
        total_sq += ((int(hi) << 24) + int(lo)) << (2 * int(sh))
    return total, total_sq


def sum_ref(score, caps):
    assert 1 <= len(caps) <= MAX_CAPS
    keys = keys_of(score)
    r = {"n_px": int(keys.size), "n_zero": int((keys == 0).sum()), "n_finite": int(((keys > 0) & (keys < INF_KEY)).sum()),
         "n_infinite": int((keys == INF_KEY).sum()), "n_caps": len(caps),
         "cap_bits": [0] * MAX_CAPS, "n_clipped": [0] * MAX_CAPS, "sum": [0.0] * MAX_CAPS, "sum_sq": [0.0] * MAX_CAPS}
    for j, cap in enumerate(caps):
        ck = key_of(cap)
        c = np.minimum(keys, np.uint32(ck))      # as unsigned integers: bit order is value order
        total, total_sq = exact_sums(c[c != INF_KEY])      # a pixel whose c is +inf is left out
        r["cap_bits"][j], r["n_clipped"][j] = ck, int((keys > ck).sum())
        r["sum"][j], r["sum_sq"][j] = round_to_double(total, 149), round_to_double(total_sq, 298)
    return r


def double_bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def result_bits(r):
    """everything of a result as integers: the doubles as their bit patterns"""
    return (r["n_px"], r["n_zero"], r["n_finite"], r["n_infinite"], r["n_caps"], list(r["cap_bits"]), list(r["n_clipped"]),
            [double_bits(x) for x in r["sum"]], [double_bits(x) for x in r["sum_sq"]])


def means(r):
    """per asked cap: (mean, rms) over the judged pixels, in float64 as FilmStats.score_mean forms them"""
    out = []
    for j in range(r["n_caps"]):
        n = r["n_px"] - (r["n_infinite"] if r["cap_bits"][j] == INF_KEY else 0)
        out.append((r["sum"][j] / n, float(np.sqrt(np.float64(r["sum_sq"][j]) / n))) if n else (float("nan"), float("nan")))
    return out
