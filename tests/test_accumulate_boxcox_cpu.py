"""The yardsticks of the per-element checks of the Box-Cox moments (tests/test_accumulate_boxcox_gpu.py), and their own tests.

The device takes v_sqrt_f32 where the oracle takes pow(x, .5), so `mean` / `m2` / `m3` of a transformed type cannot be compared
with the oracle's bit for bit -- but the comparison splits into two halves that can:
  (a) the device's Box-Cox value v of every sample is one of the few floats a root within 1 ulp allows (box_cox_candidates);
  (b) given the device's own v, the chain is the oracle's UNtransformed chain on v, bit for bit (chain_reference).
v can be read through the public entry: one sample folded into a fresh state (n = 0, every plane 0) leaves mean = v
(d = v - 0, div_by_count(v, 1, 1) = v, 0 + v = v).

The second yardstick is an exact emulation of refined_rcp / div_by_count (include/statmc_device_api.hpp) in integer arithmetic,
for every v_rcp_f32 result the ISA's 1 ulp allows: what the division may return for operands no sample recipe reaches
(subnormal quotients, FLT_MAX, infinities)."""
from fractions import Fraction

import numpy as np

F32_MIN_SUB = np.float32(2.0 ** -149)
FLT_MIN = np.float32(2.0 ** -126)
FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------ bits
def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits_or_nan(got, ref, what="", channels=None):
    """got and ref (float32 arrays of one shape, [..., C] or [...]) agree: the non-finite elements sit at the same positions, NaN
    matches NaN (whatever its payload), and everything else -- the infinities and the sign of zero included -- is equal as int32.
    A failure names the first differing pixel and channel and both values."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    c = channels if channels is not None else (got.shape[-1] if got.ndim >= 3 else 1)
    bad_nf = np.isfinite(got) != np.isfinite(ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    bad = (bad_nf | ((f32_bits(got) != f32_bits(ref)) & ~both_nan)).reshape(-1)
    if not bad.any():
        return
    e = int(np.flatnonzero(bad)[0])
    g, r = got.reshape(-1)[e], ref.reshape(-1)[e]
    raise AssertionError("%s: %d of %d elements differ%s, the first at pixel %d channel %d: %r (0x%08x) / reference %r (0x%08x)" % (
        what, int(bad.sum()), bad.size, " (%d of them finite against non-finite)" % int(bad_nf.sum()) if bad_nf.any() else "",
        e // c, e % c, float(g), int(f32_bits(g).reshape(-1)[0]) & 0xffffffff, float(r), int(f32_bits(r).reshape(-1)[0]) & 0xffffffff))


# ------------------------------------------------------------------ (a) the transform
def box_cox_of_root(c):
    """fl32(2 c - 2) -- (c - 1) / .5 -- with ONE rounding, for float32 roots c >= 0 (array).  float64 suffices everywhere:
      c >= 2^-26 and c < 2^52: 2 c - 2 has its bits between 2^-49 and 2^53 at the most: exact in double, one rounding to float;
      c <  2^-26: every value in [-2, -2 + 2^-25) rounds to -2 in both formats (the float next to -2 is -2 + 2^-23 ... the
                  midpoint -2 + 2^-24 is never reached), so the double's rounding cannot change the float's;
      c >= 2^26:  2 c is a float whose neighbours lie 16 or more away, 2 c - 2 rounds back to it in both formats.
    test_box_cox_of_root_is_one_rounding holds this against exact rational arithmetic."""
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (2.0 * c - 2.0).astype(np.float32)


def box_cox_of_root_exact(c):
    """The same for one root, in exact arithmetic (fractions): the yardstick of box_cox_of_root."""
    return round_to_f32(2 * Fraction(float(c)) - 2)


def round_to_f32(q):
    """A rational to the nearest float32, ties to even, subnormals and overflow to infinity included (np.float32)."""
    q = Fraction(q)
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                                  # 2^e <= q < 2^(e + 1)
    quantum = max(e - 23, -149)
    scaled = q / Fraction(2) ** quantum
    k = scaled.numerator // scaled.denominator
    rest = scaled - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    if k * Fraction(2) ** quantum >= Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * float(k) * 2.0 ** quantum)          # k < 2^25 and 2^quantum are doubles, their product a float32


def sqrt_floor_ceil(s):
    """(lo, hi, exact): the largest float32 <= sqrt(s) and the smallest >= sqrt(s), for float32 s > 0 finite (arrays).  The
    comparisons c^2 <=> s are exact in double: c has 24 bits, c^2 48, and 2^-150 <= c^2 < 2^128 for every float32 s."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    c = np.sqrt(s64).astype(np.float32)                         # within one float of the root; settled below
    for _ in range(2):
        c = np.where(c.astype(np.float64) ** 2 > s64, np.nextafter(c, np.float32(0)), c).astype(np.float32)
    for _ in range(2):
        up = np.nextafter(c, np.float32(np.inf))
        c = np.where(up.astype(np.float64) ** 2 <= s64, up, c).astype(np.float32)
    exact = c.astype(np.float64) ** 2 == s64
    hi = np.where(exact, c, np.nextafter(c, np.float32(np.inf))).astype(np.float32)
    assert (c.astype(np.float64) ** 2 <= s64).all() and (exact | (hi.astype(np.float64) ** 2 > s64)).all()
    return c, hi, exact


def box_cox_candidates(s):
    """The float32 values v = (root - 1) / .5 that a float32 root within 1 ulp of sqrt(s) allows -- the bound the comment in
    include/statmc_device_api.hpp states and the ISA manual gives for v_sqrt_f32 -- for float32 samples `s` (scalar or array).
    Returns (cand float32 [..., 2], exact bool [...]): the allowed values, a single one given twice.

    The roots: every float32 c with |c - sqrt(s)| <= 1 ulp.  An inexact root lies strictly between two neighbouring floats one
    ulp apart: those two and no others.  An exactly representable root is held to itself: a float32 whose root is a float32 is
    the square of a float with at most 12 significant bits (an odd k-bit significand squares to an odd one of 2 k - 1 or 2 k
    bits, which fits 24 only for k <= 12), and such a square gives exactly one value -- `exact` marks them.  Each root gives
    fl32(2 c - 2), formed with one rounding (box_cox_of_root).
    +0 and -0 give -2 (root 0), and so does every sample whose root is below 2^-25; negative samples and NaN give NaN;
    +inf gives +inf."""
    s = np.asarray(s, np.float32)
    shape = s.shape
    s = s.reshape(-1)
    cand = np.full((s.size, 2), np.nan, np.float32)
    exact = np.zeros(s.size, bool)
    zero = s == 0                                              # +0 and -0
    cand[zero] = -2.0
    exact[zero] = True
    cand[np.isposinf(s)] = np.inf
    exact[np.isposinf(s)] = True
    pos = np.isfinite(s) & (s > 0)
    lo, hi, ex = sqrt_floor_ceil(s[pos])
    cand[pos, 0], cand[pos, 1] = box_cox_of_root(lo), box_cox_of_root(hi)
    exact[pos] = ex
    return cand.reshape(shape + (2,)), exact.reshape(shape)


def in_candidates(v, cand):
    """Per element: v is one of cand[..., :] -- as bits, a NaN candidate matching any NaN."""
    v = np.asarray(v, np.float32)
    hit = np.zeros(v.shape, bool)
    for k in range(cand.shape[-1]):
        ck = cand[..., k]
        hit |= (f32_bits(v) == f32_bits(ck)) | (np.isnan(v) & np.isnan(ck))
    return hit


def nearest_box_cox(s):
    """v from the correctly rounded root (np.sqrt on float32 is): what a count of 'roots that are not the nearest' compares with."""
    with np.errstate(invalid="ignore"):
        return box_cox_of_root(np.sqrt(np.asarray(s, np.float32)))


def directed_samples(seed=2024):
    """The directed list of the per-sample transform test, about 70 000 float32 values, and the mask of the exact squares in it."""
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    parts = [np.array([0.0, -0.0, 2.0 ** -149, 1e-40, 2.0 ** -126], np.float32),
             (2.0 ** np.arange(-126, 128, dtype=np.float64)).astype(np.float32),
             np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], np.float32)]
    roots = (rng.integers(2 ** 11, 2 ** 12, 4096).astype(np.float64) * 2.0 ** (rng.integers(-14, 6, 4096) - 11)).astype(np.float32)
    squares = (roots.astype(np.float64) ** 2).astype(np.float32)
    assert (squares.astype(np.float64) == roots.astype(np.float64) ** 2).all()          # 24 bits: exact
    parts += [squares, np.nextafter(squares, np.float32(0)), np.nextafter(squares, np.float32(np.inf))]
    parts.append(np.array([FLT_MAX, np.inf, -1.0, -1e-6, np.nan], np.float32))
    expo = rng.integers(0, 255, 65536).astype(np.uint32)         # uniform in the exponent field, subnormals included, no inf / NaN
    parts.append(((expo << 23) | rng.integers(0, 2 ** 23, 65536).astype(np.uint32)).view(np.float32))
    return np.concatenate(parts).astype(np.float32)


def heavy_tailed_samples(rng, S, H, W, channels, half=False, zeros=0.15):
    """The sample recipe of the chain checks: lognormal(0, 2.5), 10 to 20 % exact zeros, one sample x 1e6 and one batch x 1e-6,
    one negative and one +inf sample in two further pixels; half: rounded to half first and capped at 65504 (the infinite one
    stays).  Returns [S, H, W, C] float32."""
    x = rng.lognormal(0, 2.5, size=(S, H, W, channels)).astype(np.float32)
    x[rng.random(x.shape) < zeros] = 0.0
    x[S // 2, H // 2, W // 2, 0] = max(float(x[S // 2, H // 2, W // 2, 0]), 0.5) * 1e6
    if S > 1:
        x[S - 1] *= np.float32(1e-6)
    else:                                                       # a single sample: the first half of the pixels (the x 1e6 one is in the second)
        x.reshape(-1, channels)[:H * W // 2] *= np.float32(1e-6)
    if half:
        x = np.minimum(x, np.float32(65504.0)).astype(np.float16).astype(np.float32)
    x[0, H - 1, min(5, W - 1), channels - 1] = -1.0
    x[S // 3, 0, W - 2 if W > 1 else 0, 0] = np.inf
    return x


def random_start_state(rng, H, W, channels, n):
    """A host-made starting state: counts `n` ([H, W] int32) and random moments where the count is positive."""
    st = dict(n=np.ascontiguousarray(n, np.int32))
    for k in ("mean", "m2", "m3", "film_mean", "film_m2"):
        st[k] = (rng.random((H, W, channels)) * (st["n"][..., None] > 0)).astype(np.float32)
    return st


# ------------------------------------------------------------------ (b) the chain
def chain_reference(oracle, start_state, v, max_moment):
    """mean / m2 / m3 after the oracle's UNtransformed chain has folded v ([S, H, W, C] float32: the device's own Box-Cox values)
    into a copy of the host-made starting state.  (film_mean / film_m2, the raw-sample chain, stay with the transform=True run.)"""
    st = {k: np.array(a, copy=True) for k, a in start_state.items()}
    oracle.accumulate(st, np.ascontiguousarray(v, np.float32), False, max_moment)
    return {k: st[k] for k in ("n", "mean", "m2", "m3")}


def oracle_box_cox(oracle, smp):
    """The oracle's own v of every sample, read by the one-sample trick: [any shape] float32 -> the same shape."""
    smp = np.asarray(smp, np.float32)
    flat = np.ascontiguousarray(smp.reshape(1, 1, -1, 1))
    st = oracle.new_state(1, flat.shape[2], 1)
    oracle.accumulate(st, flat, True, 1)
    return st["mean"].reshape(smp.shape)


def infinite_sample_elements(smp):
    """[H, W, C] bool: the elements that were handed an infinite sample ([S, H, W, C]).  The device's division by the count leaves
    NaN for an infinite dividend where the reference leaves inf (include/statmc.h, statmc_accumulate): from that sample on every
    plane of the element is NaN on the device and non-finite in the oracle.  The one-sample read-out of v goes through that
    division too: it returns NaN for a +inf sample, so chain_reference on the values read holds NaN there like the device."""
    return np.isinf(np.asarray(smp, np.float32)).any(axis=0)


# ------------------------------------------------------------------ refined_rcp / div_by_count, exactly
# A float32 as an integer count of 2^-149 (every finite float32 is one), +-inf and NaN as Python floats.
UNIT = 149
INF_UNITS = 1 << (128 + UNIT)


def to_units(x):
    x = float(np.float32(x))
    if x != x or x in (float("inf"), float("-inf")):
        return x
    u = x * 2.0 ** UNIT                                          # a power-of-two scaling: exact in double, and an integer
    assert u == int(u)
    return int(u)


def from_units(u):
    if isinstance(u, float):
        return np.float32(u)
    sign, u = (-1.0 if u < 0 else 1.0), abs(u)
    hi = u >> 100                                              # split so that both factors are doubles
    return np.float32(sign * (float(hi) * 2.0 ** (100 - UNIT) + float(u & ((1 << 100) - 1)) * 2.0 ** -UNIT))


def round_units(n, e):
    """The integer n, counting 2^-e, to the nearest float32 (ties to even) as a count of 2^-149; +-inf on overflow."""
    if n == 0:
        return 0
    sign, n = (-1 if n < 0 else 1), abs(n)
    drop = max(n.bit_length() - 24, e - UNIT, 0)               # the bits below the float's last place (24 bits, or 2^-149)
    k = n >> drop
    if drop > 0:
        rest, half = n & ((1 << drop) - 1), 1 << (drop - 1)
        if rest > half or (rest == half and k & 1):
            k += 1
    u = k << (drop - (e - UNIT))
    return sign * u if u < INF_UNITS else sign * float("inf")


def fma_units(a, b, c):
    """fl32(a b + c) with one rounding; the IEEE rules for infinite and NaN operands."""
    if any(isinstance(x, float) and x != x for x in (a, b, c)):
        return float("nan")
    if isinstance(a, float) or isinstance(b, float):             # an infinite factor
        if a == 0 or b == 0:
            return float("nan")
        prod = float("inf") if (a > 0) == (b > 0) else float("-inf")
        return float("nan") if isinstance(c, float) and c != prod else prod
    if isinstance(c, float):
        return c
    return round_units(a * b + (c << UNIT), 2 * UNIT)


def mul_units(a, b):
    return fma_units(a, b, 0)


def rcp_candidates(n):
    """The v_rcp_f32 results the ISA's 1 ulp allows for an integer n in [1, 2^24): the correctly rounded 1 / n and both its
    neighbours, as counts of 2^-149."""
    near = round_to_f32(Fraction(1, int(n)))
    return [to_units(np.nextafter(near, np.float32(0))), to_units(near), to_units(np.nextafter(near, np.float32(2)))]


def emulate_refined_rcp(n, y0):
    nf = to_units(float(n))
    e = fma_units(-nf, y0, to_units(1.0))
    return fma_units(e, y0, y0)


def emulate_div_by_count(d, n, y0):
    """div_by_count(d, n, refined_rcp(n)) for the v_rcp_f32 result y0: the three roundings of the device sequence, each exact."""
    nf, r = to_units(float(n)), emulate_refined_rcp(n, y0)
    d = to_units(d)
    q0 = mul_units(d, r)
    rem = fma_units(-q0, nf, d)
    return fma_units(rem, r, q0)


def allowed_quotients(d, n):
    """The float32 values div_by_count may return for (d, n): one per v_rcp_f32 candidate, at most three different ones."""
    return [from_units(emulate_div_by_count(d, n, y0)) for y0 in rcp_candidates(n)]


def ieee_quotient(d, n):
    d = np.float32(d)
    if not np.isfinite(d):
        return d
    return round_to_f32(Fraction(float(d)) / int(n))


# The same sequence for whole arrays, in double: a b is exact there (48 bits), and a b + c rounded to ODD in double and then to
# float32 is the correctly rounded fma (53 >= 2 x 24 + 2 bits; Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums").
# The rounding to odd comes from the exact error of the double sum (Knuth's TwoSum).  test_division_emulation_against_exact_division
# holds it against the integer emulation above.
def fma_f32(a, b, c):
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def allowed_quotients_f32(d, n):
    """allowed_quotients for arrays: float32 [3, N], row k for the v_rcp_f32 candidate k (below, nearest, above)."""
    d, nf = np.asarray(d, np.float32), np.asarray(n).astype(np.float32)
    assert (nf.astype(np.int64) == np.asarray(n)).all()
    near = np.float32(1.0) / nf                                  # IEEE division: the correctly rounded reciprocal
    out = []
    for y0 in (np.nextafter(near, np.float32(0)), near, np.nextafter(near, np.float32(2))):
        r = fma_f32(fma_f32(-nf, y0, np.float32(1.0)), y0, y0)
        q0 = fma_f32(d, r, np.float32(0.0))
        out.append(fma_f32(fma_f32(-q0, nf, d), r, q0))
    return np.stack(out)


def ieee_quotients_f32(d, n):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(d, np.float32) / np.asarray(n).astype(np.float32)


def subnormal_quotient_operands(count, n_max, seed):
    """`count` pairs (d, n): d = k 2^(-149 + j) with k below 2^24 and j in 0 .. 13, n in 2 .. n_max, kept where the quotient
    d / n is subnormal."""
    rng = np.random.default_rng(seed)
    ds, ns = np.zeros(0, np.float32), np.zeros(0, np.int64)
    while ds.size < count:
        k = rng.integers(1, 2 ** 24, 2 * count).astype(np.float64)
        j = rng.integers(0, 14, 2 * count)
        n = rng.integers(2, n_max + 1, 2 * count)
        d = k * 2.0 ** (j - 149.0)
        keep = d / n < 2.0 ** -126
        ds, ns = np.concatenate([ds, d[keep].astype(np.float32)]), np.concatenate([ns, n[keep]])
    return ds[:count], ns[:count].astype(np.int32)


DIVISION_SPECIALS = [(FLT_MAX, 1), (FLT_MAX, 2), (FLT_MAX, 3), (np.float32(np.inf), 1), (np.float32(-np.inf), 1), (np.float32(np.inf), 7),
                     (np.float32(-np.inf), 448), (np.float32(1.5504638832552652e-38), 448)]


def division_operands():
    """The directed operands of test_gpu_parity.test_exact_division_directed_operands: 40 000 subnormal quotients with n up to
    4096, 40 000 with n up to 2^24 - 1, FLT_MAX over 1, 2 and 3, the infinities, and the first case the emulation found."""
    d1, n1 = subnormal_quotient_operands(40000, 4096, seed=41)
    d2, n2 = subnormal_quotient_operands(40000, 2 ** 24 - 1, seed=42)
    ds = np.concatenate([d1, d2, np.array([d for d, _ in DIVISION_SPECIALS], np.float32)])
    ns = np.concatenate([n1, n2, np.array([n for _, n in DIVISION_SPECIALS], np.int32)])
    return ds, ns


# ------------------------------------------------------------------ the tests of the yardsticks
def test_same_bits_or_nan_tells_what_it_must():
    import pytest
    a = np.array([[[1.0, -0.0, np.nan]], [[np.inf, 2.0, 3.0]]], np.float32)
    same_bits_or_nan(a, a.copy(), "same")
    b = a.copy()
    b.view(np.int32)[0, 0, 2] ^= 1                                # another NaN payload: still NaN
    same_bits_or_nan(a, b, "payload")
    for idx, val in (((0, 0, 1), 0.0), ((1, 0, 0), np.nan), ((1, 0, 1), np.nextafter(np.float32(2), np.float32(3))), ((0, 0, 2), 1.0),
                     ((1, 0, 0), -np.inf)):
        b = a.copy()
        b[idx] = val
        with pytest.raises(AssertionError) as e:
            same_bits_or_nan(b, a, "case")
        assert "pixel %d channel %d" % (idx[0], idx[2]) in str(e.value)


def test_round_to_f32_against_numpy():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.standard_normal(200) * 10.0 ** rng.integers(-46, 39, 200), [2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -149, 2.0 ** 128, 3.4028235677973366e38]])
    with np.errstate(over="ignore"):
        for x in xs:
            assert f32_bits(round_to_f32(Fraction(float(x)))) == f32_bits(np.float32(x)), x
    for u in (0, 1, -1, 2 ** 23, 2 ** 24 - 1, -(2 ** 100 + 2 ** 77), 2 ** 276):   # the unit representation round-trips
        assert round_units(u, UNIT) == u and to_units(from_units(u)) == u


def test_box_cox_of_root_is_one_rounding():
    rng = np.random.default_rng(6)
    c = np.concatenate([(2.0 ** rng.uniform(-75, 64, 3000)).astype(np.float32),
                        (1 + rng.integers(-300, 300, 600) * 2.0 ** -24).astype(np.float32),
                        np.array([0.0, 2.0 ** -75, 2.0 ** -26, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -24, 2.0 ** 25,
                                  2.0 ** 26, 2.0 ** 52, 2.0 ** 53, 1.8446743e19], np.float32)])
    got = box_cox_of_root(c)
    for ci, gi in zip(c, got):
        assert f32_bits(gi) == f32_bits(box_cox_of_root_exact(ci)), (float(ci), float(gi))


def test_candidates_special_cases():
    def cset(s):
        cand, exact = box_cox_candidates(np.float32(s))
        return sorted(set(float(x) for x in cand if not np.isnan(x))), bool(np.isnan(cand).all()), bool(exact)
    assert cset(0.0) == ([-2.0], False, True) and cset(-0.0) == ([-2.0], False, True)
    for tiny in (2.0 ** -149, 1e-40, 2.0 ** -126, 2.0 ** -52, np.nextafter(np.float32(2.0 ** -50), np.float32(0))):    # roots below 2^-25
        assert cset(tiny)[0] == [-2.0], tiny
    assert cset(2.0 ** -50)[0] == [-2.0]                          # root 2^-25: the tie goes to the even -2
    assert len(cset(2.0 ** -48)[0]) == 1 and cset(2.0 ** -48)[0][0] > -2.0
    for bad in (-1.0, -1e-6, np.nan, -np.inf, -2.0 ** -149):
        assert cset(bad)[1], bad
    assert cset(np.inf) == ([np.inf], False, True)
    assert cset(1.0) == ([0.0], False, True) and cset(4.0) == ([2.0], False, True) and cset(FLT_MAX)[2] is False
    smp = directed_samples()
    cand, exact = box_cox_candidates(smp)
    sq = slice(5 + 254 + 3, 5 + 254 + 3 + 4096)
    assert exact[sq].all() and (cand[sq, 0] == cand[sq, 1]).all()
    pos = np.isfinite(smp) & (smp > 0) & ~exact                   # an inexact root: two neighbouring roots, v apart by at most 2 ulp of the root
    assert (cand[pos, 0] <= cand[pos, 1]).all()
    lo, hi, _ = sqrt_floor_ceil(smp[pos])
    assert (np.nextafter(lo, np.float32(np.inf)) == hi).all()
    assert in_candidates(nearest_box_cox(smp), cand).all()          # the correctly rounded root is always allowed


def test_oracle_values_lie_in_the_candidates(oracle):
    smp = directed_samples()
    assert smp.size > 65536
    v = oracle_box_cox(oracle, smp)
    cand, exact = box_cox_candidates(smp)
    ok = in_candidates(v, cand)
    assert ok.all(), "oracle v outside the candidates for %d samples, the first %r -> %r (allowed %r)" % (
        int((~ok).sum()), float(smp[~ok][0]), float(v[~ok][0]), cand[~ok][0].tolist())
    assert (f32_bits(v[exact]) == f32_bits(cand[exact, 0])).all()


def test_oracle_transformed_chain_is_the_plain_chain_on_its_own_values(oracle):
    """(b) on the CPU: oracle.accumulate(transform=True) equals chain_reference on the v read from the oracle by the one-sample
    trick, every plane bit for bit -- channels 1 and 3, max moment 1, 2 and 3, from a ragged host-made state."""
    for channels in (1, 3):
        for mm in (1, 2, 3):
            rng = np.random.default_rng(100 * channels + mm)
            H, W, S = 5, 12, 9
            smp = heavy_tailed_samples(rng, S, H, W, channels)
            start = random_start_state(rng, H, W, channels, rng.integers(0, 30, (H, W)))
            ref = {k: a.copy() for k, a in start.items()}
            oracle.accumulate(ref, smp, True, mm)
            v = oracle_box_cox(oracle, smp)
            assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 1
            chain = chain_reference(oracle, start, v, mm)
            assert np.array_equal(chain["n"], ref["n"])
            for k in ("mean", "m2", "m3"):
                same_bits_or_nan(ref[k], chain[k], "channels %d max moment %d %s" % (channels, mm, k))
            for k in ("m2", "m3")[mm - 1:]:
                assert np.array_equal(f32_bits(ref[k]), f32_bits(start[k])), k


def test_division_emulation_against_exact_division():
    """The emulated refined_rcp / div_by_count against Fraction division on the directed operands: the IEEE quotient wherever it
    is normal, within one step of 2^-149 where it is subnormal -- and the one-step cases exist (the finding the header states).
    Ordinary operands (the ranges test_exact_division_by_count sweeps) give the IEEE quotient for every reciprocal."""
    ds, ns = subnormal_quotient_operands(40000, 4096, seed=41)
    step = float(F32_MIN_SUB)
    off = 0
    for d, n in zip(ds[:6000], ns[:6000]):
        want = ieee_quotient(d, n)
        assert float(want) < 2.0 ** -126
        for got in allowed_quotients(d, n):
            assert abs(float(got) - float(want)) <= step, (float(d), int(n), float(got), float(want))
            off += f32_bits(got) != f32_bits(want)
    assert off > 0
    first = allowed_quotients(np.float32(1.5504638832552652e-38), 448)
    assert any(f32_bits(g) != f32_bits(ieee_quotient(np.float32(1.5504638832552652e-38), 448)) for g in first)
    rng = np.random.default_rng(8)
    for d, n in zip(rng.lognormal(0, 2.5, 1500).astype(np.float32) * rng.choice([-1, 1], 1500).astype(np.float32), rng.integers(1, 4201, 1500)):
        for got in allowed_quotients(d, n):
            assert f32_bits(got) == f32_bits(ieee_quotient(d, n)), (float(d), int(n))
    for n in (1, 2, 3):
        want = ieee_quotient(FLT_MAX, n)
        assert [f32_bits(g) for g in allowed_quotients(FLT_MAX, n)] == [f32_bits(want)] * 3, n
    for d in (np.inf, -np.inf):                                   # fma(-inf, n, inf) is NaN where inf / n is inf
        assert all(np.isnan(g) for g in allowed_quotients(np.float32(d), 7)) and ieee_quotient(np.float32(d), 7) == np.float32(d)
    # the array form, which the GPU test uses on all the directed operands, against the integer one
    dd, nn = division_operands()
    fast, quot = allowed_quotients_f32(dd, nn), ieee_quotients_f32(dd, nn)
    pick = np.concatenate([np.arange(0, 3000), np.arange(40000, 43000), np.arange(80000, dd.size)])
    for i in pick:
        slow = allowed_quotients(dd[i], nn[i])
        for k in range(3):
            assert f32_bits(slow[k]) == f32_bits(fast[k, i]) or (np.isnan(slow[k]) and np.isnan(fast[k, i])), (float(dd[i]), int(nn[i]), k)
        assert f32_bits(quot[i]) == f32_bits(ieee_quotient(dd[i], nn[i])), (float(dd[i]), int(nn[i]))
    sub = np.abs(quot[:80000]) < 2.0 ** -126
    assert sub.all() and (np.abs(fast[:, :80000].astype(np.float64) - quot[:80000]) <= step).all()
    print("div_by_count (emulated) differs from the IEEE quotient in %s of 40 000 + 40 000 subnormal quotients, by one step of 2^-149"
          % [int((f32_bits(fast[:, lo:lo + 40000]) != f32_bits(quot[lo:lo + 40000])).any(0).sum()) for lo in (0, 40000)])
