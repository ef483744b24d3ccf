"""The inputs of tests/test_pointwise_edges_gpu.py, and the checks that keep the oracle honest where that file holds the device
to the oracle's bits: the small kernels of the reference's surface -- mean-vars, film update, tile moments, the tile scatter.

Builders.  mean_vars_case, film_pixels_case, tile_values_case and merge_tiles_case are seeded, return read-only arrays (they are
cached and shared between tests) and assert that the classes of value they plant are in what they return, wherever the case is
large enough to hold them all.

Against float64.  The oracle's mean-vars, film update and tile moments are compared with plain float64 NumPy restatements of the
formulas in include/statmc.h, under bounds that follow from the number of float roundings (u = 2^-24), and its tile scatter with
a NumPy scatter bit for bit.  No device is needed."""
import functools

import numpy as np
import pytest

from oracle import oracle as _o
from test_device_reduce_gpu import check_union_rule                     # (importing it needs no device)

U = 2.0 ** -24                                   # the unit roundoff of float
F32 = np.float32
N_SPECIAL = (0, 1, -3, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31 - 1)
WEIGHTS = (0.0, 1.0, 2.0, 3.0, 0.37, 5e-3)
WEIGHTS_PLANTED = (-1.0, 1e-42, np.inf, np.nan)
TILE_COUNTS = (0, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 5)
NAN_PAYLOADS = (0x7FC12345, 0xFFA00001, 0x7F800001, 0xFFFFFFFF)      # quiet and signalling, both signs
XYZ_TO_RGB = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], F32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def same_bits_or_nan(got, want, what=""):
    """Bit for bit, with the one allowance of tests/test_plan_gpu.py: where `want` holds a NaN, `got` holds a NaN of any sign
    and payload."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(bits(got)[nan == 0], bits(want)[nan == 0]), what


# ------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def mean_vars_case(W, H, channels, seed):
    """(n [H, W] int32, m2 [H, W, channels] float32).  n: 2 .. 300, a tenth of the pixels from N_SPECIAL (where (nf - 1) nf is -0,
    0, negative-times-negative, or rounds), the first column of rows 1, 5, ... 0 and of rows 2, 6, ... 1 so that the row quirk
    reads them; m2: [0, 50) with an eighth of the elements 0, negative, 1e-42 (subnormal), NaN and +inf in turn."""
    rng = np.random.default_rng(seed)
    n = rng.integers(2, 301, (H, W)).astype(np.int32)
    idx = rng.permutation(W * H)[:W * H // 10]
    n.reshape(-1)[idx] = np.array(N_SPECIAL, np.int64)[np.arange(len(idx)) % len(N_SPECIAL)].astype(np.int32)
    n[1::4, 0] = 0
    n[2::4, 0] = 1
    m2 = (rng.random((H, W, channels)) * 50).astype(F32)
    flat = m2.reshape(-1)
    idx2 = rng.permutation(flat.size)[:flat.size // 8]
    kind = np.arange(len(idx2)) % 5
    flat[idx2[kind == 0]] = 0.0
    flat[idx2[kind == 1]] *= F32(-1)
    flat[idx2[kind == 2]] = F32(1e-42)
    flat[idx2[kind == 3]] = np.nan
    flat[idx2[kind == 4]] = np.inf
    if len(idx) >= 4 * len(N_SPECIAL):
        assert all((n == v).any() for v in N_SPECIAL)
    if H >= 3:
        assert (n[:, 0] == 0).any() and (n[:, 0] == 1).any()
    if len(idx2) >= 5:
        assert (m2 == 0).any() and (m2 < 0).any() and (m2 == F32(1e-42)).any() and np.isnan(m2).any() and np.isposinf(m2).any()
        assert 0 < float(F32(1e-42)) < 2.0 ** -126
    return frozen(n, m2)


@functools.lru_cache(maxsize=None)
def film_pixels_case(n, seed):
    """n Film::Pixel structs (oracle.FILM_PIXEL_DTYPE): XYZ normal(0, 2) -- negative RGB exists --, weights from WEIGHTS with up to
    sixteen pixels from WEIGHTS_PLANTED (negative, subnormal: 1 / w = inf, +inf, NaN), a splat normal(0, 1) on about 30 % of the
    pixels, NaN in up to three of them, pad NaN."""
    rng = np.random.default_rng(seed)
    px = np.zeros(n, dtype=_o.FILM_PIXEL_DTYPE)
    px["xyz"] = rng.normal(0, 2, (n, 3))
    w = rng.choice(np.array(WEIGHTS, F32), n)
    idx = rng.permutation(n)[:min(16, n // 8)]
    w[idx] = np.array(WEIGHTS_PLANTED, F32)[np.arange(len(idx)) % len(WEIGHTS_PLANTED)]
    px["filter_weight_sum"] = w
    has_splat = rng.random(n) < 0.3
    splat = (rng.normal(0, 1, (n, 3)) * has_splat[:, None]).astype(F32)
    where = np.flatnonzero(has_splat)
    for k, i in enumerate(where[:min(3, len(where) // 4)]):
        splat[i, k % 3] = np.nan
    px["splat_xyz"] = splat
    px["pad"] = np.nan
    if n >= 255:
        w = px["filter_weight_sum"]
        assert all((w == F32(v)).any() for v in WEIGHTS + WEIGHTS_PLANTED[:3]) and np.isnan(w).any()
        rgb = px["xyz"].astype(np.float64) @ XYZ_TO_RGB.astype(np.float64).T
        assert (rgb < 0).any() and ((rgb < 0) & (w == 0)[:, None]).any() and ((rgb < 0) & (w < 0)[:, None]).any()
        assert 0.2 < has_splat.mean() < 0.4 and np.isnan(px["splat_xyz"]).any() and (px["splat_xyz"][~has_splat] == 0).all()
    return frozen(px)


@functools.lru_cache(maxsize=None)
def tile_values_case(W, H, channels, offset, seed, special=False):
    """[H, W, channels] float32: offset + lognormal(0, 1) -- at offset 1e3 and 1e5 the mean is large against the spread, what
    Welford / Chan exist for.  special (W, H > 16): the last 16-aligned tile (ragged where the film is) holds one constant per
    channel, and outside it one value is NaN and one +inf."""
    rng = np.random.default_rng(seed)
    v = (offset + rng.lognormal(0, 1, (H, W, channels))).astype(F32)
    if offset and v.size >= 64:
        assert float(v.astype(np.float64).std()) < 0.01 * offset
    if special:
        assert W > 16 and H > 16
        x0, y0 = (W - 1) // 16 * 16, (H - 1) // 16 * 16
        v[y0:, x0:] = (offset + 0.75 + np.arange(channels)).astype(F32)
        v[1, 2, 0] = np.nan
        v[9, W // 2 - 1, channels - 1] = np.inf
        assert np.isnan(v).sum() == 1 and np.isposinf(v).sum() == 1 and np.isfinite(v[y0:, x0:]).all()
    return frozen(v)


def tile_grid(W, H, tw, th):
    return [(x0, y0, min(x0 + tw, W), min(y0 + th, H)) for y0 in range(0, H, th) for x0 in range(0, W, tw)]


@functools.lru_cache(maxsize=None)
def merge_tiles_case(W, H, channels, tiling, seed):
    """(bounds [T, 4] int32, offsets [T] int64, pixels: AoS oracle.TILE_PIXEL_DTYPE[channels]).  tiling = (tile width, tile height,
    partial): the film cut into such tiles in raster order, ragged at the right and bottom edge; partial keeps every other tile.
    The tiles lie in `pixels` in a shuffled order with one unused pixel ahead of each, so offsets is neither monotonic nor the
    running sum of the tile sizes.  Every byte is random -- the floats are random bit patterns, NaNs with payloads among them, the
    64-bit counts mostly above 2^32 -- and NAN_PAYLOADS, -0.0 and TILE_COUNTS are planted in pixels that are used."""
    tw, th, partial = tiling
    rng = np.random.default_rng(seed)
    dt = _o.TILE_PIXEL_DTYPE[channels]
    tiles = tile_grid(W, H, tw, th)[::2 if partial else 1]
    T = len(tiles)
    npx = np.array([(x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in tiles], np.int64)
    order = rng.permutation(T)
    if T >= 3 and (np.diff(order) > 0).all():
        order = order[::-1]
    offsets = np.zeros(T, np.int64)
    offsets[order] = np.cumsum(npx[order] + 1) - npx[order]
    total = int(npx.sum()) + T + 1
    pixels = rng.integers(0, 256, total * dt.itemsize, dtype=np.uint8).view(dt)
    used = np.repeat(offsets, npx) + (np.arange(npx.sum()) - np.repeat(np.cumsum(npx) - npx, npx))
    pick = used[rng.permutation(len(used))[:16]]
    if len(pick) == 16:
        pixels["n"][pick[:4]] = np.array(TILE_COUNTS, np.uint64)
        pixels["mean"][pick[4:6]] = -0.0
        pixels["film_m2"][pick[6:8]] = -0.0
        for k, f in enumerate(("mean", "m2", "m3", "film_mean")):
            pixels[f].view(np.uint32)[pick[8 + k]] = NAN_PAYLOADS[k]
        nan_bits = np.concatenate([pixels[f].view(np.uint32)[used].reshape(-1) for f in ("mean", "m2", "m3", "film_mean", "film_m2")])
        assert all((nan_bits == p).any() for p in NAN_PAYLOADS) and (nan_bits == 0x80000000).any()
        assert all((pixels["n"][used] == v).any() for v in TILE_COUNTS)
    if T >= 3:
        assert (np.diff(offsets) < 0).any()
    assert len(np.unique(used)) == len(used) and used.max() < total
    return frozen(np.array(tiles, np.int32).reshape(T, 4), offsets, pixels)


def prefilled_state(W, H, channels, fill=-7):
    st = _o.new_state(H, W, channels)
    for k in st:
        st[k][...] = fill
    return st


def merge_reference(oracle, W, H, channels, transform, bounds, offsets, pixels, fill=-7):
    """oracle.merge_tile per tile, into a state that holds `fill` everywhere."""
    st = prefilled_state(W, H, channels, fill)
    for (x0, y0, x1, y1), off in zip(bounds.tolist(), offsets.tolist()):
        oracle.merge_tile(pixels[off:off + (x1 - x0) * (y1 - y0)], channels, x0, y0, x1, y1, st, transform=transform)
    return st


# ------------------------------------------------------------------ mean-vars against float64
def mean_vars_f64(n, m2, quirk):
    """film_m2 / ((n - 1) n) in float64 over the count as the formula reads it: converted to float first (estimator.cpp:540), one
    per row under the quirk.  Returns (value, the count used per pixel)."""
    used = np.broadcast_to(n[:, :1], n.shape) if quirk else n
    nf = used.astype(F32).astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return m2.astype(np.float64) / ((nf - 1) * nf), used


@pytest.mark.parametrize("quirk", [False, True])
@pytest.mark.parametrize("W,H,channels", [(31, 9, 1), (40, 23, 3)])
def test_mean_vars_oracle_against_float64(oracle, W, H, channels, quirk):
    """Three roundings -- nf - 1, the product, the quotient -- so 3 u relative where the count is neither 0 nor 1 and m2 is finite,
    plus half a subnormal step (2^-150) where the quotient underflows (m2 = 1e-42).  Where the count used is 0 or 1 the
    denominator is -0 or 0 and the result is an infinity or a NaN."""
    n, m2 = mean_vars_case(W, H, channels, seed=5)
    got = oracle.mean_vars(n, m2, row_n_quirk=quirk)
    want, used = mean_vars_f64(n, m2, quirk)
    degenerate = np.broadcast_to(((used == 0) | (used == 1))[..., None], m2.shape)
    ok = np.isfinite(m2) & ~degenerate
    assert ok.sum() > m2.size // 3 and degenerate.any()
    err = np.abs(got.astype(np.float64)[ok] - want[ok])
    print("mean-vars: worst error %.3f u" % float((err / np.maximum(np.abs(want[ok]), 2.0 ** -126)).max() / U))
    assert (err <= 3 * U * np.abs(want[ok]) + 2.0 ** -150).all()
    assert not np.isfinite(got[degenerate]).any()
    assert np.array_equal(np.isnan(got[~degenerate]), np.isnan(m2[~degenerate]))
    if W > 1:
        other = oracle.mean_vars(n, m2, row_n_quirk=not quirk)
        assert not np.array_equal(bits(got), bits(other))               # the case tells the two rules apart


# ------------------------------------------------------------------ film update against float64
def film_update_f64(px, splat_scale, scale):
    """include/statmc.h: XYZ -> RGB, / weight where it is not 0, clamp >= 0, + splat_scale * splat RGB, * scale -- in float64,
    with the float constants and float splat_scale / scale widened.  Returns (value, the magnitude the error bound scales with:
    |scale| (sum_j |m_ij x_j| / |w| + |splat_scale| sum_j |m_ij s_j|))."""
    M = XYZ_TO_RGB.astype(np.float64)
    ss, sc = float(F32(splat_scale)), float(F32(scale))
    xyz, s = px["xyz"].astype(np.float64), px["splat_xyz"].astype(np.float64)
    w = px["filter_weight_sum"].astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        rgb = xyz @ M.T
        mag = np.abs(xyz) @ np.abs(M).T
        rgb = np.where(w != 0, np.maximum(0, rgb / w), rgb)
        mag = np.where(w != 0, mag / np.abs(w), mag)
        return (rgb + ss * (s @ M.T)) * sc, abs(sc) * (mag + abs(ss) * (np.abs(s) @ np.abs(M).T))


@pytest.mark.parametrize("splat_scale,scale", [(0.25, 1.5), (-3.0, 0.3), (0.0, 1.0), (1.0, 0.0)])
def test_film_update_oracle_against_float64(oracle, splat_scale, scale):
    """The longest path from an input to the output has seven roundings (product, two sums, reciprocal, product, sum, product),
    so |out - want| <= 8 u |scale| (sum_j |m_ij x_j| / |w| + |splat_scale| sum_j |m_ij s_j|); the eighth unit covers the
    second-order terms.  Over the pixels whose XYZ, weight and splat are finite and whose weight has a finite reciprocal."""
    px = film_pixels_case(4099, seed=23)
    got = oracle.film_update(px, splat_scale=splat_scale, scale=scale).astype(np.float64)
    want, mag = film_update_f64(px, splat_scale, scale)
    w = px["filter_weight_sum"]
    ok = np.isfinite(px["xyz"]).all(1) & np.isfinite(px["splat_xyz"]).all(1) & np.isfinite(w) & ((w == 0) | (np.abs(w) >= 2.0 ** -126))
    assert ok.sum() > 4000 and (~ok).sum() >= 12 and (w[ok] < 0).any()
    err = np.abs(got[ok] - want[ok])
    print("film update: worst error %.2f of the bound's 8 units" % float((err / np.maximum(mag[ok] * U, 1e-300)).max()))
    assert (err <= 8 * U * mag[ok]).all()
    # a subnormal weight: 1 / w is +inf, the clamp leaves +inf or 0 (from -inf and from NaN = 0 * inf), then the splat and the scale
    tiny = (w > 0) & (w < 2.0 ** -126) & np.isfinite(px["splat_xyz"]).all(1)
    assert tiny.any()
    if scale != 0:
        splat_only = ((F32(0) + F32(splat_scale) * (px["splat_xyz"][tiny].astype(np.float64) @ XYZ_TO_RGB.astype(np.float64).T)) * scale)
        g = got[tiny]
        assert (np.isinf(g) | (np.abs(g - splat_only) <= 8 * U * np.abs(splat_only) + 1e-30)).all() and np.isinf(g).any()
    if scale == 0:
        assert (got[ok] == 0).all()


# ------------------------------------------------------------------ tile moments against float64
def tile_moments_f64(v, ts):
    """Float64 two-pass {count, mean, M2} per tile and channel: [tiles_y, tiles_x, C, 3]."""
    H, W, Cn = v.shape
    out = np.zeros((-(-H // ts), -(-W // ts), Cn, 3))
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            blk = v[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts].astype(np.float64).reshape(-1, Cn)
            out[j, i, :, 0] = len(blk)
            with np.errstate(invalid="ignore"):
                out[j, i, :, 1] = blk.mean(0)
                out[j, i, :, 2] = ((blk - blk.mean(0)) ** 2).sum(0)
    return out


def tile_moments_sequential(v, ts):
    """Float Welford over the tile's pixels in raster order, one rounding per operation: the sequential accumulation the tree is
    measured against."""
    H, W, Cn = v.shape
    out = np.zeros((-(-H // ts), -(-W // ts), Cn, 3), F32)
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            blk = v[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts].reshape(-1, Cn)
            mean, m2 = np.zeros(Cn, F32), np.zeros(Cn, F32)
            for k, x in enumerate(blk):
                d = x - mean
                mean = mean + d / F32(k + 1)
                m2 = m2 + d * (x - mean)
            out[j, i, :, 0], out[j, i, :, 1], out[j, i, :, 2] = len(blk), mean, m2
    return out


def check_tile_moments_union(got, v, ts, what):
    """The project's rule, check_union_rule: per field, the tree is at most twice as far (relative L2) from the float64 two-pass
    moments of the tiles as the sequential float accumulation is, + 1e-6.  Counts are exact."""
    ref, sq = tile_moments_f64(v, ts), tile_moments_sequential(v, ts)
    assert np.array_equal(got[..., 0], ref[..., 0]), what
    split = lambda a: {"mean": a[..., 1], "m2": a[..., 2]}
    check_union_rule(split(got), split(sq), split(ref), ["mean", "m2"], what)


@pytest.mark.parametrize("ts", [8, 16])
@pytest.mark.parametrize("offset", [0, 1e3, 1e5])
def test_tile_moments_oracle_against_float64(oracle, offset, ts):
    v = tile_values_case(50, 37, 4, offset, seed=31)
    check_tile_moments_union(oracle.tile_moments(v, ts), v, ts, "offset %g, tile %d" % (offset, ts))


@pytest.mark.parametrize("ts", [8, 16])
def test_tile_moments_oracle_special_values(oracle, ts):
    """The constant tile gives M2 == 0 and its constant as the mean, exactly, at any offset; the tiles that hold the NaN and the
    +inf give NaN moments in that channel only, and the right count."""
    for offset in (0, 1e5):
        v = tile_values_case(50, 37, 4, offset, seed=32, special=True)
        out = oracle.tile_moments(v, ts)
        const = out[32 // ts:, 48 // ts:]
        assert (const[..., 2] == 0).all() and np.array_equal(const[..., 1], np.broadcast_to(v[36, 49], const[..., 1].shape))
        bad = np.zeros(out.shape[:3], bool)
        bad[1 // ts, 2 // ts, 0] = True
        bad[9 // ts, 24 // ts, 3] = True
        assert np.isnan(out[bad][:, 1:]).all() and np.isfinite(out[~bad]).all()
        assert np.array_equal(out[..., 0], tile_moments_f64(v, ts)[..., 0])


# ------------------------------------------------------------------ the tile scatter against NumPy
@pytest.mark.parametrize("channels,transform", [(1, True), (3, False), (3, True)])
@pytest.mark.parametrize("tiling", [(32, 32, False), (64, 8, False), (1, 1, False), (70, 45, False), (16, 16, True)])
def test_merge_tile_oracle_is_a_copy(oracle, channels, transform, tiling):
    """oracle.merge_tile per tile against a NumPy scatter of the same structs: every field arrives with its bits (NaN payloads,
    -0), n is the low 32 bits of the 64-bit count, pixels no tile covers keep their prefill, and without the transform the film
    images do too."""
    W, H = 70, 45
    bounds, offsets, pixels = merge_tiles_case(W, H, channels, tiling, seed=41)
    got = merge_reference(oracle, W, H, channels, transform, bounds, offsets, pixels)
    want = prefilled_state(W, H, channels)
    covered = np.zeros((H, W), bool)
    for (x0, y0, x1, y1), off in zip(bounds.tolist(), offsets.tolist()):
        t = pixels[off:off + (x1 - x0) * (y1 - y0)].reshape(y1 - y0, x1 - x0)
        want["n"][y0:y1, x0:x1] = (t["n"] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        for k in ("mean", "m2", "m3") + (("film_mean", "film_m2") if transform else ()):
            want[k][y0:y1, x0:x1] = t[k].reshape(y1 - y0, x1 - x0, channels)
        covered[y0:y1, x0:x1] = True
    assert covered.all() != tiling[2]
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert (got["n"][~covered] == -7).all() and (transform or (got["film_mean"] == -7).all())
