"""The small kernels of the reference's surface at their edges: statmc_prepass as a stand-alone call, statmc_prepass_pack,
statmc_calculate_mean_vars, statmc_merge_tiles, statmc_film_update and statmc_tile_moments, each against the CPU oracle bit for
bit on the inputs of tests/test_pointwise_edges_cpu.py (which holds the oracle to float64).

Two allowances, and no other:
  - where the oracle holds a NaN the device holds a NaN, of any sign and payload (the rule of tests/test_plan_gpu.py);
  - in the film update the sign of a zero that comes out of the clamp is not held -- C's fmaxf(0, -0) may return either -- so
    where a pixel took the clamp and the oracle holds a zero, the device holds a zero of either sign.
The tile scatter is a copy and gets neither: NaN payloads and -0 arrive as they left.

Second trips.  grid_for (statmc_pointwise.hip) caps a launch at 256 * 16 blocks of 256 lanes, so one pass of a grid-stride loop
covers GRID_PASS = 1 048 576 work items -- elements for mean-vars, pixels for the film update and the pre-pass + pack, groups of
four elements for the pre-pass.  The shapes under "second trips" are the smallest round ones beyond that; IF THE CAP CHANGES THEY
MUST FOLLOW IT, or the stride of every one of these loops goes unchecked again."""
import functools

import numpy as np
import pytest
import torch

from conftest import RADIUS, SD_ALBEDO, SD_NORMAL
from test_filter_per_pixel_gpu import gap_untouched, pitched
from test_pointwise_edges_cpu import (bits, film_pixels_case, frozen, mean_vars_case, merge_reference, merge_tiles_case, same_bits_or_nan,
                                      tile_values_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRID_PASS = 256 * 16 * 256                       # work items one pass of a capped grid covers (grid_for's cap x kBlock)
MAX_BUFFERS = 16                                 # STATMC_MAX_BUFFERS


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                        # (a copy: the builders' arrays are read-only)


def dev_bytes(structs):
    return torch.from_numpy(np.array(structs).view(np.uint8)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ================================================================== 1. second trips
def mean_vars_call(gpu, W, H, channels, ns, m2s, outs, quirk):
    """statmc_calculate_mean_vars itself: any number of buffers, none included."""
    gpu.check(gpu.load().statmc_calculate_mean_vars(len(ns), W, H, channels, gpu._img_array(ns), gpu._img_array(m2s), gpu._img_array(outs),
                                                    int(quirk), gpu.current_stream_handle()))


@pytest.mark.parametrize("quirk", [True, False], ids=["row-n", "pixel-n"])
@pytest.mark.parametrize("W,H,channels", [(1200, 880, 1), (600, 590, 3)])
def test_mean_vars_second_trip(gpu, oracle, W, H, channels, quirk):
    assert GRID_PASS < W * H * channels < 2 * GRID_PASS
    n, m2 = mean_vars_case(W, H, channels, seed=W)
    out = torch.full((H, W, channels), -7.0, device=DEV)
    mean_vars_call(gpu, W, H, channels, [dev(n)], [dev(m2)], [out], quirk)
    same_bits_or_nan(host(out), oracle.mean_vars(n, m2, row_n_quirk=quirk))


def same_film(got, want, px):
    """Bits, NaN for NaN, and -- where the pixel took the clamp -- a zero of either sign for a zero."""
    clamped_zero = (px["filter_weight_sum"] != 0)[:, None] & (want == 0)
    assert (got[clamped_zero] == 0).all()
    same_bits_or_nan(np.where(clamped_zero, 0, got).astype(np.float32), np.where(clamped_zero, 0, want).astype(np.float32))


def run_film_update(gpu, px, splat_scale, scale):
    out = torch.full((len(px), 3), -7.0, device=DEV)
    gpu.film_update(dev_bytes(px), len(px), out, splat_scale=splat_scale, scale=scale)
    return host(out)


def test_film_update_second_trip(gpu, oracle):
    n = GRID_PASS + 257                                                 # the second trip's last block is partial
    px = film_pixels_case(n, seed=61)
    same_film(run_film_update(gpu, px, 0.25, 1.5), oracle.film_update(px, splat_scale=0.25, scale=1.5), px)


@functools.lru_cache(maxsize=None)
def prepass_case(oracle, W, H, channels, seed):
    """Counts and moments like test_prepass_bit_exact's (tests/test_gpu_parity.py), and the oracle's pre-pass of them."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 40, (H, W)).astype(np.int32)                   # includes n = 0, 1 (discriminator = inf)
    n[0, :5] = [0, 1, 2, 4097, 100000]                                  # table edge and beyond
    n[-1, -5:] = [100000, 4097, 2, 1, 0]
    mean = rng.standard_normal((H, W, channels)).astype(np.float32)
    m2 = rng.random((H, W, channels), dtype=np.float32)
    m2[1, :4] = 0.0                                                     # zero variance
    m3 = rng.standard_normal((H, W, channels)).astype(np.float32)
    mean[2, 3] = np.nan                                                 # negative sample upstream
    mean[-1, -2] = np.nan
    mc, dc = oracle.prepass(n, mean, m2, m3)
    return frozen(n, mean, m2, m3, mc, dc)


def run_prepass(gpu, n, mean, m2, m3, mc, dc, channels):
    a, keep = gpu.make_filter_args([n], [mean], [m2], [m3], [], [mc], [dc], [], [], g_sds=[], radius=1)
    gpu.prepass(a, channels)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "mean_corr-4-bytes-off"])
def test_prepass_second_trip(gpu, oracle, off):
    """2051 x 2047 x 1: more than four passes' worth of elements and no multiple of 4.  Aligned: prepass_kernel<true> and its
    scalar tail.  mean_corr four bytes off the 16-byte grid: prepass_kernel<false>, the element path, over two trips."""
    W, H = 2051, 2047
    assert W * H > 4 * GRID_PASS and W * H % 4
    n, mean, m2, m3, mc_ref, dc_ref = prepass_case(oracle, W, H, 1, seed=12)
    base = torch.full((W * H + 8,), -7.0, device=DEV)
    mc, dc = base[off:off + W * H].view(H, W, 1), torch.full((H, W, 1), -7.0, device=DEV)
    assert mc.data_ptr() % 16 == 4 * off and dc.data_ptr() % 16 == 0
    run_prepass(gpu, dev(n), dev(mean), dev(m2), dev(m3), mc, dc, 1)
    same_bits_or_nan(host(mc), mc_ref)
    same_bits_or_nan(host(dc), dc_ref)
    assert bool((base[:off] == -7).all()) and bool((base[off + W * H:] == -7).all())


def test_prepass_pack_second_trip(gpu, oracle):
    """A 1032 x 1020 RGB block (1 052 640 pixels) into a 15-channel image of its own size: the bits of statmc_prepass followed by
    statmc_pack_filter_inputs, by-products included, and the oracle's pre-pass."""
    W, H = 1032, 1020
    assert GRID_PASS < W * H < 2 * GRID_PASS
    n, mean, m2, m3, mc_ref, dc_ref = prepass_case(oracle, W, H, 3, seed=13)
    rng = np.random.default_rng(14)
    film, g0, g1 = (torch.from_numpy(rng.standard_normal((H, W, 3)).astype(np.float32)).to(DEV) for _ in range(3))
    d = [dev(x) for x in (n, mean, m2, m3)]
    z = lambda: torch.full((H, W, 3), -7.0, device=DEV)
    mc, dc, mc2, dc2 = z(), z(), z(), z()
    out = torch.zeros(H, W, 3, device=DEV)
    a, keep = gpu.make_filter_args([d[0]], [d[1]], [d[2]], [d[3]], [film], [mc], [dc], [out], [g0, g1], g_sds=[SD_NORMAL, SD_ALBEDO], radius=RADIUS)
    gpu.prepass(a, 3)
    two_steps = torch.full((H, W, 15), float("nan"), device=DEV)
    gpu.pack_filter_inputs(a, two_steps, 0, 0)
    a2, keep2 = gpu.make_filter_args([d[0]], [d[1]], [d[2]], [d[3]], [film], [mc2], [dc2], [out], [g0, g1], g_sds=[SD_NORMAL, SD_ALBEDO], radius=RADIUS)
    one_step = torch.full((H, W, 15), float("nan"), device=DEV)
    gpu.prepass_pack(a2, one_step, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(one_step.view(torch.int32), two_steps.view(torch.int32))
    assert torch.equal(mc2.view(torch.int32), mc.view(torch.int32)) and torch.equal(dc2.view(torch.int32), dc.view(torch.int32))
    same_bits_or_nan(host(mc2), mc_ref)
    same_bits_or_nan(host(dc2), dc_ref)
    got = host(one_step)
    assert np.array_equal(bits(got[..., 6:]), bits(np.concatenate([host(film), host(g0), host(g1)], axis=2)))
    same_bits_or_nan(got[..., :3], mc_ref)
    same_bits_or_nan(got[..., 3:6], dc_ref)


# ================================================================== 2. mean-vars, the rest
@pytest.mark.parametrize("W,H", [(31, 9), (1, 1), (1, 37), (41, 1)])
@pytest.mark.parametrize("n_buffers", [0, 2, 5])
def test_mean_vars_buffers_and_thin_films(gpu, oracle, W, H, n_buffers):
    for channels in (1, 3):
        for quirk in (True, False):
            cases = [mean_vars_case(W, H, channels, seed=100 + b) for b in range(n_buffers)]
            outs = [torch.full((H, W, channels), -7.0, device=DEV) for _ in cases]
            mean_vars_call(gpu, W, H, channels, [dev(n) for n, _ in cases], [dev(m2) for _, m2 in cases], outs, quirk)
            for b, ((n, m2), out) in enumerate(zip(cases, outs)):
                same_bits_or_nan(host(out), oracle.mean_vars(n, m2, row_n_quirk=quirk), (channels, quirk, b))


def run_mean_vars(gpu, cases, W, H, channels, quirk, pitch):
    """The call on packed images, or (pitch) on images with a row pitch of their own each, NaN (-7 for n) between the rows.
    Returns the results as host arrays."""
    m = (lambda t, pad: pitched(t, pad)) if pitch else (lambda t, pad: t)
    ns = [m(dev(n), 1 + b % 3) for b, (n, _) in enumerate(cases)]
    m2s = [m(dev(m2), 2 + b % 2) for b, (_, m2) in enumerate(cases)]
    outs = [m(torch.full((H, W, channels), -7.0, device=DEV), 1 + b % 4) for b in range(len(cases))]
    mean_vars_call(gpu, W, H, channels, ns, m2s, outs, quirk)
    torch.cuda.synchronize()
    if pitch:
        assert all(gap_untouched(t) for t in m2s + outs)
        for t in ns:
            wide = torch.as_strided(t, (H, t.stride(0)), t.stride())
            assert bool((wide[:, W:] == -7).all())
    return [host(t.contiguous()) for t in outs]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n_buffers", [1, 3, MAX_BUFFERS + 1], ids=["1", "3", "17-above-max-buffers"])
def test_mean_vars_pitched_equals_packed(gpu, oracle, channels, n_buffers):
    """Pitched n / m2 / film_var: the packed call's bits, the gaps between the rows untouched.  17 buffers, one more than
    STATMC_MAX_BUFFERS: served like any other count, packed and pitched alike (include/statmc.h says so at the entry; the
    reference passes a uchar)."""
    W, H = 29, 11
    cases = [mean_vars_case(W, H, channels, seed=200 + b) for b in range(n_buffers)]
    for quirk in (True, False):
        packed, with_pitch = (run_mean_vars(gpu, cases, W, H, channels, quirk, p) for p in (False, True))
        for b, (n, m2) in enumerate(cases):
            want = oracle.mean_vars(n, m2, row_n_quirk=quirk)
            same_bits_or_nan(packed[b], want, ("packed", quirk, b))
            assert np.array_equal(bits(with_pitch[b]), bits(packed[b])), (quirk, b)
    assert not np.array_equal(bits(packed[0]), bits(packed[-1])) or n_buffers == 1     # every buffer has contents of its own


# ================================================================== 3. film update, the rest
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_film_update_block_edges(gpu, oracle, n):
    px = film_pixels_case(n, seed=70 + n)
    same_film(run_film_update(gpu, px, 0.25, 1.5), oracle.film_update(px, splat_scale=0.25, scale=1.5), px)


@pytest.mark.parametrize("splat_scale,scale", [(0.25, 0.0), (0.0, 1.5), (-2.0, -0.5)], ids=["scale-0", "splat_scale-0", "negative"])
def test_film_update_zero_scales(gpu, oracle, splat_scale, scale):
    px = film_pixels_case(4099, seed=23)
    same_film(run_film_update(gpu, px, splat_scale, scale), oracle.film_update(px, splat_scale=splat_scale, scale=scale), px)


def test_film_update_alignment(gpu, oracle):
    """An output that starts four bytes into its allocation and a pixel array that starts sixteen bytes into its own give the
    aligned call's bits; a pixel array four bytes in is refused (the kernel reads it as float4) and nothing is written."""
    n = 771
    px = film_pixels_case(n, seed=77)
    want = oracle.film_update(px, splat_scale=0.5, scale=2.0)
    raw = torch.zeros(32 * n + 32, dtype=torch.uint8, device=DEV)
    out = torch.full((3 * n + 2,), -7.0, device=DEV)
    for px_off, out_off in ((0, 1), (16, 0), (16, 1)):
        raw[px_off:px_off + 32 * n] = dev_bytes(px)
        out.fill_(-7.0)
        src, dst = raw[px_off:px_off + 32 * n], out[out_off:out_off + 3 * n]
        assert src.data_ptr() % 32 == px_off and dst.data_ptr() % 16 == 4 * out_off
        gpu.film_update(src, n, dst, splat_scale=0.5, scale=2.0)
        same_film(host(dst).reshape(n, 3), want, px)
        assert bool((out[:out_off] == -7).all()) and bool((out[out_off + 3 * n:] == -7).all())
    raw[4:4 + 32 * n] = dev_bytes(px)
    out.fill_(-7.0)
    with pytest.raises(gpu.StatmcError) as e:
        gpu.film_update(raw[4:4 + 32 * n], n, out, splat_scale=0.5, scale=2.0)
    assert e.value.code == gpu.ERR_INVALID
    assert bool((host(out) == -7).all())


# ================================================================== 4. tile moments, the rest
def run_tile_moments(gpu, v, ts):
    H, W, c = v.shape
    out = torch.full((-(-H // ts), -(-W // ts), c, 3), -7.0, device=DEV)
    gpu.tile_moments(dev(v), ts, out)
    return host(out)


@pytest.mark.parametrize("ts", [8, 16])
@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (7, 16), (32, 16), (50, 37)], ids=["1x1", "5x3", "7x16", "32x16-exact", "50x37"])
def test_tile_moments_channels_and_films(gpu, oracle, W, H, ts):
    """Channels 1, 2 and 4; films smaller than a tile in one direction or both, an exact multiple of the tile, a ragged one; a
    mean that is small and one that is large against the spread."""
    for channels in (1, 2, 4):
        for offset in (0, 1e5):
            v = tile_values_case(W, H, channels, offset, seed=300 + channels)
            same_bits_or_nan(run_tile_moments(gpu, v, ts), oracle.tile_moments(v, ts), (channels, offset))


@pytest.mark.parametrize("ts", [8, 16])
def test_tile_moments_every_case(gpu, oracle, ts):
    """Every tile_values_case at 50 x 37 x 4: the three offsets, and the variant with a NaN, a +inf and a constant tile -- M2 == 0
    and the mean exactly the constant, at offset 0 and at 1e5."""
    W, H = 50, 37
    for offset in (0, 1e3, 1e5):
        v = tile_values_case(W, H, 4, offset, seed=31)
        same_bits_or_nan(run_tile_moments(gpu, v, ts), oracle.tile_moments(v, ts), offset)
    for offset in (0, 1e5):
        v = tile_values_case(W, H, 4, offset, seed=32, special=True)
        got, want = run_tile_moments(gpu, v, ts), oracle.tile_moments(v, ts)
        assert np.isnan(want).any()
        same_bits_or_nan(got, want, ("special", offset))
        const = got[32 // ts:, 48 // ts:]
        assert (const[..., 2] == 0).all() and np.array_equal(const[..., 1], np.broadcast_to(v[36, 49], const[..., 1].shape))


@pytest.mark.parametrize("ts,channels", [(0, 3), (4, 3), (12, 3), (32, 3), (-8, 3), (8, 0), (8, 5), (16, -1)])
def test_tile_moments_refusals(gpu, ts, channels):
    """Tile sizes other than 8 and 16 and channel counts outside 1 .. 4 are refused, and the output is untouched."""
    v = dev(tile_values_case(20, 9, 5, 0, seed=33))
    out = torch.full((3 * 2 * 5 * 3,), -7.0, device=DEV)
    rc = gpu.load().statmc_tile_moments(20, 9, channels, v.data_ptr(), ts, out.data_ptr(), gpu.current_stream_handle())
    assert rc == gpu.ERR_INVALID and bool((host(out) == -7).all())
    with pytest.raises(gpu.StatmcError) as e:
        gpu.check(rc)
    assert e.value.code == gpu.ERR_INVALID


# ================================================================== 5. the tile scatter, the rest
def run_merge(gpu, W, H, channels, transform, bounds, offsets, pixels, max_tile_pixels, fill=-7):
    st = {k: torch.full((H, W) if k == "n" else (H, W, channels), fill, dtype=torch.int32 if k == "n" else torch.float32, device=DEV)
          for k in ("n", "mean", "m2", "m3", "film_mean", "film_m2")}
    gpu.merge_tiles(W, H, channels, transform, dev_bytes(pixels), dev(bounds), dev(offsets), max_tile_pixels, st)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in st.items()}


def same_state(got, want):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k           # a copy: no allowance, NaN payloads and -0 included


TILINGS = [((32, 32, False), 1024, "32x32-blocks-in-x"), ((32, 32, False), 256, "32x32-understated-max-loop"), ((64, 8, False), 512, "64x8"),
           ((1, 1, False), 1, "1x1"), ((70, 45, False), 70 * 45, "whole-film"), ((16, 16, True), 256, "partial-cover")]


@pytest.mark.parametrize("channels,transform", [(1, False), (1, True), (3, False), (3, True)])
@pytest.mark.parametrize("tiling,max_tile_pixels", [t[:2] for t in TILINGS], ids=[t[2] for t in TILINGS])
def test_merge_tiles_tilings(gpu, oracle, tiling, max_tile_pixels, channels, transform):
    """Tiles of more than one block, of more pixels than the grid is sized by (the in-kernel loop), wider than high, of one pixel,
    the whole film, and a partial cover -- stored in shuffled order.  n is the low 32 bits of the 64-bit count; pixels no tile
    covers, and without the transform the film images, keep their prefill."""
    W, H = 70, 45
    bounds, offsets, pixels = merge_tiles_case(W, H, channels, tiling, seed=41)
    want = merge_reference(oracle, W, H, channels, transform, bounds, offsets, pixels)
    got = run_merge(gpu, W, H, channels, transform, bounds, offsets, pixels, max_tile_pixels)
    same_state(got, want)
    if not transform:
        assert (got["film_mean"] == -7).all() and (got["film_m2"] == -7).all()
    if tiling[2]:
        assert (got["n"] == -7).sum() > W * H // 3


def test_merge_tiles_at_the_tile_limit(gpu, oracle):
    """65 535 tiles (a 255 x 257 film of 1 x 1 tiles) are served; 65 536 (256 x 256) are refused and the state is untouched."""
    W, H = 255, 257
    bounds, offsets, pixels = merge_tiles_case(W, H, 3, (1, 1, False), seed=43)
    assert len(bounds) == 65535
    same_state(run_merge(gpu, W, H, 3, True, bounds, offsets, pixels, 1), merge_reference(oracle, W, H, 3, True, bounds, offsets, pixels))
    W, H = 256, 256
    bounds, offsets, pixels = merge_tiles_case(W, H, 1, (1, 1, False), seed=44)
    assert len(bounds) == 65536
    st = {k: torch.full((H, W) if k == "n" else (H, W, 1), -7, dtype=torch.int32 if k == "n" else torch.float32, device=DEV)
          for k in ("n", "mean", "m2", "m3", "film_mean", "film_m2")}
    with pytest.raises(gpu.StatmcError) as e:
        gpu.merge_tiles(W, H, 1, True, dev_bytes(pixels), dev(bounds), dev(offsets), 1, st)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in st.values())
