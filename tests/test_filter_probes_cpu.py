"""The two probes that make a per-pixel check of the window filter sharp (tests/test_filter_per_pixel_gpu.py runs them
on every kernel), pinned here on the CPU oracle alone.

Membership probe.  With filter_sd = 1e18 and every G-buffer factor 0 each tap's exponent is -5e-37 * r^2: a normal float
whose exp is exactly 1.  With a colour image of integers 0 .. 15 the sums are then the member count and an integer below
2^24 -- exact in float in ANY summation order -- and the output is one IEEE division.  So a filter that takes the
oracle's tap decisions returns the oracle's bits, whatever its tiling, and one that drops, repeats or mis-judges a single
tap does not.  Here: the float oracle equals a brute-force integer reference (NumPy, the spec's membership rule written
out again) bit for bit, on real noisy statistics that reject most taps, with the pixels that take no part planted.

Weight probe.  With an infinite discriminator every valid tap is a member and the filter is a plain cross-bilateral one;
a float64 NumPy reference measures the float oracle's own rounding error e_or, the unit the kernels' error is bounded in.
oracle.filter_image_f64 (the oracle's tap decisions, weights and sums in double) extends that measure to gated windows; it
is checked here against the NumPy reference and against the integer reference."""
import numpy as np
import pytest

from conftest import FILTER_SD, SD_ALBEDO, SD_NORMAL, make_case

PROBE_SD = 1e18                                  # ds = -5e-37: ds * r^2 (r^2 <= 1152) is a normal float, exp(ds * r^2) == 1
PROBE_DS = -0.5 / PROBE_SD ** 2


# ------------------------------------------------------------------ inputs of the probes
def noisy_stats(oracle, W, H, spp, seed, features=("radiance", "normal", "albedo"), spec=None, channels=3, tighten=1):
    """Statistics of a synthetic film at a low sample count: (n, mean_corr, disc, colour, {feature: mean}).  The synthetic
    scenes' own intervals reject about 1 % of the taps of a window; tighten = 16 divides the discriminator by 16 (the intervals
    of 16 times the samples around the same noisy means) and the gate rejects about half of them, along the image's structure."""
    _, smp, st = make_case(W, H, spp, seed=seed, features=features)
    rad = st["radiance"]
    pick = (lambda a: a) if channels == 3 else (lambda a: np.ascontiguousarray(a[..., :1]))
    mc, disc = oracle.prepass(rad["n"], pick(rad["mean"]), pick(rad["m2"]), pick(rad["m3"]), spec=spec)
    disc = (disc / np.float32(tighten)).astype(np.float32)
    return rad["n"], mc, disc, pick(rad["film_mean"]), {f: st[f]["mean"] for f in features if f != "radiance"}


def random_stats(W, H, seed, channels=3):
    """Unstructured statistics (tests/test_gpu_parity.py: test_filter_non_finite_corrected_mean): about one tap in four is a member."""
    rng = np.random.default_rng(seed)
    mc = rng.standard_normal((H, W, channels)).astype(np.float32)
    disc = (rng.random((H, W, channels)) * 2).astype(np.float32)
    return mc, disc


def integer_colour(shape, seed):
    return np.random.default_rng(seed).integers(0, 16, shape).astype(np.float32)


def plant_special_pixels(mc, disc, colour, gbs):
    """The pixels of test_filter_special_pixels, test_filter_non_finite_colour and test_filter_non_finite_feature, scaled to
    the image: validity is part of membership.  In place; needs W >= 9, H >= 7."""
    H, W = mc.shape[:2]
    disc[1, 2] = np.inf                          # fewer than two samples: accepts every valid tap
    disc[2, W // 3:W // 3 + 3] = 0.0             # zero variance
    flat_patch(mc, disc)
    mc[3, W // 2] = np.nan                       # a negative sample upstream
    mc[4, 1] = 1e6
    disc[4, 1] = 0.0                             # rejects everyone but itself
    mc[5, W - 2] = np.nan
    disc[5, W - 2] = np.nan                      # not even a member of itself
    mc[0, 0, 0] = np.inf                         # one channel, in the corner a clamped border repeats
    mc[H - 1, 3] = -np.inf
    disc[H - 1, 3] = np.inf
    colour[H - 2, W - 1, 0] = np.nan             # valid statistics, NaN colour: takes no part, keeps its colour
    colour[H // 2, 4] = np.inf
    if gbs:
        gbs[0][H // 2, W - 3, gbs[0].shape[2] - 1] = np.nan
        gbs[-1][H - 1, W - 1, 0] = -np.inf       # the opposite corner


def flat_patch(mc, disc):
    """Four pixels of constant samples: equal means, zero variance.  Among them -- and for each as its own tap -- the gate's
    test is an equality, 0 <= 0: what tells `<=` from `<`.  In place."""
    H, W = mc.shape[:2]
    mc[H - 3, W // 2:W // 2 + 4] = 0.25
    disc[H - 3, W // 2:W // 2 + 4] = 0.0


# ------------------------------------------------------------------ references
def pixel_validity(mc, disc, colour, gbs):
    """Spec v2.1: corrected mean finite, discriminator not NaN, colour finite, every G-buffer value finite -- all channels."""
    H, W = mc.shape[:2]
    v = np.isfinite(mc.reshape(H, W, -1)).all(2) & ~np.isnan(disc.reshape(H, W, -1)).any(2) & np.isfinite(colour.reshape(H, W, -1)).all(2)
    for g in gbs:
        v &= np.isfinite(g.reshape(H, W, -1)).all(2)
    return v


def integer_reference(mc, disc, colour, gbs, radius, clamp=False):
    """The membership probe by brute force, in integers: (count [H, W], acc [H, W, C]) int64 of the default spec -- symmetric
    gate fma(d, d, -(D_p + D_q)) <= 0 in every channel, both pixels valid, taps beyond the image skipped or (clamp) moved
    to the nearest edge pixel and counted once per tap.  The float test is decided exactly: d and D_p + D_q are single
    float operations, d * d is exact in double, and the fma's one rounding cannot change the sign of d^2 - (D_p + D_q)."""
    H, W = mc.shape[:2]
    mc3, dc3 = mc.reshape(H, W, -1), disc.reshape(H, W, -1)
    valid = pixel_validity(mc, disc, colour, gbs)
    col = np.where(valid[..., None], colour.reshape(H, W, -1), 0).astype(np.int64)
    count = np.zeros((H, W), np.int64)
    acc = np.zeros(col.shape, np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                d = (mc3 - mc3[qy, qx]).astype(np.float64)           # float subtraction, then exact
                s = (dc3 + dc3[qy, qx]).astype(np.float64)           # float addition
                member = (d * d <= s).all(2) & valid & valid[qy, qx]
                if not clamp:
                    member &= inside
                count += member
                acc += member[..., None] * col[qy, qx]
    return count, acc


def expected_from_integers(count, acc, colour):
    """What any correct filter returns on the membership probe: float(acc) / float(count), one IEEE division of two exact
    floats; the pixel's own colour where it has no member."""
    assert acc.max() < 2 ** 24
    with np.errstate(invalid="ignore", divide="ignore"):
        q = acc.astype(np.float32) / count.astype(np.float32)[..., None]
    return np.where(count[..., None] > 0, q, colour.reshape(acc.shape)).reshape(colour.shape)


def same_bits(a, b):
    """Per element: the same float, bit for bit (a pixel that keeps a NaN colour: NaN on both sides)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def bilateral_f64(colour, gbs, g_dr, ds, radius, valid=None):
    """The weight probe's reference: the cross-bilateral filter over every valid tap of the clipped window, weights and sums
    in float64 from the float inputs, one (dy, dx) shift at a time.  Returns (out, S): sum w c / sum w and sum w |c| / sum w."""
    H, W = colour.shape[:2]
    r = radius
    col = colour.reshape(H, W, -1).astype(np.float64)
    valid = np.ones((H, W), bool) if valid is None else valid
    pad = lambda a: np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2))
    colp, vp = pad(np.where(valid[..., None], col, 0.0)), pad(valid.astype(np.float64))
    gs = [g.reshape(H, W, -1).astype(np.float64) for g in gbs]
    gps = [pad(np.where(valid[..., None], g, 0.0)) for g in gs]
    sw = np.zeros((H, W))
    acc, mag = np.zeros(col.shape), np.zeros(col.shape)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            win = (slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
            e = np.full((H, W), np.float64(np.float32(ds)) * (dx * dx + dy * dy))
            for g, gp, dr in zip(gs, gps, g_dr):
                e += np.float64(np.float32(dr)) * ((g - gp[win]) ** 2).sum(2)
            w = np.exp(e) * vp[win]
            sw += w
            acc += w[..., None] * colp[win]
            mag += w[..., None] * np.abs(colp[win])
    sw = np.where(valid, sw, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(sw[..., None] > 0, acc / sw[..., None], col)
        S = np.where(sw[..., None] > 0, mag / sw[..., None], np.abs(col))
    return out.reshape(colour.shape), S.reshape(colour.shape)


def scaled_error(out, ref64, S):
    """err(p) = |out - ref64| / S(p) per pixel and channel; where S = 0 every tap's colour is 0 and so must the output be (err 0 or inf)."""
    diff = np.abs(np.asarray(out, np.float64) - ref64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(S > 0, diff / S, np.where(diff > 0, np.inf, 0.0))


# ------------------------------------------------------------------ membership probe: oracle == integers
@pytest.mark.parametrize("W,H,radius,clamp,spp", [(23, 61, 20, False, 4), (9, 37, 6, True, 8)], ids=["23x61-r20-zero-border", "9x37-r6-clamped-border"])
@pytest.mark.parametrize("planted", [False, True], ids=["plain", "special-pixels"])
@pytest.mark.parametrize("tighten", [1, 16], ids=["film", "tight"])
def test_membership_probe_oracle_equals_integer_reference(oracle, W, H, radius, clamp, spp, planted, tighten):
    _, mc, disc, _, feats = noisy_stats(oracle, W, H, spp, seed=3, tighten=tighten)
    gbs = [feats["normal"].copy(), feats["albedo"].copy()]
    colour = integer_colour(mc.shape, seed=H)
    if planted:
        plant_special_pixels(mc, disc, colour, gbs)
    spec = oracle.FilterSpec(border=int(clamp))
    out = oracle.filter_image(mc, disc, colour, gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec)
    count, acc = integer_reference(mc, disc, colour, gbs, radius, clamp=clamp)
    window = (2 * radius + 1) ** 2
    valid = pixel_validity(mc, disc, colour, gbs)
    # the probe is not vacuous: the gate rejects a large share of the taps, and membership varies from pixel to pixel
    assert count[valid].min() >= 1 and count.max() <= window
    taps = oracle.filter_image_f64(mc, np.where(np.isnan(disc), disc, np.inf).astype(np.float32), colour, gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec)[2]
    print("members per pixel %d .. %d, %.0f %% of the valid taps rejected, %.0f %% of the pixels reject some" %
          (count[valid].min(), count.max(), 100 - 100.0 * count.sum() / taps.sum(), 100.0 * (count < taps).mean()))
    assert count.sum() < (0.7 if tighten > 1 else 1.0) * taps.sum()      # (taps: the valid taps of every window, gate open)
    assert len(np.unique(count)) > 20
    assert planted == bool((~valid).any()) and (count[~valid] == 0).all()
    want = expected_from_integers(count, acc, colour)
    bad = np.argwhere(~same_bits(out, want))
    assert not len(bad), "float oracle differs from the integer reference at (y, x, c) %s" % bad[:5].tolist()
    # the double-sum oracle on the same inputs: the same integers, exactly (every weight is exactly 1 in double as well)
    out64, S, sw = oracle.filter_image_f64(mc, disc, colour, gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec)
    assert np.array_equal(sw, count)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.rint(out64 * sw[..., None])[count > 0], acc[count > 0])


def test_membership_probe_random_statistics(oracle):
    """Unstructured statistics (no image structure for a systematic tiling error to hide behind), three clean G-buffer sets."""
    W, H, radius = 31, 17, 5
    mc, disc = random_stats(W, H, seed=3)
    rng = np.random.default_rng(4)
    colour = integer_colour(mc.shape, seed=5)
    for gbs in ([], [rng.random((H, W, 3), dtype=np.float32)], [rng.random((H, W, 3), dtype=np.float32), rng.random((H, W, 1), dtype=np.float32)]):
        out = oracle.filter_image(mc, disc, colour, gbs, [0.0] * len(gbs), PROBE_DS, radius)
        count, acc = integer_reference(mc, disc, colour, gbs, radius)
        assert 0.1 < count.mean() / (2 * radius + 1) ** 2 < 0.5
        assert same_bits(out, expected_from_integers(count, acc, colour)).all()


def test_membership_probe_under_welch(oracle):
    """Welch degrees of freedom (the pair looks its quantile up: no NumPy twin here).  The probe's property itself: with unit
    weights the float oracle's sums are exact -- its output is the one division of the member count and the integer colour
    sum that the double-sum run of the same tap decisions yields -- and with the colour replaced by ones it returns exactly 1."""
    W, H, radius = 40, 19, 7
    spec = oracle.FilterSpec(dof=1)
    n, mc, disc, _, feats = noisy_stats(oracle, W, H, 5, seed=11, spec=spec, tighten=16)
    n = n.copy()
    n[:, 25:] = 2600                              # counts that jump: pairs at very different degrees of freedom
    n[3, 4] = 1
    gbs = [feats["normal"], feats["albedo"]]
    colour = integer_colour(mc.shape, seed=12)
    out = oracle.filter_image(mc, disc, colour, gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec, n=n)
    out64, S, sw = oracle.filter_image_f64(mc, disc, colour, gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec, n=n)
    count = sw.astype(np.int64)
    assert np.array_equal(count, sw) and count.min() >= 1 and count.max() <= (2 * radius + 1) ** 2 and len(np.unique(count)) > 20
    acc = np.rint(out64 * sw[..., None]).astype(np.int64)
    assert np.abs(out64 * sw[..., None] - acc).max() < 1e-9
    assert same_bits(out, expected_from_integers(count, acc, colour)).all()
    ones = oracle.filter_image(mc, disc, np.ones_like(colour), gbs, [0.0, 0.0], PROBE_DS, radius, spec=spec, n=n)
    assert (ones == 1.0).all()
    # ... and the pixel gate of the same statistics decides differently somewhere: the Welch lookup is really in play
    pix = oracle.filter_image_f64(mc, disc, colour, gbs, [0.0, 0.0], PROBE_DS, radius)[2]
    assert (pix != sw).any()


# ------------------------------------------------------------------ weight probe: the references agree, e_or is what the formats allow
def test_weight_probe_references(oracle):
    """disc = +inf: every valid tap is a member.  The double-sum oracle equals the NumPy float64 filter to float64 rounding, and
    the float oracle's scaled error e_or against either is a few float ulps: the window's sequential sum of up to 1 681 terms
    rounds each addition by at most 2^-24 of the running sum -- 1 681 * 2^-24 = 1e-4 in the worst case, and like a random
    walk in practice (its root, 41 * 2^-24 = 2.4e-6, is the size to expect of the largest of a thousand pixels)."""
    W, H, radius = 45, 24, 20
    _, mc, _, colour, feats = noisy_stats(oracle, W, H, 6, seed=8)
    disc = np.full_like(mc, np.inf)
    gbs = [feats["normal"], feats["albedo"]]
    g_dr = [-0.5 / SD_NORMAL ** 2, -0.5 / SD_ALBEDO ** 2]
    ds = -0.5 / FILTER_SD ** 2
    ref64, S = bilateral_f64(colour, gbs, g_dr, ds, radius)
    out64, S64, sw = oracle.filter_image_f64(mc, disc, colour, gbs, g_dr, ds, radius)
    assert np.allclose(out64, ref64, rtol=1e-12, atol=0) and np.allclose(S64, S, rtol=1e-12, atol=0)
    out = oracle.filter_image(mc, disc, colour, gbs, g_dr, ds, radius)
    e_or = scaled_error(out, ref64, S).max()
    print("weight probe, %d x %d, r = %d: e_or = %.3g" % (W, H, radius, e_or))
    assert 0 < e_or < (2 * radius + 1) ** 2 * 2.0 ** -24


def test_f64_oracle_leaves_the_outside_of_the_roi_alone(oracle):
    W, H = 30, 12
    mc, disc = random_stats(W, H, seed=9)
    colour = integer_colour(mc.shape, seed=10)
    roi = (4, 2, 21, 9)
    out64, S, sw = oracle.filter_image_f64(mc, disc, colour, [], [], PROBE_DS, 4, roi=roi)
    full64, _, full_sw = oracle.filter_image_f64(mc, disc, colour, [], [], PROBE_DS, 4)
    inside = np.zeros((H, W), bool)
    inside[2:9, 4:21] = True
    assert not out64[~inside].any() and not sw[~inside].any() and not S[~inside].any()
    assert np.array_equal(out64[inside], full64[inside]) and np.array_equal(sw[inside], full_sw[inside])
