"""Every window-filter kernel per pixel: which taps it takes, and how well it weighs and sums them.

The whole-image relative L2 of tests/test_gpu_parity.py lets a single pixel be wrong by about 0.1 %: one tap dropped or
counted twice at a tile seam, one gate decision that differs from the oracle's, one clamped border tap too many.  Two probes
(pinned on the CPU by tests/test_filter_probes_cpu.py) separate the two sources of error and make each check sharp:

  membership  filter_sd = 1e18, every G-buffer factor 0, integer colours 0 .. 15: every weight is exactly 1, the sums are the
              member count and an integer below 2^24 -- exact in float in any order, through LDS accumulator rows, partial sums
              per part and the combine kernel alike -- and the output is one division.  Every kernel must return the
              oracle's bits at every pixel; a failure names the first pixels and out * count - acc, the taps gained or lost.
  weight      an infinite discriminator (every valid tap a member), the shipped sds, real colours and G-buffers: a plain
              cross-bilateral filter with a float64 NumPy reference; a kernel's scaled error may be four times the float
              oracle's own (hardware exp2: one ulp, plus the rounding of its argument; a summation tree that rounds against
              the oracle's sequential sum in the worst case).

Statistics: a synthetic film's noisy means at 6 spp with its discriminator as it is ("film": the gate rejects about 1 % of the
taps) or divided by 16 ("tight": about half, along the image's structure), and unstructured random ones ("random": three taps in
four).  Every case carries a flat patch (equal means, zero variance: the gate's test is 0 <= 0 there); test_membership_special_pixels
and the r = 7 spec builds carry the pixels that take no part (NaN / infinite mean, discriminator, colour, feature).  The probe found
that the LDS kernels did not read a G-buffer whose factor is 0 and so kept a pixel with a non-finite value in it, unlike the oracle
and the general kernel; such a buffer is now staged with the factor 2^-100 (statmc_filter_common.h: gbuffer_scale), and the planted
features run under the factor 0 like everything else.

Filter variants (statmc_last_filter_variant) covered by the membership probe:
  generic
  lds_r20  lds_rt  lds_rt_asym  lds_rt_centre  lds_rt_joint  lds_rt_asym_joint  lds_r20_f  lds_rt_f  lds_rt_f_asym
  sym_r20  sym_r20_asym  sym_r20_centre  sym_r20_joint  sym_r20_clamp  sym_r20_asym_clamp  sym_r20_joint_clamp  sym_r20_asym_joint_clamp
  sym_rt   sym_rt_asym   sym_rt_centre   sym_rt_joint   sym_rt_clamp   sym_rt_asym_clamp   sym_rt_joint_clamp   sym_rt_asym_joint_clamp
  sym_r20_f  sym_rt_f  sym_r20_f_clamp  sym_rt_f_clamp  sym_r20_f+lds_r20_f  sym_rt_f+lds_rt_f
  sym_r20_g8  sym_rt_g8  sym_r20_f_g8  sym_rt_f_g8  sym_r20_g8_clamp  sym_r20_g8_asym_joint  sym_rt_g8_joint_clamp
  sym_welch  sym_welch_joint  sym_welch_clamp  sym_welch_f  sym_welch_f_clamp
  sym_welch_g8  sym_welch_g8_joint  sym_welch_g8_clamp  sym_welch_f_g8
"""
import functools

import numpy as np
import pytest
import torch

from conftest import FILTER_SD, SD_ALBEDO, SD_NORMAL
from test_filter_probes_cpu import (PROBE_DS, PROBE_SD, bilateral_f64, flat_patch, integer_colour, noisy_stats, plant_special_pixels,
                                    random_stats, same_bits, scaled_error)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.0                        # what an output image holds before the call: pixels outside the ROI keep it
FEATURE_SDS = dict(normal=SD_NORMAL, albedo=SD_ALBEDO, depth=2.0, materialid=0.5)
# (On an MI355X every kernel and mode below returns the oracle's bits: the library divides with the plain `/` of a build without
# fast-math, and v_exp_f32 returns exactly 1 for these exponents.  No kernel needs the weaker round(out * count) == acc.)


def to_dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the shared inputs are read-only arrays)


def pitched(t, pad):
    """The same image with a row pitch: a view of a wider tensor whose extra columns hold NaN (-7 for the counts)."""
    wide = torch.full((t.shape[0], t.shape[1] + pad) + tuple(t.shape[2:]), -7 if t.dtype == torch.int32 else float("nan"), device=DEV).to(t.dtype)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def gap_untouched(view):
    """The columns between the rows of a pitched image (a view made by pitched()) still hold their NaN."""
    h, w = view.shape[:2]
    wide = torch.as_strided(view, (h, view.stride(0) // view.stride(1)) + tuple(view.shape[2:]), view.stride())
    return bool(torch.isnan(wide[:, w:]).all())


def frozen(d):
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


# ------------------------------------------------------------------ inputs and references, computed once and shared
@functools.lru_cache(maxsize=None)
def probe_inputs(W, H, kind="tight", features=("normal", "albedo"), channels=3, planted=False, prepass_spec=(), jump=False, seed=3):
    """One buffer's inputs of the membership probe: n, mc, disc, colour (integers), gbs.  Read-only: shared between tests."""
    from oracle import oracle
    spec = oracle.FilterSpec(**dict(prepass_spec))
    if kind == "random":
        mc, disc = random_stats(W, H, seed=seed, channels=channels)
        rng = np.random.default_rng(seed + 1)
        n = rng.integers(2, 40, (H, W)).astype(np.int32)
        gbs = [rng.random((H, W, 1 if f in ("depth", "materialid") else 3), dtype=np.float32) for f in features]
    else:
        n, mc, disc, _, feats = noisy_stats(oracle, W, H, 6, seed=seed, features=("radiance",) + tuple(features), spec=spec, channels=channels,
                                            tighten=16 if kind == "tight" else 1)
        n = n.copy()
        gbs = [feats[f].copy() for f in features]
    if jump:                           # Welch: counts that jump inside a tile (pairs far apart in the quantile table)
        n[:, W // 2:] = 2600
    colour = integer_colour(mc.shape, seed=seed + 2)
    flat_patch(mc, disc)
    if planted:
        plant_special_pixels(mc, disc, colour, gbs)
    return frozen(dict(n=n, mc=mc, disc=disc, colour=colour, gbs=gbs))


@functools.lru_cache(maxsize=None)
def probe_reference(inputs_key, radius, spec=(), roi=None):
    """The oracle on the membership probe (float, what the kernels must equal bit for bit)."""
    from oracle import oracle
    case = probe_inputs(*inputs_key)
    ref = oracle.filter_image(case["mc"], case["disc"], case["colour"], case["gbs"], [0.0] * len(case["gbs"]), PROBE_DS, radius, roi=roi,
                              spec=oracle.FilterSpec(**dict(spec)), n=case["n"])
    ref.setflags(write=False)
    return ref


def probe_integers(inputs_key, radius, spec=(), roi=None):
    """(count [H, W], acc [H, W, C]) of the same windows, as integers: the double-sum oracle (the float oracle's tap decisions)."""
    from oracle import oracle
    case = probe_inputs(*inputs_key)
    out64, _, sw = oracle.filter_image_f64(case["mc"], case["disc"], case["colour"], case["gbs"], [0.0] * len(case["gbs"]), PROBE_DS, radius,
                                           roi=roi, spec=oracle.FilterSpec(**dict(spec)), n=case["n"])
    with np.errstate(invalid="ignore"):
        return sw.astype(np.int64), np.nan_to_num(np.rint(out64 * sw[..., None])).astype(np.int64)


# ------------------------------------------------------------------ running a kernel
def run_kernel(gpu, buffers, gbs, g_dr, sd, radius, channels=3, force=0, parts=0, spec_kw=None, roi=None, pitch=False, packed_origin=None,
               packed=False):
    """statmc_window_filter on a list of buffers (dicts of n, mc, disc, colour; one for RGB, any number of 1-channel ones) under a
    forced kernel / split / spec, into images prefilled with SENTINEL.  Returns ([out per buffer], variant)."""
    up = (lambda a, pad=3: pitched(to_dev(a), pad)) if pitch else (lambda a, pad=0: to_dev(a))
    sq = (lambda a: a[..., 0]) if channels == 1 else (lambda a: a)           # 1-channel buffers travel as [H, W]
    outs = [up(np.full(sq(b["colour"]).shape, SENTINEL, np.float32), 1) for b in buffers]
    welch = bool(spec_kw and spec_kw.get("dof"))
    if packed:                          # the block + halo image of the multi-GPU path: 15 channels, one buffer
        b = buffers[0]
        img = to_dev(np.concatenate([b["mc"], b["disc"], b["colour"]] + list(gbs), axis=2))
        a, keep = gpu.make_filter_args([], [], [], [], [], [], [], outs, [], g_dr=g_dr, filter_sd=sd, radius=radius, roi=roi, packed=img,
                                       film_origin=packed_origin)
    else:
        a, keep = gpu.make_filter_args([up(b["n"], 2) for b in buffers] if welch else [], [], [], [], [up(sq(b["colour"]), 4) for b in buffers],
                                       [up(sq(b["mc"]), 2) for b in buffers], [up(sq(b["disc"]), 5) for b in buffers], outs,
                                       [up(g, 6) for g in gbs], g_dr=g_dr, filter_sd=sd, radius=radius, roi=roi)
    gpu.set_filter_spec(**(spec_kw or {}))
    gpu.force_filter_variant(force)
    gpu.set_filter_split(parts)
    try:
        gpu.window_filter(a, channels)
        torch.cuda.synchronize()
        variant = gpu.last_filter_variant()
    finally:
        gpu.set_filter_split(0)
        gpu.force_filter_variant(0)
        gpu.set_filter_spec()
    if pitch:                           # nothing stored past the end of a row
        assert all(gap_untouched(o) for o in outs), "wrote between the rows of a pitched output image"
    res = [o.contiguous().cpu().numpy() for o in outs]
    return [r[..., None] if channels == 1 else r for r in res], variant


def tile_of(variant, x, y, roi):
    """Tile and lane coordinates of a pixel, where they are cheap: the pair-symmetric kernel's tiles are 128 x 8 pixels, the
    one-sided kernel's 256 x 8, counted from the ROI's corner; a lane holds four neighbouring pixels."""
    x0, y0 = (roi[0], roi[1]) if roi else (0, 0)
    tw = 128 if variant.startswith("sym") else 256 if variant.startswith("lds") else 32
    return "tile (%d, %d) column %d (pixel %d of its lane) row %d" % ((x - x0) // tw, (y - y0) // 8, (x - x0) % tw, (x - x0) % 4, (y - y0) % 8)


def assert_membership(out, ref, integers, variant, what, roi=None):
    """out == ref bit for bit inside the ROI, SENTINEL outside; on failure the first differing pixels with the taps gained or lost."""
    H, W = out.shape[:2]
    x0, y0, x1, y1 = roi if roi else (0, 0, W, H)
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    assert (out[~inside] == SENTINEL).all(), "%s %s: wrote outside the ROI" % (variant, what)
    ok = same_bits(out, ref) | ~inside[..., None]
    if ok.all():
        return
    count, acc = integers()
    bad = np.argwhere(~ok.all(axis=2))
    lines = []
    for y, x in bad[:8]:
        lines.append("  (x %d, y %d) %s: out %s oracle %s, %d members, out * count - acc = %s" % (
            x, y, tile_of(variant, x, y, roi), out[y, x].tolist(), ref[y, x].tolist(), count[y, x],
            (out[y, x].astype(np.float64) * count[y, x] - acc[y, x]).round(3).tolist()))
    raise AssertionError("%s %s: %d of %d pixels differ from the oracle on the membership probe (a tap or gate error):\n%s" % (
        variant, what, len(bad), inside.sum(), "\n".join(lines)))


def membership_case(gpu, W, H, radius, variant, *, kind="tight", features=("normal", "albedo"), channels=3, planted=False, spec_kw=None, jump=False,
                    force=0, parts=0, roi=None, pitch=False, packed=False, packed_origin=None, seed=3):
    """One membership-probe run of one RGB buffer (or one 1-channel buffer) and its assertions."""
    spec_kw = spec_kw or {}
    spec = tuple(sorted(spec_kw.items()))
    key = (W, H, kind, tuple(features), channels, planted, tuple(sorted((k, v) for k, v in spec_kw.items() if k in ("sides", "small_n", "dof"))), jump, seed)
    case = probe_inputs(*key)
    ref = probe_reference(key, radius, spec, roi)
    outs, v = run_kernel(gpu, [case], case["gbs"], [0.0] * len(case["gbs"]), PROBE_SD, radius, channels=channels, force=force, parts=parts, spec_kw=spec_kw,
                         roi=roi, pitch=pitch, packed=packed, packed_origin=packed_origin)
    assert v == variant, v
    what = "%d x %d r = %d %s%s" % (W, H, radius, kind, " parts %d" % parts if parts else "")
    assert_membership(outs[0], ref, lambda: probe_integers(key, radius, spec, roi), v, what, roi=roi)


# ------------------------------------------------------------------ 1. membership probe
@pytest.mark.parametrize("kind", ["tight", "film", "random"])
@pytest.mark.parametrize("force,variant", [(0, "sym_r20"), (3, "lds_r20"), (2, "lds_rt"), (1, "generic")])
def test_membership_r20_every_kernel(gpu, kind, force, variant):
    """300 x 41 at the shipped radius: two tile columns of the one-sided kernel, three of the pair-symmetric one, a ragged right edge."""
    membership_case(gpu, 300, 41, 20, variant, kind=kind, force=force)


@pytest.mark.parametrize("parts", [1, 2, 3, 7, 41, 64])
@pytest.mark.parametrize("force,variant", [(0, "sym_r20"), (3, "lds_r20")])
def test_membership_window_sweep_parts(gpu, parts, force, variant):
    """The window rows split over `parts` workgroups per tile, partial sums combined by a second kernel: every split, both LDS kernels."""
    membership_case(gpu, 300, 41, 20, variant, force=force, parts=parts)


@pytest.mark.parametrize("W,H,radius", [(64, 50, 1), (259, 9, 3), (37, 21, 6), (420, 70, 6), (132, 30, 7), (300, 41, 13), (300, 41, 16), (300, 41, 19)])
@pytest.mark.parametrize("force,variant", [(0, "sym_rt"), (2, "lds_rt"), (1, "generic")])
def test_membership_runtime_radius(gpu, W, H, radius, force, variant):
    """The shapes of test_filter_matches_oracle: images smaller than a tile, four tile columns, widths 4k + 3, radii that are
    no multiple of 4, read groups skipped (r = 16) or cut by the table (r = 19)."""
    membership_case(gpu, W, H, radius, variant, force=force)


def test_membership_beyond_the_lds_range(gpu):
    membership_case(gpu, 45, 33, 24, "generic")
    membership_case(gpu, 45, 33, 24, "generic", kind="random")


@pytest.mark.parametrize("force", [0, 3, 2, 1])
@pytest.mark.parametrize("W,H,radius", [(270, 26, 20), (61, 23, 5)])
def test_membership_special_pixels(gpu, W, H, radius, force):
    """Validity is part of membership: NaN / infinite corrected means, discriminators, colours and G-buffer values planted, on every
    kernel -- the G-buffers under the factor 0 as everywhere in the probe: a buffer that moves no weight still excludes a pixel."""
    variant = {0: "sym_r20" if radius == 20 else "sym_rt", 3: "lds_r20" if radius == 20 else "lds_rt", 2: "lds_rt", 1: "generic"}[force]
    membership_case(gpu, W, H, radius, variant, planted=True, force=force)


@pytest.mark.parametrize("features,channels,spec_kw,force,radius,variant", [
    (("normal", "albedo", "depth", "materialid"), 3, {}, 0, 20, "sym_r20_g8"), (("depth", "normal"), 3, {}, 0, 6, "sym_rt_g8"),
    (("depth", "normal"), 3, {}, 2, 6, "lds_rt"), (("albedo", "materialid"), 1, {}, 0, 20, "sym_r20_f_g8"),
    (("normal", "albedo", "depth"), 3, dict(dof=1), 0, 20, "sym_welch_g8"), (("normal", "albedo"), 3, dict(dof=1, border=1), 0, 7, "sym_welch_clamp"),
    (("normal",), 3, {}, 0, 20, "sym_r20"), (("normal",), 1, {}, 3, 20, "lds_r20_f")])
def test_membership_special_pixels_feature_layouts(gpu, features, channels, spec_kw, force, radius, variant):
    """The same planted pixels where the features are staged otherwise: eight planes, the one-sided kernel's six slots, one buffer
    only (its neighbour slot absent), float buffers, the Welch builds."""
    membership_case(gpu, 270, 26, radius, variant, features=features, channels=channels, spec_kw=spec_kw, jump=bool(spec_kw.get("dof")), planted=True, force=force)


SPECS = [dict(gate=1), dict(border=1), dict(gate=1, border=1), dict(channel_rule=1), dict(dof=1), dict(sides=1, small_n=1), dict(gate=2),
         dict(gate=1, channel_rule=1, border=1), dict(dof=1, channel_rule=1), dict(dof=1, border=1), dict(channel_rule=1, border=1)]


def sym_name(spec_kw, radius, channels=3, g8=False):
    gate, joint, border = spec_kw.get("gate", 0), spec_kw.get("channel_rule", 0) and channels == 3, spec_kw.get("border", 0)
    f, g = "_f" if channels == 1 else "", "_g8" if g8 else ""
    if spec_kw.get("dof"):
        return "sym_welch" + f + g + ("_joint" if joint else "") + ("_clamp" if border else "")
    return ("sym_r20" if radius == 20 else "sym_rt") + f + g + ("", "_asym", "_centre")[gate] + ("_joint" if joint else "") + ("_clamp" if border else "")


@pytest.mark.parametrize("W,H,radius", [(280, 26, 20), (90, 30, 7)], ids=["r20", "r7"])
@pytest.mark.parametrize("spec_kw", SPECS, ids=["".join("%s%d" % (k[0], v) for k, v in s.items()) for s in SPECS])
def test_membership_spec_builds(gpu, spec_kw, W, H, radius):
    """The gate forms, the joint channel rule, the clamped border (its taps beyond the image come from a second kernel), Welch
    degrees of freedom (counts that jump inside a tile: work items computed again from the whole table) and the pre-pass
    choices, at the shipped radius and a small one; the one-sided kernel's build of the spec beside the pair-symmetric one."""
    welch = bool(spec_kw.get("dof"))
    membership_case(gpu, W, H, radius, sym_name(spec_kw, radius), spec_kw=spec_kw, jump=welch, planted=radius == 7)
    if not welch:
        gate, joint = spec_kw.get("gate", 0), spec_kw.get("channel_rule", 0)
        membership_case(gpu, W, H, radius, "lds_rt" + ("", "_asym", "_centre")[gate] + ("_joint" if joint else ""), spec_kw=spec_kw, force=2, planted=radius == 7)


def float_buffers(W, H, n_buffers, kind, features=("normal", "albedo"), prepass_spec=(), jump=False):
    """n 1-channel buffers with their own statistics and colours over the G-buffers of the first."""
    keys = [(W, H, kind, tuple(features), 1, False, prepass_spec, jump and b % 2 == 1, 3 + b) for b in range(n_buffers)]
    return keys, [probe_inputs(*k) for k in keys]


@pytest.mark.parametrize("n_buffers,split,radius,force,spec_kw,variant", [
    (1, 0, 20, 0, {}, "sym_r20_f"), (4, 1, 20, 0, {}, "sym_r20_f"), (2, 0, 7, 0, {}, "sym_rt_f"),
    (3, 1, 20, 0, {}, "lds_r20_f"), (5, 1, 20, 0, {}, "sym_r20_f+lds_r20_f"), (7, 1, 20, 0, {}, "sym_r20_f+lds_r20_f"),   # odd counts end on the one-sided kernel
    (5, 3, 20, 0, {}, "sym_r20_f"),                                    # ... unless the sweep is split: the last launch carries one buffer
    (3, 0, 7, 2, {}, "lds_rt_f"), (2, 0, 20, 3, {}, "lds_r20_f"), (4, 0, 7, 1, {}, "generic"),
    (3, 0, 20, 0, dict(dof=1), "sym_welch_f"), (2, 0, 6, 0, dict(dof=1, border=1), "sym_welch_f_clamp"),
    (2, 0, 20, 0, dict(border=1), "sym_r20_f_clamp"), (2, 0, 7, 0, dict(gate=1), "lds_rt_f_asym"),
    (5, 1, 7, 0, {}, "sym_rt_f+lds_rt_f"), (3, 1, 7, 0, {}, "lds_rt_f"), (2, 0, 7, 0, dict(border=1), "sym_rt_f_clamp")])
def test_membership_float_buffers(gpu, oracle, n_buffers, split, radius, force, spec_kw, variant):
    """filter<float>: 1-channel buffers with their own statistics share a launch's range weight, two per launch on the pair-symmetric
    kernel, three on the one-sided one; every buffer keeps its own windows.  Welch: every buffer its own counts."""
    W, H = 300, 31
    welch = bool(spec_kw.get("dof"))
    keys, bufs = float_buffers(W, H, n_buffers, "tight", prepass_spec=(("dof", 1),) if welch else (), jump=welch)
    gbs = bufs[0]["gbs"]
    outs, v = run_kernel(gpu, bufs, gbs, [0.0, 0.0], PROBE_SD, radius, channels=1, force=force, parts=split, spec_kw=spec_kw)
    assert v == variant, v
    spec = oracle.FilterSpec(**spec_kw)
    for b, (case, out) in enumerate(zip(bufs, outs)):
        args = (case["mc"], case["disc"], case["colour"], gbs, [0.0, 0.0], PROBE_DS, radius)
        ref = oracle.filter_image(*args, spec=spec, n=case["n"])

        def integers():
            out64, _, sw = oracle.filter_image_f64(*args, spec=spec, n=case["n"])
            return sw.astype(np.int64), np.rint(out64 * sw[..., None]).astype(np.int64)
        assert_membership(out, ref, integers, v, "buffer %d of %d" % (b, n_buffers))


@pytest.mark.parametrize("channels,features,spec_kw,W,radius", [
    (3, ("normal", "albedo", "depth", "materialid"), {}, 300, 20),
    (3, ("depth", "albedo", "materialid", "normal"), {}, 301, 20),               # any order; width 4k + 1: register staging
    (3, ("albedo", "normal", "depth"), dict(border=1), 300, 20),
    (3, ("normal", "albedo", "depth", "materialid"), dict(gate=1, channel_rule=1), 300, 20),
    (3, ("materialid", "depth", "normal", "albedo"), {}, 300, 6),
    (3, ("normal", "albedo", "depth", "materialid"), dict(channel_rule=1, border=1), 301, 7),
    (1, ("normal", "albedo", "depth", "materialid"), {}, 300, 20),
    (1, ("normal", "depth"), {}, 300, 3),
    (3, ("normal", "albedo", "depth"), dict(dof=1), 280, 20),                      # Welch x 1-channel G-buffers: n - 1 in a plane of its own
    (3, ("depth", "normal", "materialid", "albedo"), dict(dof=1, channel_rule=1), 280, 20),
    (3, ("materialid",), dict(dof=1, border=1), 280, 6),
    (1, ("normal", "albedo", "depth", "materialid"), dict(dof=1), 280, 20),
], ids=["nadm", "danm-unaligned", "three-clamp", "asym+joint", "r6", "r7-joint+clamp-unaligned", "float", "float-r3", "welch", "welch-joint", "welch-r6-clamp-one-plane",
        "welch-float"])
def test_membership_eight_feature_planes(gpu, channels, features, spec_kw, W, radius):
    """Depth and material id among the G-buffers: the pair-symmetric kernel's eight-plane builds, Welch ones included."""
    welch = bool(spec_kw.get("dof"))
    membership_case(gpu, W, 44 if not welch else 30, radius, sym_name(spec_kw, radius, channels, g8=True), features=features, channels=channels,
                    spec_kw=spec_kw, jump=welch)


@pytest.mark.parametrize("force,variant", [(0, "sym_r20"), (3, "lds_r20"), (1, "generic")])
def test_membership_roi(gpu, force, variant):
    """Outputs only inside the ROI (a ROI that starts inside a tile and a lane), window clipped to the image, the rest untouched."""
    membership_case(gpu, 330, 60, 20, variant, force=force, roi=(21, 19, 310, 41))


@pytest.mark.parametrize("radius,roi,variant", [(20, None, "sym_r20"), (3, None, "sym_rt"), (20, (8, 4, 60, 21), "sym_r20")])
def test_membership_pitched_images(gpu, radius, roi, variant):
    """Every image with its own row pitch, NaN between the rows."""
    membership_case(gpu, 68, 25, radius, variant, roi=roi, pitch=True)
    membership_case(gpu, 68, 25, radius, "generic", roi=roi, pitch=True, force=1)


@pytest.mark.parametrize("radius,origin,variant", [(20, None, "sym_r20"), (6, (128, 40), "sym_rt"), (6, (122, 34), "sym_rt"), (13, (256, 8), "sym_rt")])
def test_membership_packed_inputs(gpu, radius, origin, variant):
    """The block + halo image of the multi-GPU path (15 channels, the ROI = the block, tiles laid out from the block's film
    coordinates), at the three block origins of test_packed_inputs_at_small_radii."""
    W, H, m = 300, 56, radius
    membership_case(gpu, W, H, radius, variant, roi=(m, m, W - m, H - m), packed=True, packed_origin=origin)


def test_membership_packed_inputs_clamped(gpu):
    membership_case(gpu, 300, 56, 20, "sym_r20_clamp", roi=(20, 0, 280, 56), packed=True, spec_kw=dict(border=1))


# ------------------------------------------------------------------ 2. weight probe
@functools.lru_cache(maxsize=None)
def weight_case(W, H, radius, features=("normal", "albedo")):
    """Real colours and G-buffers, every valid tap a member; the float64 NumPy reference, its scale S, the float oracle and e_or."""
    from oracle import oracle
    n, mc, _, colour, feats = noisy_stats(oracle, W, H, 6, seed=5, features=("radiance",) + tuple(features))
    disc = np.full_like(mc, np.inf)
    gbs = [feats[f] for f in features]
    g_dr = [-0.5 / FEATURE_SDS[f] ** 2 for f in features]
    sd = FILTER_SD
    ref64, S = bilateral_f64(colour, gbs, g_dr, -0.5 / sd ** 2, radius)
    orc = oracle.filter_image(mc, disc, colour, gbs, g_dr, -0.5 / sd ** 2, radius)
    e_or = float(scaled_error(orc, ref64, S).max())
    return frozen(dict(n=n, mc=mc, disc=disc, colour=colour, gbs=gbs)), g_dr, sd, ref64, S, e_or


@pytest.mark.parametrize("W,H,radius,features,channels,force,variant", [
    (300, 41, 20, ("normal", "albedo"), 3, 0, "sym_r20"), (300, 41, 20, ("normal", "albedo"), 3, 3, "lds_r20"),
    (300, 41, 20, ("normal", "albedo"), 3, 2, "lds_rt"), (300, 41, 20, ("normal", "albedo"), 3, 1, "generic"),
    (132, 30, 6, ("normal", "albedo"), 3, 0, "sym_rt"), (300, 41, 19, ("normal", "albedo"), 3, 0, "sym_rt"),
    (300, 41, 20, ("normal", "albedo"), 1, 0, "sym_r20_f"), (300, 41, 20, ("normal", "albedo"), 1, 3, "lds_r20_f"),
    (300, 41, 20, ("normal", "albedo", "depth", "materialid"), 3, 0, "sym_r20_g8"), (132, 30, 6, ("normal", "albedo", "depth", "materialid"), 3, 0, "sym_rt_g8")])
def test_weight_probe(gpu, W, H, radius, features, channels, force, variant):
    """max_p |out - ref64| / S(p) <= 4 e_or, e_or the same measure of the float oracle (computed here, per case).
    Measured on an MI355X (gfx950) -- e_or, then each kernel's maximum (the pair-symmetric and one-sided kernels sum in trees and
    land at a third of the oracle's error where the window is large; the general kernel sums in the oracle's order; at r = 6 the
    169 taps leave the oracle's sequential sum as good as a tree and the kernels' exp2 shows):
      300 x 41 r = 20       e_or 3.15e-6   sym_r20 9.27e-7   lds_r20 9.51e-7   lds_rt 9.51e-7   generic 3.08e-6   sym_r20_f 9.27e-7   lds_r20_f 9.51e-7
      132 x 30 r = 6        e_or 9.98e-7   sym_rt 1.21e-6 (1.21 e_or)
      300 x 41 r = 19       e_or 3.10e-6   sym_rt 9.23e-7
      300 x 41 r = 20, g8   e_or 3.25e-6   sym_r20_g8 8.97e-7
      132 x 30 r = 6, g8    e_or 1.14e-6   sym_rt_g8 1.03e-6 (0.90 e_or)"""
    case, g_dr, sd, ref64, S, e_or = weight_case(W, H, radius, tuple(features))
    if channels == 3:
        bufs = [case]
    else:                               # filter<float>: the three channels as three 1-channel buffers
        bufs = [dict(n=case["n"], **{k: np.ascontiguousarray(case[k][..., c:c + 1]) for k in ("mc", "disc", "colour")}) for c in range(3)]
    outs, v = run_kernel(gpu, bufs, case["gbs"], g_dr, sd, radius, channels=channels, force=force)
    assert v == variant, v
    out = outs[0] if channels == 3 else np.concatenate(outs, axis=2)
    err = scaled_error(out, ref64, S)
    worst = np.unravel_index(np.argmax(err), err.shape)
    print("weight probe %d x %d r = %d %s: e_or = %.3g, %s max err = %.3g (%.2f e_or) at (y, x, c) %s" % (
        W, H, radius, "g8" if len(features) > 2 else "", e_or, v, err.max(), err.max() / e_or, worst))
    assert 0 < e_or < (2 * radius + 1) ** 2 * 2.0 ** -24          # (the worst case of a sequential float sum; a random walk stays near its root)
    assert err.max() <= 4 * e_or, "%s: pixel (x %d, y %d) channel %d is off by %.3g S = %.2f e_or (a weight or sum error: every tap is a member)" % (
        v, worst[1], worst[0], worst[2], err.max(), err.max() / e_or)

