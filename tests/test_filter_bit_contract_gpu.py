"""The window filter's bit contract at the C ABI: the same pinned split and the same film-anchored tile grid leave the same bits
in a pixel, whether it is filtered as part of the whole film, of a region of interest or of a block + halo image, in every
image layout include/statmc.h words (separate images; 15 / 16 / 17 / 18 channels).

Every run goes through statmc_window_filter alone, into an image prefilled with a sentinel that must survive outside the ROI.
The whole-film reference of a (G-buffer set, spec, radius, split) comes from separate images, once.  Block + halo images are cut
out of the film and packed by NumPy (tests/test_filter_layouts_cpu.py: the helpers, pinned there on the CPU oracle), not by the
product's drivers -- PeerFilm, BlockPipeline and FilmShards give a G-buffer set exactly one layout; a C host may choose another.
The real colours and the shipped feature sds make the sums sensitive to their order: test_split_regroups_the_sums is the control
(split 1 and split 3 differ in most pixels), which the exact membership probe of tests/test_filter_per_pixel_gpu.py cannot be.

What the matrix found (the commit before this file, one MI355X; every other cell returned the whole film's bits):
  - a 17-channel image that holds exactly two RGB G-buffers and no 1-channel one ran the eight-plane build, which shares the
    window after read group 6, where the whole film with the same G-buffers runs the G7 build (after group 7).  At r = 20 and
    split 2, over the five blocks (17 187 pixels), the 17-channel block differed from the whole film in 14 267 pixels under
    the default spec, in 15 167 under the joint channel rule and in 13 606 under the clamped border; in none under gate = 1,
    gate = 2, gate + joint + clamp, or at r = 7 (no G7 build there), and the 15-channel image in none anywhere.  Such an image
    is now refused under STATMC_DOF_PIXEL, by the window filter and by the pack entries, with a message that names the
    15-channel layout: test_two_rgb_17_channel_image_is_refused.  The 18-channel two-RGB image under Welch has no G7 build on
    either side and stays in the matrix.

The one-sided kernel (window_filter_lds; forced, and by default for float buffers under a non-symmetric gate, more than two
1-channel G-buffers and the last three of an odd number of float buffers with the sweep in one part) lays its tiles from the
ROI's corner.  Which alignment do its sums depend on -- 4, 2 or the tile?  Read from the kernel: NONE.  A lane's staged columns
start at x0 - rp with x0 = roi_x0 + a multiple of 4 and rp a multiple of 4; tap i of a read group goes to the accumulator half
i mod 2 (load_half<H>: taps 2H, 2H + 1; LaneState::acc as v2f), and for pixel k of the lane i = dx + k + rp - 4j.  So a tap's
half is (dx + x - roi_x0) mod 2, and within a half the taps are added in ascending (dy, dx) whatever the tile, the lane or
the pixel's place in the lane (the parts split the window rows by their offset in the window).  The parity of x - roi_x0
decides only WHICH of the two halves holds the taps with dx even, and the epilogue adds the halves: acc.x + acc.y is
acc.y + acc.x.  Measured: the blocks with origin columns 0, 148, 122 (2 mod 4), 129 and 37 (odd) all return the whole film's
bits, on the forced r = 20 and runtime-radius builds, from separate images and from the 15-channel image, and on the float
paths.  So include/statmc.h keeps "whatever the region of interest" for this kernel and says why; what it now adds is that the
promise compares a kernel with itself (the float tail: the same buffer count on both sides).

Wall time of this file on one MI355X: 3.6 s for 105 tests (the slowest 0.2 s, plus 0.2 s to set the library up);
tests/test_filter_per_pixel_gpu.py at the commit before this file, in the same session: 6.1 s for 137 tests."""
import functools

import numpy as np
import pytest
import torch

from test_filter_layouts_cpu import (BAND, BLOCKS, CELLS, FEATURE_CHANNELS, FILM_H, FILM_W, G_SETS, cell_id, cut, film_case, filter_sd, g_dr,
                                     local_rect, pack_numpy, roi_in, split_slots)
from test_filter_per_pixel_gpu import gap_untouched, pitched
from test_filter_probes_cpu import same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.0
WHOLE = (0, 0, FILM_W, FILM_H)
# the one-sided kernel lays its tiles from the ROI's corner: besides the blocks of the matrix (corner columns 0, 148, 122 = 2 mod 4,
# 129), a large block with an odd corner column and an odd corner row
ONE_SIDED_BLOCKS = BLOCKS + [(37, 9, 170, 51)]


def to_dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def layouts_of(features, welch):
    """The layouts a G-buffer set is run in: separate images and every packed image the header allows for it."""
    two_rgb = tuple(FEATURE_CHANNELS[f] for f in features) == (3, 3)
    if welch:
        return ["separate"] + ([16] if two_rgb else []) + [18]
    return ["separate"] + ([15] if two_rgb else []) + [17]


def refused(features, layout, welch):
    """The layout the header refuses: exactly two RGB G-buffers and no 1-channel one in 17 channels (STATMC_DOF_PIXEL)."""
    return layout == 17 and not welch and tuple(FEATURE_CHANNELS[f] for f in features) == (3, 3)


def with_g8(variant):
    """The variant string with the eight-plane suffix a 17- / 18-channel image implies."""
    if "_g8" in variant:
        return variant
    for build in ("sym_r20", "sym_rt", "sym_welch"):
        if variant.startswith(build):
            return build + "_g8" + variant[len(build):]
    return variant


# ------------------------------------------------------------------ one call
def run_filter(gpu, case, features, radius, spec_kw, split, layout="separate", L=WHOLE, roi=None, pitch=False, force=0):
    """statmc_window_filter on the film (L = WHOLE) or on its cut-out L (film origin = L's corner) in one layout, under a pinned
    split.  Returns (out [h, w, 3] with SENTINEL outside the ROI, variant)."""
    welch = bool(spec_kw.get("dof"))
    n, mc, disc, colour = (cut(case[k], L) for k in ("n", "mc", "disc", "colour"))
    gbs = [cut(case[f], L) for f in features]
    up = (lambda a, pad: pitched(to_dev(a), pad)) if pitch else (lambda a, pad: to_dev(a))
    out = up(np.full(mc.shape, SENTINEL, np.float32), 1)
    common = dict(g_dr=g_dr(features), filter_sd=filter_sd(radius), radius=radius, roi=roi, film_origin=L[:2])
    if layout == "separate":
        a, keep = gpu.make_filter_args([up(n, 2)] if welch else [], [], [], [], [up(colour, 4)], [up(mc, 2)], [up(disc, 5)], [out],
                                       [up(g, 6) for g in gbs], **common)
    else:
        rgb, sc = split_slots(features, gbs)
        img = to_dev(pack_numpy(mc, disc, colour, rgb, sc, n, layout))
        a, keep = gpu.make_filter_args([], [], [], [], [], [], [], [out], [], packed=img, packed_g_channels=[FEATURE_CHANNELS[f] for f in features], **common)
    gpu.set_filter_spec(**spec_kw)
    gpu.force_filter_variant(force)
    gpu.set_filter_split(split)
    try:
        gpu.window_filter(a, 3)
        torch.cuda.synchronize()
        variant = gpu.last_filter_variant()
    finally:
        gpu.set_filter_split(0)
        gpu.force_filter_variant(0)
        gpu.set_filter_spec()
    if pitch:
        assert gap_untouched(out), "wrote between the rows of a pitched output image"
    return out.contiguous().cpu().numpy(), variant


_whole = {}


def whole_film(gpu, features, radius, spec_kw, split, force=0):
    """The whole film from separate images: once per (set, spec, radius, split)."""
    key = (features, radius, tuple(spec_kw.items()), split, force)
    if key not in _whole:
        out, v = run_filter(gpu, film_case(bool(spec_kw.get("dof"))), features, radius, spec_kw, split, force=force)
        assert not (out == SENTINEL).all(axis=2).any(), "%s: pixels of the whole film not written" % v
        out.setflags(write=False)
        _whole[key] = (out, v)
    return _whole[key]


def differing(out, B, L, ref):
    """Pixels of block B (film coordinates) whose bits differ between `out` (the local image L) and the whole film: film (y, x)."""
    x0, y0, x1, y1 = roi_in(B, L)
    inside = np.zeros(out.shape[:2], bool)
    inside[y0:y1, x0:x1] = True
    assert (out[~inside] == SENTINEL).all(), "wrote outside the ROI"
    ok = same_bits(out[y0:y1, x0:x1], ref[B[1]:B[3], B[0]:B[2]]).all(axis=2)
    return np.argwhere(~ok) + np.array([B[1], B[0]]), ok.size


def assert_same_bits(out, v, B, L, ref, v_ref, what, g8=False):
    """Block B of `out` (local image L, variant v) == the whole film's (ref, v_ref) bit for bit, run by the same variant up to the
    _g8 suffix of a 17- / 18-channel image; a failure names the cell, the first pixels with their place in tile, row and lane, both variants."""
    bad, total = differing(out, B, L, ref)
    if len(bad):
        loc = roi_in(B, L)
        lines = ["  film (x %d, y %d): x mod 128 = %d, y mod 8 = %d, x mod 4 = %d: block %s, whole film %s" % (
            x, y, x % 128, y % 8, x % 4, out[y - B[1] + loc[1], x - B[0] + loc[0]].tolist(), ref[y, x].tolist()) for y, x in bad[:6]]
        raise AssertionError("%s: %d of %d pixels of block %s differ from the whole film (block: %s, whole film: %s); columns mod 4 of all of them %s:\n%s" % (
            what, len(bad), total, B, v, v_ref, np.bincount(bad[:, 1] % 4, minlength=4).tolist(), "\n".join(lines)))
    assert v == (with_g8(v_ref) if g8 else v_ref), "%s: ran %s, the whole film %s" % (what, v, v_ref)


def check_cell(gpu, features, radius, spec_kw, split, blocks=BLOCKS, layouts=None, force=0, pitched_block=BLOCKS[2]):
    """Every block x layout of one (set, spec, radius, split) against the whole film; the band also as a ROI of the whole film; one
    block per layout from pitched tensors."""
    welch = bool(spec_kw.get("dof"))
    case = film_case(welch)
    ref, v_ref = whole_film(gpu, features, radius, spec_kw, split, force)
    for layout in layouts or layouts_of(features, welch):
        if refused(features, layout, welch):
            continue                    # (test_two_rgb_17_channel_image_is_refused)
        g8 = layout in (17, 18)
        runs = [(B, local_rect(B, radius, FILM_W, FILM_H), False) for B in blocks]
        if BAND in blocks:
            runs.append((BAND, WHOLE, False))
        if pitched_block in blocks:
            runs.append((pitched_block, local_rect(pitched_block, radius, FILM_W, FILM_H), True))
        for B, L, pitch in runs:
            what = "%s r = %d %s split %d, layout %s%s%s" % ("+".join(features), radius, spec_kw or "default", split, layout,
                                                            ", ROI of the whole film" if L == WHOLE else ", local image %s" % (L,), ", pitched" if pitch else "")
            out, v = run_filter(gpu, case, features, radius, spec_kw, split, layout=layout, L=L, roi=roi_in(B, L), pitch=pitch, force=force)
            assert_same_bits(out, v, B, L, ref, v_ref, what, g8=g8)


# ------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("features", G_SETS, ids=["+".join(f) for f in G_SETS])
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_layouts_same_bits(gpu, cell, features):
    """Split 2: every block, in every layout of the set, equals the whole film bit for bit; the variant is the whole film's up to
    the _g8 suffix of the 17- / 18-channel images."""
    radius, spec_kw = cell
    check_cell(gpu, features, radius, spec_kw, 2)


@pytest.mark.parametrize("features", G_SETS, ids=["+".join(f) for f in G_SETS])
@pytest.mark.parametrize("radius", [20, 7])
@pytest.mark.parametrize("split", [1, 3])
def test_layouts_same_bits_other_splits(gpu, split, radius, features):
    check_cell(gpu, features, radius, {}, split)


@pytest.mark.parametrize("radius", [20, 7])
def test_split_regroups_the_sums(gpu, radius):
    """The control: the data can see a regrouping.  The whole film under split 1 and under split 3 differ in a pixel's bits."""
    a, va = whole_film(gpu, G_SETS[0], radius, {}, 1)
    b, vb = whole_film(gpu, G_SETS[0], radius, {}, 3)
    differ = (~same_bits(a, b).all(axis=2)).sum()
    print("r = %d: %d of %d pixels differ between split 1 and split 3 (%s)" % (radius, differ, a.shape[0] * a.shape[1], va))
    assert va == vb and differ >= 1


@pytest.mark.parametrize("spec_kw", [dict(), dict(channel_rule=1), dict(border=1), dict(gate=1)], ids=["default", "joint", "clamp", "asym"])
@pytest.mark.parametrize("radius", [20, 7])
def test_two_rgb_17_channel_image_is_refused(gpu, radius, spec_kw):
    """Exactly two RGB G-buffers and no 1-channel one in a 17-channel image under STATMC_DOF_PIXEL: the eight-plane build would share the
    window after read group 6 where the whole film (and its 15-channel image) shares it after group 7.  Refused; the message
    names the layout to use."""
    case, B = film_case(False), BLOCKS[1]
    L = local_rect(B, radius, FILM_W, FILM_H)
    with pytest.raises(gpu.StatmcError) as e:
        run_filter(gpu, case, G_SETS[0], radius, spec_kw, 2, layout=17, L=L, roi=roi_in(B, L))
    assert e.value.code == gpu.ERR_UNSUPPORTED and "15-channel" in str(e.value), str(e.value)
    # ... and nothing is packed that way either
    blk = {k: to_dev(cut(case[k], B)) for k in ("n", "mc", "disc", "colour", "normal", "albedo")}
    img = torch.full((B[3] - B[1], B[2] - B[0], 17), SENTINEL, device=DEV)
    z = torch.zeros_like(blk["mc"])
    a, keep = gpu.make_filter_args([blk["n"]], [z], [z], [z], [blk["colour"]], [blk["mc"]], [blk["disc"]], [torch.zeros_like(z)], [blk["normal"], blk["albedo"]],
                                   g_dr=g_dr(G_SETS[0]), radius=radius)
    for call in (lambda: gpu.pack_filter_inputs(a, img, 0, 0), lambda: gpu.prepass_pack(a, img, 0, 0), lambda: gpu.prepass_pack(a, img, 0, 0, rows=[(0, 4)])):
        with pytest.raises(gpu.StatmcError) as e:
            call()
        assert e.value.code == gpu.ERR_UNSUPPORTED and "15-channel" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((img == SENTINEL).all())


# ------------------------------------------------------------------ 2. the other kernels
@pytest.mark.parametrize("features,radius", [(("normal", "albedo"), 24), (("normal", "albedo", "tint"), 7)], ids=["r24", "three-rgb-r7"])
def test_general_kernel(gpu, features, radius):
    """Beyond the LDS kernels' range: one lane per pixel, the oracle's order, whatever the image around the window."""
    check_cell(gpu, features, radius, {}, 2, layouts=["separate"])
    assert whole_film(gpu, features, radius, {}, 2)[1] == "generic"


@pytest.mark.parametrize("layout", ["separate", 15])
@pytest.mark.parametrize("force,variant", [(3, "lds_r20"), (2, "lds_rt")])
def test_forced_one_sided_kernel(gpu, force, variant, layout):
    """The one-sided kernel lays its tiles from the ROI's corner, and its sums do not depend on where that is (module docstring):
    what include/statmc.h promises holds for it at every block -- corner columns that are multiples of 4, 2 mod 4 and odd."""
    for split in (2, 1):
        check_cell(gpu, G_SETS[0], 20, {}, split, blocks=ONE_SIDED_BLOCKS, layouts=[layout], force=force)
        assert whole_film(gpu, G_SETS[0], 20, {}, split, force)[1] == variant


@functools.lru_cache(maxsize=None)
def float_buffers(n_buffers):
    """n 1-channel buffers with their own statistics: the channels of the film and of a second film (another seed)."""
    cases = [film_case(False), film_case(False, seed=4)]
    return [{k: np.ascontiguousarray(cases[b // 3][k][..., b % 3]) for k in ("mc", "disc", "colour")} for b in range(n_buffers)]


def run_float(gpu, n_buffers, radius, spec_kw, split, L=WHOLE, roi=None):
    """filter<float> on n buffers over normal + albedo.  Returns ([out per buffer], variant of the last launch)."""
    bufs, features = float_buffers(n_buffers), G_SETS[0]
    gbs = [to_dev(cut(film_case(False)[f], L)) for f in features]
    outs = [to_dev(np.full(cut(b["mc"], L).shape, SENTINEL, np.float32)) for b in bufs]
    a, keep = gpu.make_filter_args([], [], [], [], [to_dev(cut(b["colour"], L)) for b in bufs], [to_dev(cut(b["mc"], L)) for b in bufs],
                                   [to_dev(cut(b["disc"], L)) for b in bufs], outs, gbs, g_dr=g_dr(features), filter_sd=filter_sd(radius), radius=radius, roi=roi,
                                   film_origin=L[:2])
    gpu.set_filter_spec(**spec_kw)
    gpu.set_filter_split(split)
    try:
        gpu.window_filter(a, 1)
        torch.cuda.synchronize()
        variant = gpu.last_filter_variant()
    finally:
        gpu.set_filter_split(0)
        gpu.set_filter_spec()
    return [o.cpu().numpy()[..., None] for o in outs], variant


@pytest.mark.parametrize("n_buffers,radius,spec_kw,split,variant,blocks", [
    (2, 20, {}, 2, "sym_r20_f", BLOCKS), (5, 20, {}, 2, "sym_r20_f", BLOCKS), (2, 7, {}, 2, "sym_rt_f", BLOCKS), (5, 7, {}, 2, "sym_rt_f", BLOCKS),
    (5, 20, {}, 1, "sym_r20_f+lds_r20_f", ONE_SIDED_BLOCKS), (2, 20, dict(gate=1), 2, "lds_rt_f_asym", ONE_SIDED_BLOCKS),
    (3, 7, dict(gate=2), 2, "lds_rt_f_centre", ONE_SIDED_BLOCKS)],
    ids=["2-sym", "5-sym", "2-sym-r7", "5-sym-r7", "5-sym+one-sided-tail", "2-one-sided-asym", "3-one-sided-centre-r7"])
def test_float_buffers(gpu, n_buffers, radius, spec_kw, split, variant, blocks):
    """filter<float>, the same buffer count on both sides: two buffers per launch on the pair-symmetric kernel; the one-sided kernel
    (the last three of five with the sweep in one part; the one-sided gates) at the blocks whose corner column is a multiple of
    4 and at the others."""
    refs, v_ref = run_float(gpu, n_buffers, radius, spec_kw, split)
    assert v_ref == variant, v_ref
    for B in blocks:
        L = local_rect(B, radius, FILM_W, FILM_H)
        outs, v = run_float(gpu, n_buffers, radius, spec_kw, split, L=L, roi=roi_in(B, L))
        for b, (out, ref) in enumerate(zip(outs, refs)):
            assert_same_bits(out, v, B, L, ref, v_ref, "filter<float> buffer %d of %d r = %d %s split %d" % (b, n_buffers, radius, spec_kw or "default", split))


# ------------------------------------------------------------------ 3. the pack kernels against the stated layout
@functools.lru_cache(maxsize=None)
def pack_case(W, H, welch):
    """Statistics of a W x H block (n, mean, m2, m3, colour, features) and their pre-pass under the spec, from the oracle."""
    from conftest import make_case
    from oracle import oracle
    _, _, st = make_case(W, H, 6, seed=77, features=("radiance", "normal", "albedo", "depth", "materialid"))
    rad = {k: v.copy() for k, v in st["radiance"].items()}
    rad["n"][3, 5] = 1                                                 # infinite discriminator
    rad["n"][4, 6] = 0
    rad["m2"][5, 7] = 0.0
    if welch:
        rad["n"][:, W // 2:] = 2600
    mc, disc = oracle.prepass(rad["n"], rad["mean"], rad["m2"], rad["m3"], spec=oracle.FilterSpec(dof=int(welch)))
    case = dict(n=rad["n"], mean=rad["mean"], m2=rad["m2"], m3=rad["m3"], colour=rad["film_mean"], mc=mc, disc=disc,
                **{f: np.ascontiguousarray(st[f]["mean"], np.float32).reshape(H, W, -1) for f in ("normal", "albedo", "depth", "materialid")})
    for a in case.values():
        a.setflags(write=False)
    return case


PACK_SETS = {16: [("normal", "albedo")], 17: [("depth", "normal", "materialid", "albedo"), ("albedo",), ("materialid",)],
             18: [("materialid", "albedo", "depth", "normal"), ("normal", "albedo"), ("depth",)]}


@pytest.mark.parametrize("W,H,mx,my,Wp,Hp", [(116, 34, 20, 7, 156, 48), (37, 9, 3, 2, 45, 14)], ids=["116x34", "37x9"])
@pytest.mark.parametrize("channels", [16, 17, 18])
@pytest.mark.parametrize("entry", ["pack", "prepass_pack", "prepass_pack_rows"])
def test_pack_kernels_write_the_stated_layout(gpu, entry, channels, W, H, mx, my, Wp, Hp):
    """statmc_pack_filter_inputs / statmc_prepass_pack / statmc_prepass_pack_rows into 16-, 17- and 18-channel images: the block is
    pack_numpy's, as int32 (a count is a denormal bit pattern and must arrive unchanged); absent slots are 0, the G-buffers come
    in any argument order, the margins keep their sentinel; the two outer row ranges, then the middle and an empty range."""
    welch = channels in (16, 18)
    case = pack_case(W, H, welch)
    gpu.set_filter_spec(dof=int(welch))
    try:
        for features in PACK_SETS[channels]:
            gbs = [case[f] for f in features]
            rgb, sc = split_slots(features, gbs)
            want = np.full((Hp, Wp, channels), SENTINEL, np.float32)
            want[my:my + H, mx:mx + W] = pack_numpy(case["mc"], case["disc"], case["colour"], rgb, sc, case["n"], channels)
            img = torch.full((Hp, Wp, channels), SENTINEL, device=DEV)
            d = {k: to_dev(case[k]) for k in ("n", "mean", "m2", "m3", "colour", "mc", "disc")}
            stats = ([d["n"]], [d["mean"]], [d["m2"]], [d["m3"]]) if entry != "pack" else ([d["n"]], [], [], [])
            mc_out, dc_out = (d["mc"], d["disc"]) if entry == "pack" else (torch.full((H, W, 3), SENTINEL, device=DEV), torch.full((H, W, 3), SENTINEL, device=DEV))
            a, keep = gpu.make_filter_args(*stats, [d["colour"]], [mc_out], [dc_out], [torch.zeros(H, W, 3, device=DEV)], [to_dev(g) for g in gbs],
                                           g_dr=g_dr(features), radius=20)
            same = lambda t, w: bool(same_bits(t.cpu().numpy(), w).all())
            what = "%s, %d channels, G-buffers %s" % (entry, channels, features)
            if entry == "pack":
                gpu.pack_filter_inputs(a, img, mx, my)
            elif entry == "prepass_pack":
                gpu.prepass_pack(a, img, mx, my)
            else:
                gpu.prepass_pack(a, img, mx, my, rows=[(0, 5), (H - 9, H)] if H > 14 else [(0, 2), (H - 3, H)])
                lo, hi = (5, H - 9) if H > 14 else (2, H - 3)
                torch.cuda.synchronize()
                part = want.copy()
                part[my + lo:my + hi] = SENTINEL
                assert same(img, part), what + ": the two outer ranges"
                assert bool((mc_out[lo:hi] == SENTINEL).all()) and bool((dc_out[lo:hi] == SENTINEL).all())
                gpu.prepass_pack(a, img, mx, my, rows=[(lo, hi)])
                gpu.prepass_pack(a, img, mx, my, rows=[(3, 3)])            # an empty range
            torch.cuda.synchronize()
            got = img.cpu().numpy()
            bad = np.argwhere(~same_bits(got, want))           # (the same integers, or NaN on both sides)
            assert not len(bad), "%s: %d values differ from the stated layout, first (y, x, channel) %s" % (what, len(bad), bad[:6].tolist())
            if entry != "pack":         # the by-products: the oracle's pre-pass, bit for bit
                assert same(mc_out, case["mc"]) and same(dc_out, case["disc"]), what + ": mean_corr / discriminator"
    finally:
        gpu.set_filter_spec()
