"""The window filter's bit contract, the part that needs no GPU: the helpers of tests/test_filter_bit_contract_gpu.py and
their check against the CPU oracle.

include/statmc.h promises that two window-filter calls with the same pinned split and the same film-anchored tile grid leave
the same bits in a pixel whether it is filtered as part of the whole film, of a region of interest or of a block + halo
image, in every image layout.  The GPU test states that at the C ABI: it cuts block + halo images out of one film, packs them
in every layout the header words, and compares with the whole film.  Everything it needs besides the kernels is here:

  local_rect   the local image of a block: the block dilated by the radius, clipped to the film
  cut          the local image cut out of the film's arrays
  pack_numpy   the 15- / 16- / 17- / 18-channel block + halo pixel as include/statmc.h words it (written from the header's
               packed_inputs paragraph, not from the pack kernels: they are compared with it)
  film_case    the film: noisy statistics that reject about half the taps, real colours, a flat patch; under Welch degrees
               of freedom the discriminator of FilterSpec(dof=1) and counts that jump in the middle of the film

The oracle sums a pixel's taps in one fixed order (dy, then dx, ascending), whatever the image around the window looks like.
So the oracle on the cut-out, with the block as ROI, equals the oracle on the whole film at the block BIT FOR BIT -- if and
only if the rectangle, the clamped border's edge (a local image ends exactly where the film does on true-border sides) and the
counts travel correctly.  That is what test_cut_out_equals_whole_film pins, for every block, spec and radius of the GPU test."""
import functools

import numpy as np
import pytest

from conftest import FILTER_SD, SD_ALBEDO, SD_NORMAL
from test_filter_probes_cpu import flat_patch, noisy_stats, same_bits

# ------------------------------------------------------------------ the cells of the contract (shared with the GPU test)
FILM_W, FILM_H = 300, 72          # three tile columns of the pair-symmetric kernel (128), nine tile rows (8), a ragged right edge
BLOCKS = [
    (0, 0, 148, 36),              # a film corner
    (148, 36, 300, 72),           # origin 4-aligned but on no tile seam; row origin no multiple of 8
    (122, 34, 259, 61),           # origin column = 2 mod 4, local width 4k + 1: register staging instead of LDS-DMA
    (129, 0, 133, 72),            # four columns beside the seam at 128
    (0, 20, 300, 28),             # a band of the Upload / Denoise / Download pipeline
]
BAND = BLOCKS[4]
SPECS_R20 = [dict(), dict(gate=1), dict(gate=2), dict(channel_rule=1), dict(border=1), dict(gate=1, channel_rule=1, border=1), dict(dof=1),
             dict(dof=1, border=1), dict(dof=1, channel_rule=1)]
SPECS_R7 = [dict(), dict(border=1), dict(dof=1)]
CELLS = [(20, s) for s in SPECS_R20] + [(7, s) for s in SPECS_R7]
G_SETS = [("normal", "albedo"), ("albedo",), ("materialid", "depth", "normal", "albedo"), ("depth", "normal")]
FEATURE_SDS = dict(normal=SD_NORMAL, albedo=SD_ALBEDO, depth=2.0, materialid=0.5, tint=0.05)   # (tint: a third RGB G-buffer, for the general kernel)
FEATURE_CHANNELS = dict(normal=3, albedo=3, depth=1, materialid=1, tint=3)


def spec_id(spec_kw):
    return "".join("%s%d" % (k[0], v) for k, v in spec_kw.items()) or "default"


def cell_id(cell):
    return "r%d-%s" % (cell[0], spec_id(cell[1]))


def filter_sd(radius):
    """The shipped spatial sd at the shipped radius, and the same sd : radius at the others."""
    return FILTER_SD * radius / 20.0


def g_dr(features):
    return [-0.5 / FEATURE_SDS[f] ** 2 for f in features]


# ------------------------------------------------------------------ helpers
def local_rect(B, r, W, H):
    """The local image L = (x0, y0, x1, y1) of block B: B dilated by r, clipped to the W x H film."""
    x0, y0, x1, y1 = B
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    return max(x0 - r, 0), max(y0 - r, 0), min(x1 + r, W), min(y1 + r, H)


def roi_in(B, L):
    """Block B (film coordinates) in the coordinates of the local image L."""
    return B[0] - L[0], B[1] - L[1], B[2] - L[0], B[3] - L[1]


def cut(arrays, L):
    """The local image L cut out of film arrays ([H, W] or [H, W, C]; a list gives a list, None stays None)."""
    if arrays is None:
        return None
    if isinstance(arrays, (list, tuple)):
        return [cut(a, L) for a in arrays]
    x0, y0, x1, y1 = L
    return np.ascontiguousarray(arrays[y0:y1, x0:x1])


def pack_numpy(mc, disc, colour, rgb_gbs, sc_gbs, n, channels):
    """The block + halo image of include/statmc.h (statmc_filter_args::packed_inputs), [H, W, channels] float32:
    channels 0 .. 14 mean_corr.rgb, discriminator.rgb, colour.rgb, the first RGB G-buffer, the second; with 17 or 18 channels
    the two 1-channel G-buffers in channels 15 and 16, in argument order; the last channel of 16 or 18 holds the BITS of the
    pixel's int32 sample count.  An absent slot is 0."""
    assert channels in (15, 16, 17, 18) and len(rgb_gbs) <= 2 and len(sc_gbs) <= 2
    assert channels >= 17 or not sc_gbs, "1-channel G-buffers travel in the 17- / 18-channel images"
    H, W = mc.shape[:2]
    out = np.zeros((H, W, channels), np.float32)
    out[..., 0:3], out[..., 3:6], out[..., 6:9] = mc, disc, colour
    for i, g in enumerate(rgb_gbs):
        out[..., 9 + 3 * i:12 + 3 * i] = g
    for i, g in enumerate(sc_gbs):
        out[..., 15 + i] = g.reshape(H, W)
    if channels in (16, 18):
        out.view(np.int32)[..., channels - 1] = n           # (as integers: a count is a denormal bit pattern)
    return out


def split_slots(features, gbs):
    """(RGB G-buffers, 1-channel G-buffers) of a set, each in argument order: the slots of the packed image."""
    return ([g for f, g in zip(features, gbs) if FEATURE_CHANNELS[f] == 3], [g for f, g in zip(features, gbs) if FEATURE_CHANNELS[f] == 1])


@functools.lru_cache(maxsize=None)
def film_case(welch=False, seed=3, W=FILM_W, H=FILM_H):
    """The film: n, mc, disc, colour and every feature's mean, read-only.  Statistics at 6 spp with the discriminator divided
    by 16 (the gate rejects about half the taps, along the image's structure), the film's own colours, a flat patch."""
    from oracle import oracle
    n, mc, disc, colour, feats = noisy_stats(oracle, W, H, 6, seed=seed, features=("radiance", "normal", "albedo", "depth", "materialid"),
                                             spec=oracle.FilterSpec(dof=1 if welch else 0), tighten=16)
    n, colour = n.copy(), np.ascontiguousarray(colour, np.float32).copy()
    if welch:                          # counts that jump inside a tile: pairs far apart in the quantile table
        n[:, W // 2:] = 2600
    flat_patch(mc, disc)
    case = dict(n=n, mc=mc, disc=disc, colour=colour, **{f: np.ascontiguousarray(g, np.float32).reshape(H, W, -1) for f, g in feats.items()})
    case["tint"] = np.ascontiguousarray(0.5 * case["albedo"][..., ::-1] + 0.25 * case["normal"], np.float32)
    for a in case.values():
        a.setflags(write=False)
    return case


def oracle_run(case, features, radius, spec_kw, L=None, roi=None):
    """oracle.filter_image on the film (L None) or on its cut-out L, under the shipped feature sds."""
    from oracle import oracle
    L = L or (0, 0) + case["mc"].shape[1::-1]
    welch = bool(spec_kw.get("dof"))
    return oracle.filter_image(cut(case["mc"], L), cut(case["disc"], L), cut(case["colour"], L), cut([case[f] for f in features], L), g_dr(features),
                               -0.5 / filter_sd(radius) ** 2, radius, roi=roi, spec=oracle.FilterSpec(**spec_kw), n=cut(case["n"], L) if welch else None)


@functools.lru_cache(maxsize=None)
def oracle_whole(features, radius, spec_items):
    spec_kw = dict(spec_items)
    out = oracle_run(film_case(bool(spec_kw.get("dof"))), features, radius, spec_kw)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ tests
def test_local_rect_and_cut():
    W, H = FILM_W, FILM_H
    assert local_rect((0, 0, 148, 36), 20, W, H) == (0, 0, 168, 56)            # no halo beyond a true border
    assert local_rect((148, 36, 300, 72), 20, W, H) == (128, 16, 300, 72)
    assert local_rect((122, 34, 259, 61), 20, W, H) == (102, 14, 279, 72)
    assert local_rect((129, 0, 133, 72), 7, W, H) == (122, 0, 140, 72)
    L = local_rect(BLOCKS[2], 20, W, H)
    assert (L[2] - L[0]) % 4 == 1 and BLOCKS[2][0] % 4 == 2 and L[0] % 4 == 2   # what the block is there for
    assert roi_in(BLOCKS[2], L) == (20, 20, 157, 47)
    a = np.arange(H * W * 2).reshape(H, W, 2)
    c = cut(a, L)
    assert c.shape == (L[3] - L[1], L[2] - L[0], 2) and c.flags["C_CONTIGUOUS"] and c[0, 0, 0] == a[L[1], L[0], 0] and c[-1, -1, 1] == a[L[3] - 1, L[2] - 1, 1]
    assert cut(None, L) is None and cut([a[..., 0]], L)[0].shape == c.shape[:2]
    for B in BLOCKS:                   # every block lies in the film and every local image holds its block's windows
        for r in (20, 7, 24):
            L = local_rect(B, r, W, H)
            x0, y0, x1, y1 = roi_in(B, L)
            assert (x0 == r or L[0] == 0) and (y0 == r or L[1] == 0) and (L[2] - L[0] - x1 == r or L[2] == W) and (L[3] - L[1] - y1 == r or L[3] == H)


def test_pack_numpy_layout():
    """The layouts, channel by channel, from planes that name themselves."""
    H, W = 3, 5
    plane = lambda v, c=3: np.full((H, W, c), v, np.float32) + np.arange(c, dtype=np.float32) / 8
    mc, disc, colour, g0, g1, s0, s1 = plane(1), plane(2), plane(3), plane(4), plane(5), plane(6, 1), plane(7, 1)
    n = np.arange(H * W, dtype=np.int32).reshape(H, W) + 2
    n[1, 2] = 2600
    px = lambda a: a[1, 2].tolist()
    assert px(pack_numpy(mc, disc, colour, [g0, g1], [], None, 15)) == [1, 1.125, 1.25, 2, 2.125, 2.25, 3, 3.125, 3.25, 4, 4.125, 4.25, 5, 5.125, 5.25]
    p17 = pack_numpy(mc, disc, colour, [g1], [s1, s0], None, 17)
    assert px(p17)[9:] == [5, 5.125, 5.25, 0, 0, 0, 7, 6]                      # one RGB G-buffer: slot 1 absent; the 1-channel ones in argument order
    assert px(pack_numpy(mc, disc, colour, [g0, g1], [], None, 17))[15:] == [0, 0]
    p16 = pack_numpy(mc, disc, colour, [g0, g1], [], n, 16)
    assert p16.view(np.int32)[1, 2, 15] == 2600 and 0 < p16[0, 0, 15] < 1e-44     # the count's bits: a denormal float
    p18 = pack_numpy(mc, disc, colour, [], [s0], n, 18)
    assert px(p18)[9:17] == [0, 0, 0, 0, 0, 0, 6, 0] and np.array_equal(p18.view(np.int32)[..., 17], n)
    assert np.array_equal(p18[..., :9], p16[..., :9]) and p18.dtype == np.float32 and p18.flags["C_CONTIGUOUS"]
    with pytest.raises(AssertionError):
        pack_numpy(mc, disc, colour, [g0], [s0], None, 15)


def test_split_slots():
    gbs = ["m", "d", "n", "a"]
    assert split_slots(("materialid", "depth", "normal", "albedo"), gbs) == (["n", "a"], ["m", "d"])
    assert split_slots(("albedo",), ["a"]) == (["a"], [])


@pytest.mark.parametrize("welch", [False, True], ids=["pixel", "welch"])
def test_film_case_is_sensitive(oracle, welch):
    """The film carries what the contract's cells need: a gate that rejects a large share of the taps, the flat patch, every
    feature, and under Welch the jump of the counts."""
    case = film_case(welch)
    assert case["mc"].shape == (FILM_H, FILM_W, 3) and case["depth"].shape == (FILM_H, FILM_W, 1) and case["materialid"].shape == (FILM_H, FILM_W, 1)
    assert (case["disc"][FILM_H - 3, FILM_W // 2:FILM_W // 2 + 4] == 0).all()
    assert bool((case["n"][:, FILM_W // 2:] == 2600).all()) == welch and (case["n"][:, :FILM_W // 2] < 100).all()
    spec = dict(dof=1) if welch else {}
    feats = ("normal", "albedo")
    gbs = [case[f] for f in feats]
    _, _, members = oracle.filter_image_f64(case["mc"], case["disc"], case["colour"], gbs, [0.0, 0.0], -5e-37, 7, spec=oracle.FilterSpec(**spec), n=case["n"])
    _, _, taps = oracle.filter_image_f64(case["mc"], np.full_like(case["disc"], np.inf), case["colour"], gbs, [0.0, 0.0], -5e-37, 7, spec=oracle.FilterSpec(**spec),
                                         n=case["n"])
    print("members / valid taps at r = 7: %.2f" % (members.sum() / taps.sum()))
    assert 0.2 < members.sum() / taps.sum() < 0.8
    out = oracle_whole(feats, 7, tuple(spec.items()))
    assert np.isfinite(out).all() and len(np.unique(out)) > out.size // 2        # real colours: the sums are sensitive to their order


@pytest.mark.parametrize("features", [G_SETS[0], G_SETS[2]], ids=["normal-albedo", "all-four"])
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_cut_out_equals_whole_film(oracle, cell, features):
    """oracle(cut-out, roi = the block) == oracle(whole film) at the block, bit for bit: every block, spec and radius of the GPU
    test, clamp and Welch cells included."""
    radius, spec_kw = cell
    case = film_case(bool(spec_kw.get("dof")))
    whole = oracle_whole(features, radius, tuple(spec_kw.items()))
    for B in BLOCKS:
        L = local_rect(B, radius, FILM_W, FILM_H)
        roi = roi_in(B, L)
        out = oracle_run(case, features, radius, spec_kw, L=L, roi=roi)
        assert out.shape == (L[3] - L[1], L[2] - L[0], 3)
        inside = np.zeros(out.shape[:2], bool)
        inside[roi[1]:roi[3], roi[0]:roi[2]] = True
        assert not out[~inside].any(), "block %s: the oracle wrote outside the ROI" % (B,)
        ok = same_bits(out[roi[1]:roi[3], roi[0]:roi[2]], whole[B[1]:B[3], B[0]:B[2]])
        assert ok.all(), "block %s r = %d %s: %d pixels of the cut-out differ from the whole film, first (y, x, c) %s" % (
            B, radius, spec_kw, (~ok.all(2)).sum(), np.argwhere(~ok)[:4].tolist())
    # the band as a ROI of the whole film: the same bits as well
    out = oracle_run(case, features, radius, spec_kw, roi=BAND)
    assert same_bits(out[BAND[1]:BAND[3]], whole[BAND[1]:BAND[3]]).all() and not out[:BAND[1]].any() and not out[BAND[3]:].any()
