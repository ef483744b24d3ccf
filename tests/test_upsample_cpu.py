"""statmc_upsample_filtered (include/statmc.h) without a GPU: the symbol, its declaration and the ctypes mirror; the argument checks
of statmc_amd/csrc/statmc_upsample_args.h -- compiled alone into tests/cpp/test_upsample_args.cpp, plain and under AddressSanitizer
and UBSan -- against a table of the header's rules, in the header's order; what the built library answers without a device; and
the properties of the numpy float32 restatement (tests/upsample_reference.py) that tests/test_upsample_gpu.py holds the device to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import upsample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_upsample_args.cpp")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -2
ULP = 2.0 ** -23          # of a float32 in [1, 2): the unit the bounds below are counted in


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- 1. the args header, alone
# name -> (code, the words the message must hold): the rules of include/statmc.h.  The program's film is 37 x 23, two buffers, G-buffers
# of 3, 3 and 1 channels.
RULES = {
    "null_fine": (INVALID, ["fine"]),
    "null_coarse": (INVALID, ["coarse"]),
    "k_3": (INVALID, ["k = 3"]),
    "k_16": (INVALID, ["k = 16"]),
    "k_comes_before_channels": (INVALID, ["k = 1"]),
    "channels_2": (INVALID, ["channels = 2"]),
    "empty_fine": (INVALID, ["fine", "empty"]),
    "coarse_size_floor": (INVALID, ["coarse is 18x12", "19x12"]),
    "coarse_height": (INVALID, ["coarse is 10x7", "10x6"]),
    "n_buffers_differ": (INVALID, ["n_buffers"]),
    "n_g_buffers_differ": (INVALID, ["n_g_buffers"]),
    "g_channel_counts_differ": (INVALID, ["g_channel_counts[2]"]),
    "null_g_table": (INVALID, ["fine", "G-buffer table"]),
    "null_coarse_g_table": (INVALID, ["coarse", "G-buffer table"]),
    "welch": (UNSUPPORTED, ["STATMC_DOF_WELCH"]),
    "size_comes_before_welch": (INVALID, ["coarse is 20x12"]),
    "packed_fine": (UNSUPPORTED, ["fine->packed_inputs"]),
    "packed_coarse": (UNSUPPORTED, ["coarse->packed_inputs"]),
    "three_rgb_g_buffers": (UNSUPPORTED, ["g_buffers[2]"]),
    "g_channels_2": (UNSUPPORTED, ["g_channel_counts[2] = 2"]),
    "null_mean_corr_table": (INVALID, ["fine", "mean_corr"]),
    "null_coarse_discriminator_table": (INVALID, ["coarse", "discriminator"]),
    "null_film_table": (INVALID, ["fine", "film"]),
    "null_coarse_filtered_table": (INVALID, ["coarse", "film_filtered"]),
    "null_image": (INVALID, ["fine->discriminator[1]", "null"]),
    "null_coarse_image": (INVALID, ["coarse->film_filtered[0]", "null"]),
    "image_size": (INVALID, ["coarse->mean_corr[1]", "20x12"]),
    "short_pitch": (INVALID, ["fine->film[0]", "pitch"]),
    "pitched_fine": (UNSUPPORTED, ["fine->film[0]", "pitch"]),
    "pitched_coarse_g": (UNSUPPORTED, ["coarse->g_buffers[0]", "pitch"]),
    "misaligned": (INVALID, ["fine->mean_corr[0]", "aligned"]),
    "roi_outside": (INVALID, ["roi [0,38)x[0,4)"]),
    "roi_empty": (INVALID, ["roi [5,5)"]),
    "image_comes_before_roi": (INVALID, ["fine->mean_corr[0]"]),
    "out_is_colour": (INVALID, ["output 0", "colour image 0"]),
    "out_overlaps_mean_corr_tail": (INVALID, ["output 1", "fine->mean_corr[0]"]),
    "out_is_other_out": (INVALID, ["output 0", "output 1"]),
    "out_overlaps_coarse_filtered": (INVALID, ["output 0", "coarse filtered image 1"]),
    "out_overlaps_fine_g": (INVALID, ["output 0", "fine->g_buffers[2]"]),
    "out_overlaps_coarse_g": (INVALID, ["output 1", "coarse->g_buffers[0]"]),
    "roi_comes_before_overlap": (INVALID, ["roi [-1,4)"]),
}
# name -> what fill_upsample_args makes of a valid call: shift = log2(2 k), the coarse size, vec, the flat pixel range, workgroups, ROI
VALID = {
    "valid_k2_rgb": "2 19 12 1 0 851 1 0,0,37,23",
    "valid_k4_rgb": "3 10 6 1 0 851 1 0,0,37,23",
    "valid_k8_float": "4 5 3 1 0 851 1 0,0,37,23",
    "valid_roi": "2 19 12 1 184 333 1 3,5,30,9",             # rows 5 .. 8: pixels 185 .. 332, begun on the quad at 184
    "valid_unaligned_plane": "2 19 12 0 0 851 1 0,0,37,23",
    "valid_denoise_film_without_film_tables": "2 19 12 1 0 851 1 0,0,37,23",
    "valid_no_g_buffers": "2 19 12 1 0 851 1 0,0,37,23",
}


def verdicts(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out():
    from statmc_amd import build
    build.build_tools()
    return verdicts(build.UPSAMPLE_ARGS_BIN)


def test_the_args_header_gives_the_rules_of_the_header(args_out):
    got = dict(line.split(" : ", 1) for line in args_out.splitlines())
    assert set(got) == set(RULES) | set(VALID)
    for name, (code, words) in RULES.items():
        rc, msg = got[name].split(" ", 1)
        assert int(rc) == code, (name, got[name])
        for w in words:
            assert w in msg, (name, w, msg)
    for name, filled in VALID.items():
        assert got[name] == "0 ok " + filled, (name, got[name])


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    binary = str(tmp_path / "upsample_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary) == args_out


# ---------------------------------------------------------------- 2. the library, without a device
def test_the_symbol_is_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    sym = "statmc_upsample_filtered"
    assert hasattr(lib, sym) and sym in api.EXPORTS
    decl = re.search(r"int " + sym + r"\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(decl.group(1).split()) == "const statmc_filter_args *fine, const statmc_filter_args *coarse, int k, int channels"
    assert "statmc_upsample.hip" in build.SOURCES and "statmc_upsample_args.h" in build.HEADERS
    assert callable(api.upsample_filtered) and callable(film.FilmStats.preview) and callable(film.FilmStats.upsample_from)
    # the window-filter kernels are not this entry's: it has a translation unit of its own
    for name in ("statmc_filter.hip", "statmc_filter_sym.hip"):
        assert "upsample" not in open(os.path.join(ROOT, "statmc_amd", "csrc", name)).read()


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up pointers, never dereferenced: a refusal names its argument whether or not a device is set up."""
    from statmc_amd import api
    img = lambda at, w, h, ch: api.Image(C.c_void_p(at), w * ch * 4, w, h)

    def block(w, h, base):
        a = api.FilterArgs()
        a.n_buffers, a.width, a.height = 1, w, h
        tabs = [(api.Image * 1)(img(base + (i << 20), w, h, 3)) for i in range(4)]
        a.mean_corr, a.discriminator, a.film, a.film_filtered = tabs
        return a, tabs

    fine, keep_f = block(37, 23, 16 << 20)
    coarse, keep_c = block(19, 12, 64 << 20)
    call = lambda k=2, ch=3: lib.statmc_upsample_filtered(C.byref(fine), C.byref(coarse), k, ch)
    assert call(k=3) == api.ERR_INVALID and b"k = 3" in lib.statmc_last_error()
    assert call(ch=4) == api.ERR_INVALID and b"channels = 4" in lib.statmc_last_error()
    assert call(k=4) == api.ERR_INVALID and b"coarse is 19x12" in lib.statmc_last_error()
    assert lib.statmc_upsample_filtered(None, C.byref(coarse), 2, 3) == api.ERR_INVALID and b"null fine" in lib.statmc_last_error()
    keep_f[3][0].data = keep_f[2][0].data
    assert call() == api.ERR_INVALID and b"output 0 overlaps" in lib.statmc_last_error()
    keep_f[3][0].data = (16 << 20) + (3 << 20)
    import torch
    if not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_upsample_gpu.py runs real ones)
        assert call() == api.ERR_NO_DEVICE and b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- 3. the restatement's own properties
def draw(w, h, k, seed, ch=3):
    """a film and its coarse twin with unrelated positive values"""
    rng = np.random.default_rng(seed)
    wc, hc = ref.coarse_size(w, h, k)
    fine = dict(mean_corr=rng.uniform(0.5, 2, (h, w, ch)).astype(F32), disc=rng.uniform(0.01, 0.5, (h, w, ch)).astype(F32),
                colour=rng.uniform(0.5, 2, (h, w, ch)).astype(F32))
    coarse = dict(mean_corr=rng.uniform(0.5, 2, (hc, wc, ch)).astype(F32), disc=rng.uniform(0.01, 0.5, (hc, wc, ch)).astype(F32),
                  filtered=rng.uniform(0.5, 2, (hc, wc, ch)).astype(F32))
    return fine, coarse


def ulps(a, b):
    """|a - b| in units of the last place of b's magnitude (float32)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (np.abs(b) * 2.0 ** -24 * 2)       # ulp(b) <= 2^-23 |b|: an upper bound of the count


def test_the_grid_position_is_the_header_s():
    for k in (2, 4, 8):
        x0, w0, w1 = ref.grid_position(37, k)
        assert x0[0] == -1 and (x0[:k // 2] == -1).all() and x0[k // 2] == 0
        assert x0[36] == (2 * 36 + 1 - k) // (2 * k)
        centre = (np.arange(37) + 0.5) / k - 0.5                   # the fine pixel's centre on the grid of block centres
        assert np.array_equal(x0, np.floor(centre)) and np.array_equal(w1.astype(np.float64), centre - np.floor(centre))
        assert np.array_equal(w0.astype(np.float64) + w1.astype(np.float64), np.ones(37))


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("border", [ref.BORDER_CLIP, ref.BORDER_CLAMP])
def test_a_constant_film_maps_to_the_constant_bit_for_bit(k, border):
    """Every tap carries the constant c and passes the gate (d = 0, D >= 0).  A tent weight has at most 8 significant bits and a partial
    sum of weights at most 9 (m / 256, m <= 256), so with a c of 12 bits every product and partial sum is exact, and so is the
    quotient."""
    w, h = 37, 23
    wc, hc = ref.coarse_size(w, h, k)
    c = F32(761.0 / 1024.0)
    full = lambda H, W, v: np.full((H, W, 3), v, F32)
    fine = dict(mean_corr=full(h, w, c), disc=full(h, w, 0), colour=full(h, w, c))
    coarse = dict(mean_corr=full(hc, wc, c), disc=full(hc, wc, 0), filtered=full(hc, wc, c))
    for gate in (0, 1, 2):
        for rule in (0, 1):
            r = ref.upsample_ref(fine, coarse, k, gate, rule, border)
            assert not r["fallback"].any()
            assert np.array_equal(r["out"].view(np.uint32), fine["colour"].view(np.uint32))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_an_open_gate_under_a_clamped_border_is_the_bilinear_interpolation(k):
    """Every discriminator +inf, no features, STATMC_BORDER_CLAMP: each pixel is torch's bilinear interpolation with half-pixel
    centres (align_corners=False, scale 1 / k, cropped to the film) of the coarse image, to <= 2 ulp -- the independent check of
    the tent arithmetic."""
    import torch
    w, h = 37, 23
    fine, coarse = draw(w, h, k, seed=k)
    fine["disc"][:] = np.inf
    coarse["disc"][:] = np.inf
    r = ref.upsample_ref(fine, coarse, k, border=ref.BORDER_CLAMP)
    assert r["member"].all() and not r["fallback"].any()
    t = torch.from_numpy(coarse["filtered"]).permute(2, 0, 1)[None]
    want = torch.nn.functional.interpolate(t, scale_factor=float(k), mode="bilinear", align_corners=False, recompute_scale_factor=False)
    want = want[0].permute(1, 2, 0).numpy()[:h, :w]
    assert want.shape == r["out"].shape
    assert ulps(r["out"], want).max() <= 2
    assert ulps(r["out64"], want).max() <= 2


@pytest.mark.parametrize("k", [2, 4, 8])
def test_a_clipped_border_renormalises_the_in_image_candidates(k):
    """Under STATMC_BORDER_CLIP a border pixel's taps are its in-image candidates only, and its value their convex combination; in
    exact arithmetic that is the clamped image (an outside tap clamps onto the pixel its in-image partner already is).  In float32
    each side makes at most 4 products, 3 + 3 additions and 1 quotient of positive numbers: the two differ by under 9 * 2^-24
    relative, and not at all away from the border."""
    w, h = 37, 23
    wc, hc = ref.coarse_size(w, h, k)
    fine, coarse = draw(w, h, k, seed=10 + k)
    fine["disc"][:] = np.inf
    clip = ref.upsample_ref(fine, coarse, k, border=ref.BORDER_CLIP)
    clamp = ref.upsample_ref(fine, coarse, k, border=ref.BORDER_CLAMP)
    x0, _, _ = ref.grid_position(w, k)
    y0, _, _ = ref.grid_position(h, k)
    for tap, (j, i) in enumerate(ref.TAPS):
        inside = ((y0 + j >= 0) & (y0 + j < hc))[:, None] & ((x0 + i >= 0) & (x0 + i < wc))[None, :]
        assert np.array_equal(clip["member"][..., tap], inside)
    assert clamp["member"].all() and not clip["fallback"].any()
    border = ~clip["member"].all(-1)
    # (the last row and column are border pixels only where the edge block is a whole one: a partial block's centre lies past them)
    assert border[0].all() and border[:, 0].all() and not border[h // 2, w // 2]
    assert border[-1].all() == (h % k == 0 or h % k > k // 2) and border[:, -1].all() == (w % k == 0 or w % k > k // 2)
    assert np.array_equal(clip["out"][~border].view(np.uint32), clamp["out"][~border].view(np.uint32))
    assert (np.abs(clip["out"].astype(np.float64) - clamp["out"]) <= 9 * 2.0 ** -24 * clamp["out"]).all()
    lo = np.minimum.reduce([coarse["filtered"].min()]), np.maximum.reduce([coarse["filtered"].max()])
    assert (clip["out"] >= lo[0]).all() and (clip["out"] <= lo[1]).all()
    # a corner has one candidate: fl(fl(w c) / w), two roundings from c (the bits of c where w is a power of two)
    assert ulps(clip["out"][0, 0], coarse["filtered"][0, 0]).max() <= 2


@pytest.mark.parametrize("gate", [0, 1, 2])
@pytest.mark.parametrize("rule", [0, 1])
def test_closed_gates_pass_the_fine_colour_through_bit_for_bit(gate, rule):
    """Every discriminator 0 and all means distinct: no pair is a member, every pixel keeps its own colour's bits."""
    fine, coarse = draw(37, 23, 4, seed=3)
    fine["disc"][:] = 0
    coarse["disc"][:] = 0
    assert not np.isin(fine["mean_corr"], coarse["mean_corr"]).any()
    fine["colour"][2, 3, 1] = F32(-0.0)
    r = ref.upsample_ref(fine, coarse, 4, gate, rule, ref.BORDER_CLAMP)
    assert r["fallback"].all() and not r["member"].any()
    assert np.array_equal(r["out"].view(np.uint32), fine["colour"].view(np.uint32))


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("gate", [0, 1, 2])
def test_no_candidate_across_an_edge_is_a_member(k, gate):
    """Two half-planes with means 1 and 5 and tiny variances, the edge inside a coarse block: a coarse pixel takes part in a fine
    pixel's sums only if it lies wholly on that pixel's side, so no output leaves the range of its own side's coarse values; the
    blocks that straddle the edge (mean 3) serve nobody.  The range is that of the exact convex combination: the float32 one makes at
    most 4 products, 3 + 3 additions and 1 quotient of positive numbers, each within 2^-24, so it may pass an end by 9 * 2^-24 of it."""
    w, h, edge = 37, 23, 21            # 21 is a multiple of no k: the edge cuts a block
    wc, hc = ref.coarse_size(w, h, k)
    rng = np.random.default_rng(5)
    side = np.where(np.arange(w) < edge, 1.0, 5.0)
    c_lo, c_hi = np.arange(wc) * k, np.minimum(np.arange(wc) * k + k, w)
    c_side = np.where(c_hi <= edge, 1.0, np.where(c_lo >= edge, 5.0, 3.0))
    assert (c_side == 3.0).sum() == 1
    fine = dict(mean_corr=np.broadcast_to(side[None, :, None], (h, w, 3)).astype(F32), disc=np.full((h, w, 3), 1e-6, F32),
                colour=(side[None, :, None] + rng.uniform(-0.2, 0.2, (h, w, 3))).astype(F32))
    coarse = dict(mean_corr=np.broadcast_to(c_side[None, :, None], (hc, wc, 3)).astype(F32), disc=np.full((hc, wc, 3), 1e-6, F32),
                  filtered=(c_side[None, :, None] + rng.uniform(-0.1, 0.1, (hc, wc, 3))).astype(F32))
    for rule in (0, 1):
        r = ref.upsample_ref(fine, coarse, k, gate, rule, ref.BORDER_CLAMP)
        x0, _, _ = ref.grid_position(w, k)
        for tap, (j, i) in enumerate(ref.TAPS):
            cand = c_side[np.clip(x0 + i, 0, wc - 1)]
            assert np.array_equal(r["member"][..., tap], np.broadcast_to(cand == side, (h, w)))
        for s, cols in ((1.0, np.arange(w) < edge), (5.0, np.arange(w) >= edge)):
            own = coarse["filtered"][:, c_side == s]
            got = r["out"][:, cols & ~r["fallback"].all(0)]
            slack = 9 * 2.0 ** -24
            assert got.size and got.min() >= own.min() * (1 - slack) and got.max() <= own.max() * (1 + slack)
            assert got.min() > s - 0.11 and got.max() < s + 0.11         # nowhere near the other side's 1 or 5, or the straddler's 3
        fb = r["fallback"]
        assert np.array_equal(r["out"][fb].view(np.uint32), fine["colour"][fb].view(np.uint32))


def test_invalid_pixels_pass_through_and_invalid_candidates_are_skipped():
    fine, coarse = draw(37, 23, 2, seed=8)
    fine["disc"][:] = np.inf
    fine["g"], coarse["g"] = [np.ones((23, 37, 3), F32)], [np.ones((12, 19, 3), F32)]
    fine["mean_corr"][4, 5, 0] = np.nan
    fine["colour"][4, 5, 2] = np.nan
    fine["g"][0][9, 9, 1] = np.inf
    coarse["mean_corr"][3, 3, 1] = np.nan
    coarse["filtered"][5, 7, 0] = np.inf
    coarse["g"][0][8, 2, 2] = np.nan
    coarse["disc"][10:12, 10:12] = np.nan          # a whole 2 x 2 neighbourhood
    r = ref.upsample_ref(fine, coarse, 2, border=ref.BORDER_CLAMP, g_dr=[-0.5])
    # fine pixels 21 and 22 have X0 = 10: the four of them see nothing but the neighbourhood
    assert r["fallback"][4, 5] and r["fallback"][9, 9] and r["fallback"][21:23, 21:23].all()
    assert np.array_equal(r["out"][4, 5].view(np.uint32), fine["colour"][4, 5].view(np.uint32))
    assert r["fallback"].sum() == 6
    assert np.isfinite(r["out"][~r["fallback"]]).all()
    # fine pixel (6, 6): x0 = 2 -- its taps are coarse (2..3, 2..3); coarse (3, 3) is out
    assert list(r["member"][6, 6]) == [True, True, True, False]
    # equal features: e == 0, the float and the double evaluation see the same weights
    assert np.abs(r["out"].astype(np.float64) - r["out64"])[~r["fallback"]].max() <= 4 * 2.0 ** -24 * 2


def test_the_vectorised_fma_is_libm_s_bit_for_bit():
    """fmaf_fast (tools/time_upsample.py checks full-size films with it) against libm on random operands, on sums that land exactly
    half-way between two float32 in float64, on subnormal results and on the non-finite cases"""
    rng = np.random.default_rng(4)
    a = (rng.normal(0, 1, 20000) * 2.0 ** rng.integers(-20, 20, 20000)).astype(F32)
    b = (rng.normal(0, 1, 20000) * 2.0 ** rng.integers(-20, 20, 20000)).astype(F32)
    c = (-(a.astype(np.float64) * b) * rng.choice([1.0, 1 + 2.0 ** -20, 0.5, 3.0], 20000)).astype(F32)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: with c = 0 the exact product is a float32 half-way point; a tiny c decides the side
    one = np.full(6, 1 + 2.0 ** -12, F32)
    tie_c = np.array([0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -149, -2.0 ** -149, 2.0 ** -30], F32)
    small = np.array([2.0 ** -70, 3 * 2.0 ** -75, 2.0 ** -64, 1.5 * 2.0 ** -63], F32)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 3e38], F32)
    for x, y, z in ((a, b, c), (one, one, tie_c), (small, small, -small * small), (small, small, np.zeros(4, F32)),
                    (special, special[::-1].copy(), special), (special, np.ones(6, F32), -special)):
        assert np.array_equal(ref.fmaf_fast(x, y, z).view(np.uint32), ref.fmaf(x, y, z).view(np.uint32))
    fine, coarse = draw(37, 23, 4, seed=12)
    fine["g"], coarse["g"] = [fine["colour"] * 0.3], [coarse["filtered"] * 0.3]
    for gate in (0, 1, 2):
        slow = ref.upsample_ref(fine, coarse, 4, gate, 1, 1, [-3.0])
        fast = ref.upsample_ref(fine, coarse, 4, gate, 1, 1, [-3.0], fma=ref.fmaf_fast)
        assert np.array_equal(slow["out"].view(np.uint32), fast["out"].view(np.uint32)) and np.array_equal(slow["member"], fast["member"])
