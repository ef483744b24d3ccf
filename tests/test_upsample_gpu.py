"""statmc_upsample_filtered on the device against the numpy float32 restatement of include/statmc.h (tests/upsample_reference.py,
whose own properties tests/test_upsample_cpu.py checks): with factors 0 the output bit for bit -- which identifies the member taps of
every pixel --, the fallback mask, the G-buffer range term to 1e-5 against the float64 evaluation, invalid pixels, the ROI, every
refusal, and the upper layers: FilmStats.preview and statmc_denoise --pool k --upsample.  Every call goes through the C ABI on a
library stream, not the default one."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import upsample_reference as ref
from conftest import FILTER_SD, RADIUS, SD_ALBEDO, SD_NORMAL

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
SENTINEL = F32(-777.25)
# (W, H, k, planes 4 bytes off a 16-byte boundary): partial edge blocks in both axes and Hc = 3 at k = 8; a 1 x 1 coarse film; a 1 x 1
# film; a wave's run ending on the row; a wave straddling rows over unaligned planes
SHAPES = [(37, 23, 2, False), (37, 23, 4, False), (37, 23, 8, False), (5, 3, 8, False), (1, 1, 2, False), (64, 8, 2, False), (67, 5, 4, True)]
SHAPE_IDS = ["%dx%d_k%d%s" % (w, h, k, "_unaligned" if off else "") for w, h, k, off in SHAPES]
SPECS = [(gate, rule, border) for gate in (0, 1, 2) for rule in (0, 1) for border in (0, 1)]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def dev(a, offset=False):
    """a numpy image on the device; offset: starting 4 bytes into its allocation (4-byte but not 16-byte aligned)"""
    import torch
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a.copy()).to(DEV)
    flat = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
    buf = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device=DEV)
    view = buf[1:1 + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(a.shape)


@pytest.fixture(scope="module")
def stream(gpu):
    lib = gpu.load()
    s = C.c_void_p()
    gpu.check(lib.statmc_stream_create(C.byref(s)))
    yield s
    gpu.check(lib.statmc_stream_destroy(s))


@pytest.fixture()
def spec(gpu):
    """sets the device's filter spec for a test and puts the pinned one back"""
    yield lambda gate=0, rule=0, border=0, dof=0: gpu.set_filter_spec(gate=gate, channel_rule=rule, border=border, dof=dof)
    gpu.set_filter_spec()


def draw(w, h, k, ch, seed, g_channels=()):
    """Statistics with a mixed verdict: means on a few levels plus noise, discriminators from 0 over the noise's scale to +inf, so
    that every gate accepts some pairs and refuses others; colours unrelated to everything, so that a sum's bits name its taps."""
    rng = np.random.default_rng(seed)
    wc, hc = ref.coarse_size(w, h, k)

    def side(hh, ww):
        mc = (rng.integers(0, 3, (hh, ww, 1)) * 0.5 + rng.normal(0, 0.15, (hh, ww, ch))).astype(F32)
        disc = (rng.uniform(0, 0.08, (hh, ww, ch)) ** 2 * 4).astype(F32)
        u = rng.random((hh, ww, 1))
        disc = np.where(u < 0.08, F32(0), np.where(u > 0.92, F32(np.inf), disc)).astype(F32)
        colour = rng.uniform(0.25, 4, (hh, ww, ch)).astype(F32)
        g = [rng.uniform(0, 1, (hh, ww, gc)).astype(F32) for gc in g_channels]
        return mc, disc, colour, g

    mc, disc, col, g = side(h, w)
    cmc, cdisc, cf, cg = side(hc, wc)
    return dict(mean_corr=mc, disc=disc, colour=col, g=g), dict(mean_corr=cmc, disc=cdisc, filtered=cf, g=cg)


def squeeze(a, ch):
    return a[..., 0] if ch == 1 else a


def upload(fine, coarse, ch, offset=False):
    f = {key: dev(squeeze(fine[key], ch), offset) for key in ("mean_corr", "disc", "colour")}
    c = {key: dev(squeeze(coarse[key], ch), offset) for key in ("mean_corr", "disc", "filtered")}
    f["g"] = [dev(G if G.shape[-1] == 3 else G[..., 0], offset) for G in fine["g"]]
    c["g"] = [dev(G if G.shape[-1] == 3 else G[..., 0], offset) for G in coarse["g"]]
    f["out"] = dev(np.full(squeeze(fine["colour"], ch).shape, SENTINEL, F32), offset)
    return f, c


def blocks(gpu, f, c, stream, g_dr, roi=None):
    import torch
    fa, keep_f = gpu.make_filter_args(n=[], mean=[], m2=[], m3=[], film=[f["colour"]], mean_corr=[f["mean_corr"]], disc=[f["disc"]],
                                      film_filtered=[f["out"]], g_buffers=f["g"], g_dr=list(g_dr), roi=roi, stream=stream)
    unused = torch.zeros_like(c["filtered"])      # the coarse colour image: not read by the call
    ca, keep_c = gpu.make_filter_args(n=[], mean=[], m2=[], m3=[], film=[unused], mean_corr=[c["mean_corr"]], disc=[c["disc"]],
                                      film_filtered=[c["filtered"]], g_buffers=c["g"], g_dr=list(g_dr), stream=stream)
    return fa, ca, (keep_f, keep_c, unused)


def run(gpu, stream, f, c, k, ch, g_dr=(), roi=None):
    """one call on the library stream; the default stream is idle before (the uploads) and the library stream after"""
    import torch
    fa, ca, keep = blocks(gpu, f, c, stream, g_dr, roi)
    torch.cuda.synchronize()
    gpu.upsample_filtered(fa, ca, k, ch)
    gpu.check(gpu.load().statmc_synchronize(stream))
    out = f["out"].cpu().numpy()
    return out[..., None] if ch == 1 else out


# ---------------------------------------------------------------- membership, fallback and bits
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_with_zero_factors_every_bit_is_the_restatement_s(gpu, stream, spec, shape, ch):
    """e == 0: the exponential is exactly 1 and every other operation is IEEE, so the device's image IS the restatement's.  The coarse
    colours are unrelated random numbers: a sum over another set of taps has other bits, so equal bits mean equal member sets, and a
    pixel holds its own colour's bits exactly where the restatement falls back.  Every gate x channel rule x border; without
    G-buffers, and with two RGB G-buffers whose factors are 0."""
    w, h, k, offset = shape
    for g_channels, g_dr in (((), ()), ((3, 3), (0.0, 0.0))):
        fine, coarse = draw(w, h, k, ch, seed=w + 3 * k + ch, g_channels=g_channels)
        f, c = upload(fine, coarse, ch, offset)
        seen = set()
        for gate, rule, border in SPECS:
            spec(gate, rule, border)
            want = ref.upsample_ref(fine, coarse, k, gate, rule, border, g_dr)
            f["out"].fill_(float(SENTINEL))
            got = run(gpu, stream, f, c, k, ch, g_dr)
            assert np.array_equal(bits(got), bits(want["out"])), (gate, rule, border, g_channels)
            own = (bits(got) == bits(fine["colour"])).all(-1)
            assert np.array_equal(own, want["fallback"]), (gate, rule, border)
            seen.add(want["member"].tobytes())
        if w * h > 100:     # the cases tell the specs apart: the centre gate and the borders select other taps (symmetric and asymmetric
                            # differ by a rounding only)
            assert len(seen) >= 4 and 0 < want["fallback"].sum() < w * h


# ---------------------------------------------------------------- the G-buffer range term
@pytest.mark.parametrize("g_channels", [(3, 3), (3, 3, 1, 1), (1, 3)], ids=["rgb_rgb", "rgb_rgb_depth_id", "depth_rgb"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[6]], ids=[SHAPE_IDS[1], SHAPE_IDS[6]])
def test_the_range_term_is_within_1e5_of_the_float64_evaluation(gpu, stream, spec, shape, g_channels):
    """Non-zero factors: per channel <= 1e-5 relative L2 against the float64 evaluation of the same taps -- the bound include/statmc.h
    states for every filter kernel (the exponential is the hardware's) -- and still the restatement's fallback mask."""
    from conftest import rel_l2
    w, h, k, offset = shape
    g_dr = [-0.5 / (sd * sd) for sd in (0.4, 0.25, 1.0, 0.5)][:len(g_channels)]
    for ch in (1, 3):
        fine, coarse = draw(w, h, k, ch, seed=11 + len(g_channels) + ch, g_channels=g_channels)
        f, c = upload(fine, coarse, ch, offset)
        for gate, rule, border in ((0, 0, 0), (1, 1, 1), (2, 0, 1)):
            spec(gate, rule, border)
            want = ref.upsample_ref(fine, coarse, k, gate, rule, border, g_dr)
            got = run(gpu, stream, f, c, k, ch, g_dr)
            fb = want["fallback"]
            assert np.array_equal(bits(got)[fb], bits(fine["colour"])[fb])
            assert not (bits(got)[~fb] == bits(fine["colour"])[~fb]).all(-1).any()
            for cc in range(ch):
                err = rel_l2(got[..., cc], want["out64"][..., cc])
                print("range term %s %dx%d k=%d ch=%d spec=%s channel %d: rel L2 %.3g" % (g_channels, w, h, k, ch, (gate, rule, border), cc, err))
                assert err <= 1e-5
            assert 0 < fb.sum() < w * h
            # the weights moved something: this is not the zero-factor image
            assert not np.array_equal(bits(got), bits(ref.upsample_ref(fine, coarse, k, gate, rule, border, [0.0] * len(g_dr))["out"]))


# ---------------------------------------------------------------- invalid pixels
def test_invalid_pixels_pass_through_and_invalid_candidates_are_skipped(gpu, stream, spec):
    w, h, k = 37, 23, 2
    fine, coarse = draw(w, h, k, 3, seed=5, g_channels=(3, 1))
    fine["disc"][:] = np.inf                          # every valid pair is a member: only validity decides
    nan_payload = np.array([0x7fc12345], np.uint32).view(F32)[0]
    fine["mean_corr"][4, 5, 0] = np.nan               # single fine pixels
    fine["disc"][6, 30, 2] = np.nan
    fine["colour"][4, 5, 2] = nan_payload             # ... one of them with a NaN colour that passes through, payload and all
    fine["colour"][9, 9, 1] = np.inf                  # a non-finite colour makes the pixel invalid by itself
    fine["g"][1][12, 3, 0] = np.nan
    coarse["mean_corr"][3, 3, 1] = np.nan             # single coarse pixels
    coarse["filtered"][5, 7, 0] = np.inf
    coarse["g"][0][8, 2, 2] = -np.inf
    coarse["disc"][10:12, 10:12] = np.nan             # a whole 2 x 2 neighbourhood: fine pixels (21..22, 21..22) see nothing else
    f, c = upload(fine, coarse, 3)
    for border in (0, 1):
        spec(0, 0, border)
        want = ref.upsample_ref(fine, coarse, k, border=border, g_dr=[0.0, 0.0])
        got = run(gpu, stream, f, c, k, 3, [0.0, 0.0])
        assert np.array_equal(bits(got), bits(want["out"]))
        fb = want["fallback"]
        assert fb[4, 5] and fb[6, 30] and fb[9, 9] and fb[12, 3] and fb[21:23, 21:23].all() and fb.sum() == 8
        assert bits(got)[4, 5, 2] == 0x7fc12345 and np.isinf(got[9, 9, 1])
        assert np.isfinite(got[~fb]).all()
        assert list(want["member"][6, 6]) == [True, True, True, False]      # coarse (3, 3) is skipped, its neighbours serve


# ---------------------------------------------------------------- ROI
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[6]], ids=[SHAPE_IDS[0], SHAPE_IDS[6]])
def test_two_disjoint_roi_calls_are_the_whole_film_call(gpu, stream, spec, shape):
    w, h, k, offset = shape
    fine, coarse = draw(w, h, k, 3, seed=21, g_channels=(3, 3))
    g_dr = [-2.0, -3.0]
    f, c = upload(fine, coarse, 3, offset)
    spec(0, 0, 1)
    whole = run(gpu, stream, f, c, k, 3, g_dr).copy()
    assert not (whole == SENTINEL).any()
    y = h // 2
    rois = [(0, 0, w, y), (3, y, w - 2, h)]           # whole rows (the vector path where aligned), then a window with both x edges inside
    f["out"].fill_(float(SENTINEL))
    for roi in rois:
        got = run(gpu, stream, f, c, k, 3, g_dr, roi=roi)
    inside = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in rois:
        inside[y0:y1, x0:x1] = True
    assert np.array_equal(bits(got)[inside], bits(whole)[inside])
    assert (got[~inside] == SENTINEL).all() and (~inside).any()


# ---------------------------------------------------------------- refusals
def test_every_refusal_returns_its_code_names_its_argument_and_writes_nothing(gpu, stream, spec):
    import torch
    api, lib = gpu, gpu.load()
    w, h, k = 37, 23, 2
    fine, coarse = draw(w, h, k, 3, seed=2, g_channels=(3, 3, 1))
    f, c = upload(fine, coarse, 3)
    g_dr = [-1.0, -1.0, -1.0]

    def refused(code, word, change=None, k=k, ch=3, fine_null=False, coarse_null=False):
        fa, ca, keep = blocks(api, f, c, stream, g_dr)
        extra = change(fa, ca) if change else None
        rc = lib.statmc_upsample_filtered(None if fine_null else C.byref(fa), None if coarse_null else C.byref(ca), k, ch)
        msg = lib.statmc_last_error().decode()
        assert rc == code and word in msg, (rc, code, word, msg)
        del extra

    def set_field(side, **kw):
        def change(fa, ca):
            for name, v in kw.items():
                setattr(fa if side == "fine" else ca, name, v)
        return change

    def image_field(side, table, idx, **kw):
        def change(fa, ca):
            im = getattr(fa if side == "fine" else ca, table)[idx]
            for name, v in kw.items():
                setattr(im, name, v)
        return change

    INV, UNS = api.ERR_INVALID, api.ERR_UNSUPPORTED
    refused(INV, "null fine", fine_null=True)
    refused(INV, "null coarse", coarse_null=True)
    for bad in (0, 1, 3, 16):
        refused(INV, "k = %d" % bad, k=bad)
    refused(INV, "channels = 2", ch=2)
    refused(INV, "coarse is 19x12", k=4)
    refused(INV, "n_buffers", set_field("coarse", n_buffers=2))
    refused(INV, "n_g_buffers", set_field("coarse", n_g_buffers=2))
    counts = (C.c_uint8 * 3)(3, 1, 1)
    refused(INV, "g_channel_counts[1]", set_field("coarse", g_channel_counts=counts))
    null_img, null_u8, null_f = C.POINTER(api.Image)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_float)()
    refused(INV, "fine: null G-buffer table", set_field("fine", g_dr_factors=null_f))
    refused(INV, "coarse: null G-buffer table", set_field("coarse", g_buffers=null_img))
    refused(INV, "fine: null mean_corr", set_field("fine", mean_corr=null_img))
    refused(INV, "coarse: null mean_corr", set_field("coarse", discriminator=null_img))
    refused(INV, "fine: null film", set_field("fine", film_filtered=null_img))
    refused(INV, "coarse: null film_filtered", set_field("coarse", film_filtered=null_img))
    refused(INV, "fine->discriminator[0]: null", image_field("fine", "discriminator", 0, data=None))
    refused(INV, "coarse->g_buffers[2]: null", image_field("coarse", "g_buffers", 2, data=None))
    refused(INV, "coarse->mean_corr[0]: 18x12", image_field("coarse", "mean_corr", 0, cols=18))
    refused(INV, "roi [0,38)", set_field("fine", roi_x1=w + 1, roi_y1=4))
    refused(INV, "roi [5,5)", set_field("fine", roi_x0=5, roi_x1=5, roi_y1=4))
    refused(INV, "output 0 overlaps the fine colour", image_field("fine", "film_filtered", 0, data=f["colour"].data_ptr()))
    refused(INV, "output 0 overlaps fine->mean_corr[0]", image_field("fine", "film_filtered", 0, data=f["mean_corr"].data_ptr() + 16))
    refused(INV, "output 0 overlaps the coarse filtered", image_field("coarse", "film_filtered", 0, data=f["out"].data_ptr() + w * h * 12 - 4))
    refused(INV, "output 0 overlaps coarse->g_buffers[1]", image_field("coarse", "g_buffers", 1, data=f["out"].data_ptr()))
    refused(UNS, "fine->packed_inputs", lambda fa, ca: setattr(fa, "packed_inputs", api.image_of(f["colour"])))
    refused(UNS, "coarse->packed_inputs", lambda fa, ca: setattr(ca, "packed_inputs", api.image_of(c["filtered"])))
    refused(UNS, "fine->film[0]: row pitch", image_field("fine", "film", 0, step=w * 12 + 16))
    refused(UNS, "coarse->film_filtered[0]: row pitch", image_field("coarse", "film_filtered", 0, step=19 * 12 + 4))
    three = (C.c_uint8 * 3)(3, 3, 3)

    def three_rgb(fa, ca):
        fa.g_channel_counts = ca.g_channel_counts = three
    refused(UNS, "more than two RGB", three_rgb)
    spec(dof=api.DOF_WELCH)
    refused(UNS, "STATMC_DOF_WELCH")
    spec()
    torch.cuda.synchronize()
    gpu.check(lib.statmc_synchronize(stream))
    assert (f["out"].cpu().numpy() == SENTINEL).all()
    # ... and the same blocks, untouched, are a valid call
    got = run(gpu, stream, f, c, k, 3, g_dr)
    assert not (got == SENTINEL).any()


# ---------------------------------------------------------------- end to end
def synthetic_film(gpu, w, h, spp, fused):
    import torch
    from statmc_amd import film, synthetic
    scene = synthetic.Scene(w, h, n_regions=6, seed=1)
    smp = scene.samples(spp, seed=101, features=("radiance", "normal", "albedo"))
    fs = film.FilmStats(w, h, torch.device(DEV), filter_sd=FILTER_SD, radius=RADIUS, g_sds=[SD_NORMAL, SD_ALBEDO], fused_prepass=fused)
    fs.accumulate({t: v.to(DEV) for t, v in smp.items()})
    return fs


@pytest.mark.parametrize("fused", [False, True], ids=["prepass", "fused_epilogue"])
def test_preview_is_its_four_steps_by_hand_and_only_reads_the_film(gpu, fused):
    """80 x 48 synthetic film at 8 spp: FilmStats.preview(2) leaves the bits of pooled(2), the coarse pre-pass and window filter, the
    fine pre-pass and the upsample called one by one; every statistics plane of the fine film keeps its bits; a second preview reuses
    the coarse film it kept."""
    import torch
    w, h, k = 80, 48, 2
    fs = synthetic_film(gpu, w, h, 8, fused)
    before = {(t, f): v.clone() for t, st in fs.state.items() for f, v in st.items() if v is not None}
    coarse = fs.pooled(k)
    coarse.prepass()
    coarse.window_filter()
    fs.prepass()
    fa, keep_f = fs.filter_args()
    ca, keep_c = coarse.filter_args()
    fs.film_f.fill_(float(SENTINEL))
    gpu.upsample_filtered(fa, ca, k, 3)
    torch.cuda.synchronize()
    by_hand = fs.film_f.clone()
    assert not (by_hand == float(SENTINEL)).any() and torch.isfinite(by_hand).all()
    for again in range(2):
        fs.film_f.fill_(float(SENTINEL))
        out = fs.preview(k)
        torch.cuda.synchronize()
        assert out is fs.film_f and tuple(out.shape) == (h, w, 3)
        assert np.array_equal(bits(out), bits(by_hand)), again
    assert list(fs._previews) == [k] and (fs._previews[k].width, fs._previews[k].height) == (40, 24)
    for (t, f), v in before.items():
        assert np.array_equal(bits(fs.state[t][f]), bits(v)), (t, f)
    # the preview is a denoised image: closer to the full filter's result than the noisy colour is
    full = fs.denoise().clone()
    noisy = fs.state["radiance"]["film_mean"]
    assert float((by_hand - full).norm()) < float((noisy - full).norm())
    with pytest.raises(ValueError):
        fs.upsample_from(coarse, 4)


def test_offline_tool_upsamples_a_pooled_dump(gpu, stream, tmp_path):
    """statmc_denoise --pool 2 --upsample on a small dump of the synthetic film writes a W x H film-f: the bits of the same steps --
    pool, coarse filter, fine pre-pass, upsample -- through the Python binding on the dump's images ("film" is the colour).  Without
    --upsample the tool writes the coarse film-f it always wrote."""
    import torch
    from statmc_amd import build, pfm
    api = gpu
    exe = build.build_tools()
    w, h, S, k = 80, 48, 8, 2
    wc, hc = api.pooled_size(w, h, k)
    fs = synthetic_film(gpu, w, h, S, False)
    rad = fs.state["radiance"]
    film, normal, albedo = rad["film_mean"], fs.state["normal"]["mean"], fs.state["albedo"]["mean"]
    stem, out = str(tmp_path / "fine"), str(tmp_path / "up")
    dump = {"film": film, "t0-b0-n": rad["n"], "t0-b0-mean": rad["mean"], "t0-b0-m2": rad["m2"], "t0-b0-m3": rad["m3"],
            "t1-b0-film-mean": normal, "t2-b0-film-mean": albedo}
    for name, t in dump.items():
        pfm.write_pfm("%s-%d-%s.pfm" % (stem, S, name), t.cpu().numpy())
    common = [exe, "--stem", stem, "--spp", str(S), "--pool", str(k), "--filtersd", str(FILTER_SD), "--filterradius", str(RADIUS), "--output", "film-f"]
    r = subprocess.run(common + ["--output-stem", out, "--upsample"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = pfm.read_pfm("%s-%d-film-f.pfm" % (out, S)).astype(F32)
    assert got.shape[:2] == (h, w)
    # the same steps by hand.  The C++ host forms a G-buffer's factor in float, -.5f / (sd * sd): an ulp from the double quotient the
    # Python helpers round, which the range weight of this entry sees (e = fma(dr, dist2, e)) -- so the factors are passed as the tool has them
    g_dr = [float(F32(-0.5) / (F32(sd) * F32(sd))) for sd in (SD_NORMAL, SD_ALBEDO)]
    z = lambda hh, ww, c=3: torch.zeros((hh, ww, c) if c else (hh, ww), dtype=torch.float32, device=DEV)
    d_rad = dict(n=torch.zeros(hc, wc, dtype=torch.int32, device=DEV), mean=z(hc, wc), m2=z(hc, wc), m3=z(hc, wc))
    d_film, d_normal, d_albedo = ({"mean": z(hc, wc)} for _ in range(3))
    api.pool_statistics(w, h, k, [api.make_pool_entry(d_rad, {key: rad[key] for key in ("n", "mean", "m2", "m3")}, 3, 3),
                                  api.make_pool_entry(d_normal, {"mean": normal}, 3, 1, count_of=0),
                                  api.make_pool_entry(d_albedo, {"mean": albedo}, 3, 1, count_of=0),
                                  api.make_pool_entry(d_film, {"mean": film}, 3, 1, count_of=0)])
    cmc, cdc, cff = z(hc, wc), z(hc, wc), z(hc, wc)
    ca, keep_c = api.make_filter_args(n=[d_rad["n"]], mean=[d_rad["mean"]], m2=[d_rad["m2"]], m3=[d_rad["m3"]], film=[d_film["mean"]],
                                      mean_corr=[cmc], disc=[cdc], film_filtered=[cff], g_buffers=[d_normal["mean"], d_albedo["mean"]],
                                      g_dr=g_dr, filter_sd=FILTER_SD, radius=RADIUS)
    api.filter_f32x3(ca)
    mc, dc, ff = z(h, w), z(h, w), z(h, w)
    fa, keep_f = api.make_filter_args(n=[rad["n"]], mean=[rad["mean"]], m2=[rad["m2"]], m3=[rad["m3"]], film=[film], mean_corr=[mc], disc=[dc],
                                      film_filtered=[ff], g_buffers=[normal, albedo], g_dr=g_dr, filter_sd=FILTER_SD, radius=RADIUS)
    api.prepass(fa, 3)
    api.upsample_filtered(fa, ca, k, 3)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(ff)) and np.isfinite(got).all()
    # without --upsample: the coarse film-f, as before
    r = subprocess.run(common + ["--output-stem", str(tmp_path / "coarse")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    low = pfm.read_pfm("%s-%d-film-f.pfm" % (str(tmp_path / "coarse"), S)).astype(F32)
    assert low.shape[:2] == (hc, wc) and np.array_equal(bits(low), bits(cff))
    r = subprocess.run([exe, "--stem", stem, "--spp", str(S), "--upsample"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--upsample" in r.stderr
