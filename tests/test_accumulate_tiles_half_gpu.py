"""statmc_accumulate_tiles_formats: tile arenas given as IEEE half.  The yardstick throughout is api.accumulate_tiles on fp32
arenas that hold the widened halves, with the same tables and the same non-zero starting state: every plane of every type
compared as int32 bits.  A case (film, tile table, samples, warmed state) and its fp32 reference are computed once and shared by
the mixes, loaders and orders that are compared against it; neither is written to afterwards.  Shapes: the smallest at which
each path of the half tile kernel can go wrong."""
import ctypes as C
import functools
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SET9 = ("radiance", "normal", "albedo")
SET11 = ("radiance", "normal", "albedo", "depth", "materialid")
MIXES = {"features_half": lambda t: t != "radiance", "all_half": lambda t: True,
         "irregular": lambda t: t in ("radiance", "depth")}           # radiance half, albedo (and normal) fp32, depth half
PLANES = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
RING = 3                                                              # kAccTilesDmaD: slots per wave; a half slot holds two samples


def cfg(t):
    from statmc_amd import film
    c = film.STAT_TYPES[t]
    return c["channels"], c["transform"], c["max_moment"]


def tile_table(W, H, counts, T=16, shift=0):
    """16 x 16 tiles in row order, tile k with counts[k] samples (an int: every tile); blocks start on 4-pixel-sample boundaries,
    or -- shift 1 .. 3 -- `shift` past one."""
    tiles = [(x, y, min(x + T, W), min(y + T, H)) for y in range(0, H, T) for x in range(0, W, T)]
    if isinstance(counts, int):
        counts = (counts,) * len(tiles)
    assert len(counts) == len(tiles), (len(counts), len(tiles))
    offsets, off = [], shift
    for (x0, y0, x1, y1), S in zip(tiles, counts):
        offsets.append(off)
        off += (S * (x1 - x0) * (y1 - y0) + 3) // 4 * 4
    return tiles, list(counts), offsets, off


@functools.lru_cache(maxsize=None)
def case(W, H, types, counts, shift=0, warm=2, seed=11):
    """The device tables, one fp32 arena of half values per type, and the state the launches start from: zeros, or `warm`
    samples per pixel folded by the fp32 entry (so that the counts, moments and film chain are non-zero)."""
    from statmc_amd import api, film
    api.setup(0)
    tiles, counts, offsets, total = tile_table(W, H, counts, shift=shift)
    g = torch.Generator(device=DEV).manual_seed(seed + 1000 * W + H + 7 * total)
    arenas = {}
    for t in types:
        c = cfg(t)[0]
        x = torch.rand(total * c, device=DEV, generator=g)
        if t == "radiance":                                           # exact zeros, a few large values
            x = torch.where(x < 0.2, torch.zeros_like(x), x * 3.0)
            x = torch.where(x > 2.99, x * 400.0, x)
        arenas[t] = x.half().float()
    tab = dict(bounds=torch.tensor(tiles, dtype=torch.int32, device=DEV), offsets=torch.tensor(offsets, dtype=torch.int64, device=DEV),
               samples=torch.tensor(counts, dtype=torch.int32, device=DEV))
    state = {t: film.new_state(H, W, cfg(t)[0], DEV, cfg(t)[1]) for t in types}
    if warm:
        wt, wc, wo, wtotal = tile_table(W, H, warm)
        sts = [api.make_stat_type_arena((torch.rand(wtotal * cfg(t)[0], device=DEV, generator=g) * 2).half().float(), cfg(t)[0], state[t],
                                        cfg(t)[1], cfg(t)[2]) for t in types]
        api.accumulate_tiles(W, H, sts, torch.tensor(wt, dtype=torch.int32, device=DEV), torch.tensor(wo, dtype=torch.int64, device=DEV),
                             torch.tensor(wc, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
    return dict(W=W, H=H, types=types, tiles=tiles, counts=counts, offsets=offsets, arenas=arenas, tab=tab, state=state)


def fresh(cs, epilogue):
    st = {t: {k: (v.clone() if v is not None else None) for k, v in s.items()} for t, s in cs["state"].items()}
    pre = (torch.full((cs["H"], cs["W"], 3), -7.0, device=DEV), torch.full((cs["H"], cs["W"], 3), -7.0, device=DEV)) if epilogue else None
    return st, pre


def launch(cs, arenas, formats, epilogue=False):
    """One launch on a copy of the case's state; arenas: {type: flat tensor}; formats: None (the existing entry) or a list."""
    from statmc_amd import api
    st, pre = fresh(cs, epilogue)
    sts = [api.make_stat_type_arena(arenas[t], cfg(t)[0], st[t], cfg(t)[1], cfg(t)[2], prepass_into=pre if t == "radiance" else None)
           for t in cs["types"]]
    api.accumulate_tiles(cs["W"], cs["H"], sts, cs["tab"]["bounds"], cs["tab"]["offsets"], cs["tab"]["samples"], sample_formats=formats)
    torch.cuda.synchronize()
    return st, pre


@functools.lru_cache(maxsize=None)
def reference(W, H, types, counts, shift=0, warm=2, epilogue=False):
    """The yardstick: the existing entry on the widened arenas, default switches."""
    cs = case(W, H, types, counts, shift, warm)
    return launch(cs, cs["arenas"], None, epilogue)


def half_arena(x, byte_shift=0):
    """x.half() at an address 16-byte aligned (torch's), or 2 bytes past one (every half type element by element), or 8 bytes
    past one (the 8-byte pieces of the register loader are aligned, the 16-byte rows of the ring are not)."""
    if not byte_shift:
        return x.half()
    assert byte_shift in (2, 8)
    buf = torch.empty(x.numel() + 8, dtype=torch.float16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[byte_shift // 2:byte_shift // 2 + x.numel()]
    out.copy_(x)
    assert out.data_ptr() % 16 == byte_shift
    return out


def run_half(W, H, types, counts, mix, shift=0, warm=2, epilogue=False, byte_shift=0):
    from statmc_amd import api
    cs = case(W, H, types, counts, shift, warm)
    arenas = {t: (half_arena(x, byte_shift) if MIXES[mix](t) else x) for t, x in cs["arenas"].items()}
    fmts = [api.SAMPLES_F16 if MIXES[mix](t) else api.SAMPLES_F32 for t in types]
    assert api.SAMPLES_F16 in fmts
    return launch(cs, arenas, fmts, epilogue)


def assert_same(got, want, what=""):
    (sa, pa), (sb, pb) = got, want
    for t in sa:
        for k in PLANES:
            if sa[t][k] is not None:
                assert torch.equal(sa[t][k].view(torch.int32), sb[t][k].view(torch.int32)), (what, t, k)
    if pa is not None:
        assert torch.equal(pa[0].view(torch.int32), pb[0].view(torch.int32)), (what, "mean_corr")
        assert torch.equal(pa[1].view(torch.int32), pb[1].view(torch.int32)), (what, "discriminator")


def both(W, H, types, counts, mix, **kw):
    ref_kw = {k: v for k, v in kw.items() if k != "byte_shift"}
    assert_same(run_half(W, H, types, counts, mix, **kw), reference(W, H, types, counts, **ref_kw), (W, H, counts, mix))


# ---- 1. one workgroup of full tiles
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("types", [SET9, SET11], ids=["9ch", "11ch"])
def test_one_workgroup_of_full_tiles(gpu, types, mix):
    """32 x 32, four 16 x 16 tiles: an odd run with no partner row, an even run, an odd run longer than the ring, an untouched
    tile -- and every tile at one below, at and above what a ring of two-sample slots holds."""
    both(32, 32, types, (1, 2, 7, 0), mix)
    ref, cs = reference(32, 32, types, (1, 2, 7, 0)), case(32, 32, types, (1, 2, 7, 0))
    x0, y0, x1, y1 = cs["tiles"][3]
    for t in types:                                                    # the tile without samples keeps every bit
        for k in PLANES:
            if cs["state"][t][k] is not None:
                assert torch.equal(ref[0][t][k][y0:y1, x0:x1], cs["state"][t][k][y0:y1, x0:x1]), (t, k)
        assert int(ref[0][t]["n"][0, 0]) == 2 + 1 and int(ref[0][t]["n"][16, 0]) == 2 + 7
    for S in (2 * RING - 3, 2 * RING - 1, 2 * RING, 2 * RING + 1, 2 * RING + 2):     # 3, 5, 6, 7, 8
        both(32, 32, types, S, mix)


# ---- 2. partial tiles in the cooperative walk
@pytest.mark.parametrize("mix", list(MIXES))
def test_partial_tiles(gpu, mix):
    """40 x 24: tiles 8 wide (32 four-pixel groups) and 8 high beside full ones."""
    both(40, 24, SET11, (7, 3, 1, 4, 2, 6), mix)
    both(40, 24, SET9, 5, mix, epilogue=True)
    # 44 x 21: tiles of 12 x 16 (48 groups), 16 x 5 (20) and 12 x 5 -- 15 groups, rows that are no whole number of 16-byte pieces:
    # the ring is not for them
    both(44, 21, SET11, (7, 2, 5, 3, 6, 1), mix, epilogue=True)


# ---- 3. the element path: the same bits
@pytest.mark.parametrize("mix", list(MIXES))
def test_element_path(gpu, mix):
    """A film whose width is no multiple of 4; blocks that start off the 4-pixel-sample grid; an arena 2 bytes past an aligned
    address."""
    n_tiles = 4 * 3
    both(50, 37, SET11, tuple((1, 2, 7, 0, 3, 5)[k % 6] for k in range(n_tiles)), mix, epilogue=True)
    for shift in (1, 2, 3):
        both(32, 32, SET11, (1, 2, 7, 0), mix, shift=shift)
    for byte_shift in (2, 8):
        both(32, 32, SET11, (1, 2, 7, 0), mix, byte_shift=byte_shift)
        both(40, 24, SET9, 5, mix, byte_shift=byte_shift, epilogue=True)


# ---- 4. a wave that walks more than one item
def test_wave_walks_several_items(gpu):
    """256 x 256, five types, 3 samples, one workgroup per CU: 1280 items on at most 1024 waves."""
    lib = gpu.load()
    lib.statmc_debug_accumulate_tiles_variant.argtypes = [C.c_int] * 3
    ref = reference(256, 256, SET11, 3)
    try:
        gpu.check(lib.statmc_debug_accumulate_tiles_variant(2, 2, 1))
        for mix in MIXES:
            assert_same(run_half(256, 256, SET11, 3, mix), ref, mix)
    finally:
        gpu.check(lib.statmc_debug_accumulate_tiles_variant(2, 2, 0))


# ---- 5. both loaders, every order
@pytest.mark.parametrize("mix", list(MIXES))
def test_loaders_and_orders(gpu, mix):
    lib = gpu.load()
    lib.statmc_debug_accumulate_tiles_variant.argtypes = [C.c_int] * 3
    shapes = [(32, 32, SET11, (1, 2, 7, 0)), (32, 32, SET9, 6), (32, 32, SET9, 7), (40, 24, SET11, (7, 3, 1, 4, 2, 6)), (44, 21, SET11, (7, 2, 5, 3, 6, 1))]
    try:
        for dma in (0, 1):
            gpu.accumulate_dma(dma)
            for umul, order in ((2, 2), (2, 0), (2, 1), (1, 2)):
                gpu.check(lib.statmc_debug_accumulate_tiles_variant(umul, order, 0))
                for W, H, types, counts in shapes:
                    assert_same(run_half(W, H, types, counts, mix), reference(W, H, types, counts), (dma, umul, order, W, H))
    finally:
        gpu.accumulate_dma(1)
        gpu.check(lib.statmc_debug_accumulate_tiles_variant(2, 2, 0))


# ---- 6. every finite half
@pytest.mark.parametrize("byte_shift", [0, 2], ids=["vector", "element"])
def test_every_finite_half(gpu, byte_shift):
    """All 63 488 finite halves, one sample each into a fresh state, as 1-channel samples and as RGB: a non-transform mean is
    the widened value (bit for bit; -0, which the fold's 0 + (x - 0) / 1 turns into +0, by value), and every plane of the
    transform type carries the fp32 entry's bits."""
    from statmc_amd import api, film
    W, H = 256, 248
    h = torch.arange(65536, dtype=torch.int32, device=DEV).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h)]
    assert h.numel() == 63488 == W * H
    tiles, counts, offsets, total = tile_table(W, H, 1)
    assert total == W * H
    tab = [torch.tensor(tiles, dtype=torch.int32, device=DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV),
           torch.tensor(counts, dtype=torch.int32, device=DEV)]
    perm = torch.randperm(h.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    one = h[perm].contiguous()
    rgb = torch.stack([one, h, h.flip(0)], dim=1).reshape(-1).contiguous()

    def fold(arenas, formats):
        st = {"depth": film.new_state(H, W, 1, DEV, False), "normal": film.new_state(H, W, 3, DEV, False),
              "radiance": film.new_state(H, W, 3, DEV, True)}
        sts = [api.make_stat_type_arena(arenas["depth"], 1, st["depth"], False, 1), api.make_stat_type_arena(arenas["normal"], 3, st["normal"], False, 1),
               api.make_stat_type_arena(arenas["radiance"], 3, st["radiance"], True, 3)]
        api.accumulate_tiles(W, H, sts, *tab, sample_formats=formats)
        torch.cuda.synchronize()
        return st

    wide = {"depth": one.float(), "normal": rgb.float(), "radiance": rgb.float()}
    got = fold({"depth": half_arena(wide["depth"], byte_shift), "normal": half_arena(wide["normal"], byte_shift),
                "radiance": half_arena(wide["radiance"], byte_shift)}, [api.SAMPLES_F16] * 3)
    want = fold(wide, None)
    assert_same((got, None), (want, None))

    def in_film_order(arena, c):                                       # [tile][y][x][c] blocks -> [H][W][c]
        out = torch.empty(H, W, c, device=DEV)
        for (x0, y0, x1, y1), off in zip(tiles, offsets):
            out[y0:y1, x0:x1] = arena[off * c:(off + (x1 - x0) * (y1 - y0)) * c].view(y1 - y0, x1 - x0, c)
        return out

    for t, c in (("depth", 1), ("normal", 3)):
        x, mean = in_film_order(wide[t], c), got[t]["mean"]
        assert torch.equal(mean, x), t                                 # by value: -0 == +0
        not_minus_zero = x.view(torch.int32) != -2 ** 31
        assert torch.equal(mean.view(torch.int32)[not_minus_zero], x.view(torch.int32)[not_minus_zero]), t
        assert int((~not_minus_zero).sum()) == c
        assert int(got[t]["n"].min()) == int(got[t]["n"].max()) == 1


# ---- 7. the epilogue
@pytest.mark.parametrize("mix", ["all_half", "irregular"])
def test_epilogue_is_the_prepass_of_the_result(gpu, mix):
    """(the mixes in which the radiance type, whose epilogue it is, is half)"""
    from statmc_amd import api
    st, (mc, dc) = run_half(32, 32, SET9, (1, 2, 7, 0), mix, epilogue=True)
    assert_same((st, (mc, dc)), reference(32, 32, SET9, (1, 2, 7, 0), epilogue=True))
    r = st["radiance"]
    mc2, dc2 = torch.zeros_like(r["mean"]), torch.zeros_like(r["mean"])
    args, keep = api.make_filter_args(n=[r["n"]], mean=[r["mean"]], m2=[r["m2"]], m3=[r["m3"]], film=[r["mean"]], mean_corr=[mc2], disc=[dc2],
                                      film_filtered=[torch.zeros_like(mc2)], g_buffers=[])
    api.prepass(args, 3)
    torch.cuda.synchronize()
    live = torch.ones(32, 32, dtype=torch.bool, device=DEV)
    live[16:32, 16:32] = False                                         # the tile without samples: its epilogue did not run
    assert torch.equal(mc.view(torch.int32)[live], mc2.view(torch.int32)[live])
    assert torch.equal(dc.view(torch.int32)[live], dc2.view(torch.int32)[live])
    assert bool((mc[~live] == -7.0).all()) and bool((dc[~live] == -7.0).all())


# ---- 8. fp32 through the new entry
def test_fp32_formats_are_the_existing_call(gpu):
    from statmc_amd import api
    lib = gpu.load()
    for W, H, types, counts in ((32, 32, SET11, (1, 2, 7, 0)), (50, 37, SET9, 3)):
        cs, ref = case(W, H, types, counts), reference(W, H, types, counts)
        assert_same(launch(cs, cs["arenas"], [api.SAMPLES_F32] * len(types)), ref)
        st, _ = fresh(cs, False)                                       # sample_formats == NULL at the C entry itself
        sts = [api.make_stat_type_arena(cs["arenas"][t], cfg(t)[0], st[t], cfg(t)[1], cfg(t)[2]) for t in types]
        arr = (api.StatType * len(sts))(*sts)
        gpu.check(lib.statmc_accumulate_tiles_formats(W, H, arr, None, len(sts), cs["tab"]["bounds"].data_ptr(), cs["tab"]["offsets"].data_ptr(),
                                                      cs["tab"]["samples"].data_ptr(), len(cs["tiles"]), gpu.current_stream_handle()))
        torch.cuda.synchronize()
        assert_same((st, None), ref)


# ---- 9. errors
def test_errors_leave_the_state_alone(gpu):
    from statmc_amd import api
    lib = gpu.load()
    cs = case(32, 32, SET9, (1, 2, 7, 0))
    st, _ = fresh(cs, False)
    arenas = {t: x.half() for t, x in cs["arenas"].items()}
    sts = [api.make_stat_type_arena(arenas[t], cfg(t)[0], st[t], cfg(t)[1], cfg(t)[2]) for t in SET9]
    tabs = (cs["tab"]["bounds"], cs["tab"]["offsets"], cs["tab"]["samples"])
    with pytest.raises(api.StatmcError) as e:
        api.accumulate_tiles(32, 32, sts, *tabs, sample_formats=[1, 2, 1])
    assert e.value.code == api.ERR_INVALID and "sample_formats[1]" in str(e.value)
    sts[2].samples = arenas["albedo"].data_ptr() + 1
    with pytest.raises(api.StatmcError) as e:
        api.accumulate_tiles(32, 32, sts, *tabs, sample_formats=[1, 1, 1])
    assert e.value.code == api.ERR_INVALID and "odd address" in str(e.value)
    torch.cuda.synchronize()
    assert_same((st, None), (cs["state"], None))


# ---- the CPU oracle, fed the widened samples
def test_against_the_oracle(gpu, oracle):
    """Fresh state, features half: n, the feature means and the raw-sample chain bit for bit, the Box-Cox planes to 1e-5."""
    W, H, counts = 32, 32, (1, 2, 7, 0)
    cs = case(W, H, SET11, counts, 0, 0)
    st, _ = run_half(W, H, SET11, counts, "features_half", warm=0)
    assert_same((st, None), reference(W, H, SET11, counts, warm=0))
    for t in SET11:
        c, transform, mm = cfg(t)
        ref = oracle.new_state(H, W, c)
        arena = cs["arenas"][t].cpu().numpy()
        for (x0, y0, x1, y1), S, off in zip(cs["tiles"], cs["counts"], cs["offsets"]):
            if S:
                smp = arena[off * c:(off + S * (x1 - x0) * (y1 - y0)) * c].reshape(S, y1 - y0, x1 - x0, c)
                sub = {k: np.ascontiguousarray(v[y0:y1, x0:x1]) for k, v in ref.items()}
                oracle.accumulate(sub, np.ascontiguousarray(smp), transform, mm)
                for k, v in sub.items():
                    ref[k][y0:y1, x0:x1] = v
        got = {k: v.cpu().numpy() for k, v in st[t].items() if v is not None}
        assert np.array_equal(got["n"], ref["n"]), t
        for k in (("film_mean", "film_m2") if transform else ("mean",)):
            assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), (t, k)
        if transform:
            for k in ("mean", "m2", "m3"):
                assert rel_l2(got[k], ref[k]) <= 1e-5, (t, k)


# ---- 10. the drop-in
@pytest.mark.parametrize("W,H,stage_mb", [(88, 44, 1), (50, 37, 2048)], ids=["vector-tiles-small-staging", "scalar-tiles"])
def test_render_sim_half_features(gpu, oracle, tmp_path, W, H, stage_mb):
    """statmc_render_sim --half-features against the oracle fed the normal and albedo samples rounded to half (as
    tests/test_render_sim_gpu.py compares the fp32 run); the radiance files are those of a run without the flag; the staged
    bytes are 12 + 6 + 6 per pixel-sample with the flag and 36 without."""
    from statmc_amd import build, pfm
    from test_render_sim_gpu import make_samples
    build.build_tools()
    spp, iterations, seed = 4, 3, 5
    stems = {flag: str(tmp_path / ("half" if flag else "full")) for flag in (True, False)}
    staged = {}
    for flag, stem in stems.items():
        out = subprocess.run([build.RENDER_SIM_BIN, "--width", str(W), "--height", str(H), "--spp", str(spp), "--iterations", str(iterations),
                              "--threads", "4", "--seed", str(seed), "--stem", stem, "--stage-mb", str(stage_mb)]
                             + (["--half-features"] if flag else []), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        found = re.findall(r"^Staged bytes: (\d+)$", out.stdout, re.M)
        assert len(found) == 1, out.stdout
        staged[flag] = int(found[0])
    total = spp + sum(spp << (i - 2) for i in range(2, iterations + 1))
    assert staged[True] == W * H * total * 24 and staged[False] == W * H * total * 36
    st = {"nrm": oracle.new_state(H, W, 3), "alb": oracle.new_state(H, W, 3)}
    done = 0
    for i in range(1, iterations + 1):
        target = spp if i == 1 else spp << (i - 2)
        _, nrm, alb = make_samples(seed, W, H, done, target)
        oracle.accumulate(st["nrm"], nrm.astype(np.float16).astype(np.float32), False, 1)
        oracle.accumulate(st["alb"], alb.astype(np.float16).astype(np.float32), False, 1)
        done += target
        rd = lambda flag, name: pfm.read_pfm("%s-%d-%s.pfm" % (stems[flag], done, name))
        assert np.array_equal(rd(True, "t1-b0-n"), st["nrm"]["n"].astype(np.float32))
        assert np.array_equal(rd(True, "t1-b0-mean").view(np.int32), st["nrm"]["mean"].view(np.int32)), i
        assert np.array_equal(rd(True, "t2-b0-mean").view(np.int32), st["alb"]["mean"].view(np.int32)), i
        for name in ("n", "mean", "m2", "m3", "film-mean", "film-m2"):
            assert np.array_equal(rd(True, "t0-b0-" + name).view(np.int32), rd(False, "t0-b0-" + name).view(np.int32)), (i, name)
        assert not np.array_equal(rd(True, "t1-b0-mean"), rd(False, "t1-b0-mean"))     # the rounding did happen
