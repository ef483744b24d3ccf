"""statmc_accumulate_formats: sample arenas given as IEEE half.  The yardstick everywhere is two films warmed identically, one fed
the half arena through the new entry, the other fed half.float() through statmc_accumulate: every plane of every type (and
mean_corr / disc where the epilogue is on) compared as int32 bits, and the launch asked which loader read its 16-bit arenas (a
comparison against a launch that had silently fallen back would prove nothing).  Shapes: the smallest at which each mechanism can
break."""
import functools
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SET9 = ("radiance", "normal", "albedo")
SET11 = ("radiance", "normal", "albedo", "depth", "materialid")
ORDERS = {SET9: ("normal", "radiance", "albedo"), SET11: ("depth", "normal", "materialid", "radiance", "albedo")}
RINGS = (5, 6)    # rows in flight per wave of the fused 16-bit walk: features half (acc_fused_depth(1)), all half (2)
BATCHES = sorted({s for d in RINGS for s in (1, d - 1, d, d + 1, d + 2, 3 * d)})
# which types are handed over as half
MIXES = {"all_half": lambda t: True, "features_half": lambda t: t != "radiance", "radiance_half": lambda t: t == "radiance"}


@functools.lru_cache(maxsize=None)
def samples(W, H, S, seed=7):
    """{type: [S, H, W, C]} fp32 holding half values: positive radiance with exact zeros and a few large values, features in
    [0, 1), rounded to half first so that both sides see the same values.  Computed once per shape."""
    from statmc_amd import synthetic
    g = torch.Generator(device=DEV).manual_seed(seed + 1000 * W + H)
    out = {}
    for t in SET11:
        x = torch.rand(S, H, W, synthetic.CHANNELS[t], device=DEV, generator=g)
        if t == "radiance":
            x = torch.where(x < 0.2, torch.zeros_like(x), x * 3.0)
            x = torch.where(x > 2.99, x * 400.0, x)
        out[t] = x.half().float()
    return out


def cut(smp, types, a, b):
    return {t: smp[t][a:b].contiguous() for t in types}


def as_given(smp, mix):
    """The batch as the renderer holds it: the types of the mix as half arenas (exact: the values are halves already)."""
    return {t: (x.half() if MIXES[mix](t) else x) for t, x in smp.items()}


def new_film(gpu, W, H, types, epilogue, warm=2):
    from statmc_amd import film
    fs = film.FilmStats(W, H, DEV, types=types, fused_prepass=epilogue)
    if warm:
        fs.accumulate(cut(samples(W, H, warm, seed=3), types, 0, warm))
    return fs


def assert_same_bits(fa, fb, epilogue):
    torch.cuda.synchronize()
    for t in fa.types:
        for k, v in fa.state[t].items():
            if v is not None:
                assert torch.equal(v.view(torch.int32), fb.state[t][k].view(torch.int32)), (t, k)
    if epilogue:
        assert torch.equal(fa.mean_corr.view(torch.int32), fb.mean_corr.view(torch.int32)), "mean_corr"
        assert torch.equal(fa.disc.view(torch.int32), fb.disc.view(torch.int32)), "disc"


def launch_half(gpu, fs, smp, rows=None, fused=0, blocks=0, dma=1):
    """One launch through the new entry; returns (loader, fused, workgroups)."""
    lib = gpu.load()
    gpu.accumulate_fused(fused)
    gpu.accumulate_resident_blocks(blocks)
    gpu.accumulate_dma(dma)
    try:
        fs.accumulate(smp, rows=rows)
        return gpu.last_accumulate_loader(), gpu.last_accumulate_fused(), lib.statmc_debug_last_accumulate_grid()
    finally:
        gpu.accumulate_fused(0)
        gpu.accumulate_resident_blocks(0)
        gpu.accumulate_dma(1)


def both_ways(gpu, W, H, types, S, mix, epilogue, prepare=None, rows=None, loader=1, is_fused=None, **how):
    smp = cut(samples(W, H, S), types, 0, S)
    fa, fb = new_film(gpu, W, H, types, epilogue), new_film(gpu, W, H, types, epilogue)
    if prepare is not None:
        prepare(fa)
        prepare(fb)
    got_loader, got_fused, grid = launch_half(gpu, fa, as_given(smp, mix), rows=rows, **how)
    fb.accumulate(smp, rows=rows)                       # statmc_accumulate, the shipped dispatch
    assert gpu.last_accumulate_loader() == 0
    assert got_loader == loader, (got_loader, loader)
    if is_fused is not None:
        assert got_fused == is_fused, (got_fused, is_fused)
    assert_same_bits(fa, fb, epilogue and rows is None)
    if rows is None:
        for t in types:
            assert int(fa.state[t]["n"].min()) >= 2 + S
    return grid


def fused_expected(mix, W=256, H=4):
    """The fused 16-bit walk serves launches whose features are all half (the radiance type in either format) on films whose
    half rows are 16-byte aligned: a multiple of 8 pixels."""
    return 1 if mix != "radiance_half" and (W * H) % 8 == 0 else 0


@pytest.mark.parametrize("S", BATCHES)
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("types", [SET9, SET11], ids=["9ch", "11ch"])
def test_one_workgroup_of_full_waves(gpu, types, mix, S):
    """256 x 4 pixels: one workgroup, four full waves; batches around both ring depths; epilogue on and off; the radiance type
    first in the list and not."""
    for epilogue in (False, True):
        for order in (types, ORDERS[types]):
            both_ways(gpu, 256, 4, order, S, mix, epilogue, is_fused=fused_expected(mix))


@pytest.mark.parametrize("mix", list(MIXES))
def test_partial_wave_beside_idle_waves(gpu, mix):
    """252 x 5 pixels: 315 groups -- the second workgroup holds one wave of 59 lanes and three waves with nothing to do (1260
    pixels are no multiple of 8: the per-type 16-bit kernel); 248 x 5: 310 groups, a wave of 54 lanes inside the fused walk."""
    for epilogue in (False, True):
        both_ways(gpu, 252, 5, SET11, 7, mix, epilogue, is_fused=0)
        both_ways(gpu, 248, 5, SET11, 7, mix, epilogue, is_fused=fused_expected(mix, 248, 5))


@pytest.mark.parametrize("mix", list(MIXES))
def test_grid_stride_walk_starts_clean_on_every_pass(gpu, mix):
    """512 x 6 pixels: 768 groups = three units on ONE workgroup."""
    assert both_ways(gpu, 512, 6, SET11, 8, mix, True, blocks=1, is_fused=fused_expected(mix)) == 1
    assert both_ways(gpu, 512, 6, ORDERS[SET9], 8, mix, False, blocks=1, is_fused=fused_expected(mix)) == 1


@pytest.mark.parametrize("mix", ["all_half", "features_half"])
def test_forced_paths(gpu, mix):
    """The fused 16-bit walk forced on, forced off (the per-type 16-bit kernel), and the launch with the LDS-DMA rows switched off
    (the per-type kernel as well: its half rows come by register loads)."""
    for W, H, S in ((256, 4, 7), (252, 5, 6), (248, 5, 6), (512, 6, 8)):
        for types in (SET11, ORDERS[SET9]):
            both_ways(gpu, W, H, types, S, mix, True, fused=1, is_fused=fused_expected(mix, W, H))
            both_ways(gpu, W, H, types, S, mix, True, fused=-1, is_fused=0)
    both_ways(gpu, 256, 4, SET11, 7, mix, True, dma=0, is_fused=0)
    both_ways(gpu, 512, 6, SET11, 7, mix, False, fused=-1, blocks=1, is_fused=0)


@pytest.mark.parametrize("ragged_type", ["radiance", "albedo", "depth"])
def test_ragged_counts_inside_a_group(gpu, ragged_type):
    """One type's counts differ inside one 4-pixel group of the second wave: the existing ragged walk, on widened values."""
    def ragged(fs):
        fs.state[ragged_type]["n"][1, 41] += 2       # pixel 297: group 74, the second wave of the workgroup
    for mix in MIXES:
        both_ways(gpu, 256, 4, SET11, 7, mix, True, prepare=ragged, is_fused=fused_expected(mix))
    both_ways(gpu, 256, 4, SET11, 7, "all_half", True, prepare=ragged, fused=-1, is_fused=0)


def test_types_starting_from_different_counts(gpu):
    """The radiance type has seen three samples more than the features."""
    def radiance_alone(fs):
        fs.accumulate(cut(samples(256, 4, 3, seed=11), ("radiance",), 0, 3))
    for mix in MIXES:
        for types in (SET11, ORDERS[SET9]):
            both_ways(gpu, 256, 4, types, 7, mix, True, prepare=radiance_alone, is_fused=fused_expected(mix))


@pytest.mark.parametrize("rows", [(1, 3), [(0, 1), (2, 4)]], ids=["one_range", "two_ranges"])
def test_row_ranges(gpu, rows):
    """Rows outside the ranges keep every bit; rows inside hold what statmc_accumulate_rows / _row_ranges leave."""
    W, H, S = 256, 4, 7
    ranges = [rows] if not hasattr(rows[0], "__len__") else rows
    inside = torch.zeros(H, dtype=torch.bool)
    for y0, y1 in ranges:
        inside[y0:y1] = True
    for mix in MIXES:
        smp = cut(samples(W, H, S), SET11, 0, S)
        fa, fb = new_film(gpu, W, H, SET11, False), new_film(gpu, W, H, SET11, False)
        before = {t: {k: v.clone() for k, v in fa.state[t].items() if v is not None} for t in SET11}
        loader, _, _ = launch_half(gpu, fa, as_given(smp, mix), rows=rows)
        fb.accumulate(smp, rows=rows)
        assert loader == 1
        assert_same_bits(fa, fb, False)
        for t in SET11:
            for k, v in before[t].items():
                assert torch.equal(v[~inside].view(torch.int32), fa.state[t][k][~inside].view(torch.int32)), (t, k)
            assert int(fa.state[t]["n"][inside].min()) == 2 + S and int(fa.state[t]["n"][~inside].max()) == 2


@pytest.mark.parametrize("W,H", [(5, 3), (7, 1)])
def test_small_odd_films_take_the_fallback(gpu, W, H):
    for mix in MIXES:
        for epilogue in (False, True):
            both_ways(gpu, W, H, SET11, 6, mix, epilogue, loader=2, is_fused=0)


def test_arena_one_element_past_an_aligned_address(gpu):
    """A 256 x 4 film whose half arenas start 2 bytes past an aligned address: the loader reads 2, and the bits match."""
    W, H, S = 256, 4, 7
    smp = cut(samples(W, H, S), SET11, 0, S)
    for mix in ("all_half", "features_half"):
        given, keep = {}, []
        for t, x in as_given(smp, mix).items():
            if x.dtype == torch.float16:
                buf = torch.zeros(x.numel() + 8, dtype=torch.float16, device=DEV)
                buf[1:1 + x.numel()] = x.reshape(-1)
                keep.append(buf)
                x = buf[1:1 + x.numel()].view(x.shape)
                assert x.data_ptr() % 8 == 2
            given[t] = x
        fa, fb = new_film(gpu, W, H, SET11, True), new_film(gpu, W, H, SET11, True)
        loader, fused, _ = launch_half(gpu, fa, given)
        fb.accumulate(smp)
        assert (loader, fused) == (2, 0)
        assert_same_bits(fa, fb, True)


def finite_halves():
    bits = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
    assert bits.size == 63488
    return bits


def planes(bits, n_elems):
    """[S = 2] planes of n_elems halves each: the patterns repeated (or followed by zeros), and the same reversed."""
    reps = n_elems // bits.size
    first = np.concatenate([np.tile(bits, reps), np.zeros(n_elems - reps * bits.size, np.uint16)])
    return np.stack([first, first[::-1]]).view(np.float16)


@pytest.mark.parametrize("case", ["one_channel", "rgb", "fallback", "fused_walk"])
def test_every_finite_half(gpu, case):
    """All 63 488 finite bit patterns as the samples of a non-transform, mean-only type, from a zero state, S = 1 and S = 2 (the
    second sample: the patterns reversed); the other side is widened by numpy.  Catches a flushed subnormal or a wrong half-word
    select.  fused_walk: the same patterns as the features of a launch that carries a radiance type, i.e. through the LDS-DMA rows."""
    from statmc_amd import film
    bits = finite_halves()
    W, H = (249, 255) if case == "fallback" else (248, 256)
    types = {"one_channel": ("depth",), "rgb": ("normal",), "fallback": ("depth", "normal"), "fused_walk": ("radiance", "normal", "depth")}[case]
    for S in (1, 2):
        given, wide = {}, {}
        for t in types:
            c = film.STAT_TYPES[t]["channels"]
            if t == "radiance":
                h = samples(W, H, S)["radiance"][:S].half().cpu().numpy()
            else:
                h = planes(bits, W * H * c)[:S].reshape(S, H, W, c)
            given[t] = torch.from_numpy(np.ascontiguousarray(h)).to(DEV)
            wide[t] = torch.from_numpy(h.astype(np.float32)).to(DEV)
            assert given[t].dtype == torch.float16
        fa, fb = new_film(gpu, W, H, types, False, warm=0), new_film(gpu, W, H, types, False, warm=0)
        loader, fused, _ = launch_half(gpu, fa, given)
        fb.accumulate(wide)
        assert loader == (2 if case == "fallback" else 1) and fused == (1 if case == "fused_walk" else 0)
        assert_same_bits(fa, fb, False)
        if S == 1 and case != "fused_walk":     # one sample from a zero state: the mean IS the widened sample (0 + -0 = +0)
            t = types[0]
            assert torch.equal(fa.state[t]["mean"].view(torch.int32), (wide[t][0] + 0.0).view(torch.int32))


def test_all_fp32_through_the_new_entry_is_the_existing_call(gpu):
    from statmc_amd import film
    lib = gpu.load()
    W, H, S = 256, 4, 7
    smp = cut(samples(W, H, S), SET11, 0, S)
    fa, fb, fc = (new_film(gpu, W, H, SET11, True) for _ in range(3))
    def types_of(fs):
        return [gpu.make_stat_type(smp[t], fs.state[t], film.STAT_TYPES[t]["transform"], film.STAT_TYPES[t]["max_moment"],
                                   prepass_into=(fs.mean_corr, fs.disc) if t == "radiance" else None) for t in SET11]
    gpu.accumulate(W, H, types_of(fa))
    grids = [lib.statmc_debug_last_accumulate_grid()]
    gpu.accumulate(W, H, types_of(fb), sample_formats=[gpu.SAMPLES_F32] * 5)
    grids.append(lib.statmc_debug_last_accumulate_grid())
    assert gpu.last_accumulate_loader() == 0
    arr = (gpu.StatType * 5)(*types_of(fc))
    gpu.check(lib.statmc_accumulate_formats(W, H, arr, None, 5, None, 0, gpu.current_stream_handle()))
    grids.append(lib.statmc_debug_last_accumulate_grid())
    assert gpu.last_accumulate_loader() == 0
    assert grids[0] == grids[1] == grids[2]
    assert_same_bits(fa, fb, True)
    assert_same_bits(fa, fc, True)


def test_film_stats_refuses_other_dtypes(gpu):
    fs = new_film(gpu, 8, 4, SET9, False, warm=0)
    smp = {t: torch.zeros(1, 4, 8, 3, dtype=torch.bfloat16, device=DEV) for t in SET9}
    with pytest.raises(TypeError):
        fs.accumulate(smp)


@pytest.mark.parametrize("W,H", [(61, 37), (96, 64)])
def test_estimator_accumulate_film_equals_merge_tiles(gpu, W, H):
    """include/statmc_denoiser.hpp: an Estimator fed through AccumulateFilm with half features and fp32 radiance holds the bits of
    one fed the widened samples through Merge*Tile and denoises to the same film-f; before EnableDeviceAccumulation() the call
    throws (tests/cpp/test_accumulate_film.cpp)."""
    from statmc_amd import build
    build.build_tools()
    r = subprocess.run([build.ACC_FILM_BIN, str(W), str(H)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"OK" in r.stdout
